"""Real captures on the device: mask PNGs (dgm_png_unfilter at one byte per pixel + dgm_png_expand) against Pillow's reading of the
same files, dgm_resample_nearest against Pillow's resize of P and 1 images, dgm_image_ingest_masked against tests/_capture_ref.py,
Scene on a written scene of each layout (tests/_capture_fixture.py), and a short training run across dpsr_iter on the iPhone one."""
import os

import numpy as np
import pytest
import torch

import _capture_fixture as F
import _capture_ref as CR
import _png_ref
import _resample_ref as RR
from conftest import pkg

KINDS = ("Nerfies", "iPhone", "NeuralActor")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return F.golden()


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    out = {}
    for kind in KINDS:
        root = str(tmp_path_factory.mktemp(kind))
        out[kind] = (root, F.write_scene(root, pkg("synthetic"), kind))
    return out


def as_bytes(pixels):
    """np.asarray(Image.open(file)) as the decoder's (H, W, C) bytes: mode 1's bools are the grey samples 0 and 255."""
    a = np.asarray(pixels)
    a = a.astype(np.uint8) * 255 if a.dtype == bool else a
    return a[..., None] if a.ndim == 2 else a


@pytest.mark.gpu
def test_mask_files_decode_bit_exact(gold, tmp_path):
    """Every golden file in one decode_mask_groups call, the 67 x 70 ones twice (groups of two)."""
    P = pkg("png_io")
    keys = sorted(k[:-4] for k in gold.files if k.endswith("/png"))
    order = keys + [k for k in keys if "67x70" in k]
    paths = []
    for k in order:
        paths.append(str(tmp_path / f"{len(paths)}.png"))
        with open(paths[-1], "wb") as fh:
            fh.write(gold[k + "/png"].tobytes())
    groups = P.decode_mask_groups(paths, DEV)
    torch.cuda.synchronize()
    assert sorted(i for idx, _, _ in groups for i in idx) == list(range(len(paths)))
    assert sorted(len(idx) for idx, _, _ in groups).count(2) == 8
    for idx, batch, kind in groups:
        assert batch.dtype == torch.uint8 and batch.shape[0] == len(idx) and batch.is_cuda
        got = batch.cpu().numpy()
        for k, i in enumerate(idx):
            flavour = order[i].split("/")[1]
            assert kind == {"1": "index", "L": "grey", "RGB": "rgb", "RGBA": "rgba"}.get(flavour, "index"), order[i]
            want = as_bytes(gold[order[i] + "/pixels"])
            assert got[k].shape == want.shape and np.array_equal(got[k], want), order[i]
            assert np.array_equal(got[k][..., 0] > 0, gold[order[i] + "/gt0"]), order[i]


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1, 1), (17, 1), (1, 9), (67, 70), (300, 5), (3, 1100)])
def test_unfilter_one_byte_per_pixel(W, H):
    """Every content under every filter choice at one byte per pixel, in one batched call."""
    from test_ingest_kernels import contents, filter_choices, run_unfilter
    rng = np.random.RandomState(W * 5 + H)
    pixels, filtered = [], []
    for px in contents(rng, H, W, 1).values():
        for types in filter_choices(rng, H):
            pixels.append(px)
            filtered.append(_png_ref.filter_rows(px, types))
    want = np.stack([_png_ref.unfilter(f, W, H, 1) for f in filtered])
    assert np.array_equal(want, np.stack(pixels))
    got = run_unfilter(filtered, W, H, 1)
    bad = np.argwhere((got != want).reshape(len(filtered), -1).any(axis=1)).ravel()
    assert bad.size == 0, f"images {bad.tolist()} differ"


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2, 4, 8])
def test_expand_every_depth_and_scale(depth):
    """Packed rows with a tail (W no multiple of the samples per byte), junk in the padding bits, grey scale and index scale."""
    P = pkg("png_io")
    rng = np.random.RandomState(depth)
    for W, H in ((1, 1), (13, 3), (67, 70), (301, 5)):
        rb = (W * depth + 7) // 8
        packed = rng.randint(0, 256, (2, H, rb)).astype(np.uint8)
        bits = np.unpackbits(packed, axis=2)[:, :, :W * depth].reshape(2, H, W, depth)
        want = (bits * (1 << np.arange(depth - 1, -1, -1))).sum(axis=3)
        for scale in (1, P.GREY_SCALE[depth]):
            got = P.expand(torch.tensor(packed, device=DEV), W, depth, scale)
            torch.cuda.synchronize()
            assert got.shape == (2, H, W, 1) and np.array_equal(got.cpu().numpy()[..., 0], want * scale), (W, H, scale)
    assert P.GREY_SCALE == {1: 255, 2: 85, 4: 17, 8: 1}
    with pytest.raises(RuntimeError):
        P.expand(torch.zeros((1, 1, 1), dtype=torch.uint8), 1, depth, 1)


@pytest.mark.gpu
def test_resize_nearest_equals_pillow(gold):
    R = pkg("resample")
    keys = sorted(k[:-3] for k in gold.files if k.startswith("resize/") and k.endswith("/in"))
    assert len(keys) == 24
    for key in keys:
        src, want = as_bytes(gold[key + "/in"]), as_bytes(gold[key + "/out"])
        batch = np.stack([src, src[::-1, ::-1]])  # (a second, different image in the batch)
        got = R.resize_nearest(torch.tensor(batch, device=DEV), (want.shape[1], want.shape[0]))
        torch.cuda.synchronize()
        assert got.shape == (2,) + want.shape and np.array_equal(got[0].cpu().numpy(), want), key
        xs, ys = R.nearest_indices(src.shape[1], want.shape[1]), R.nearest_indices(src.shape[0], want.shape[0])
        assert np.array_equal(got[1].cpu().numpy(), batch[1][ys][:, xs]), key
    # three and four channels through the same table; an unchanged size is the tensor itself
    rng = np.random.RandomState(3)
    for C in (3, 4):
        px = rng.randint(0, 256, (2, 11, 13, C)).astype(np.uint8)
        t = torch.tensor(px, device=DEV)
        got = R.resize_nearest(t, (20, 17)).cpu().numpy()
        assert np.array_equal(got, px[:, R.nearest_indices(11, 17)][:, :, R.nearest_indices(13, 20)])
        assert R.resize_nearest(t, (13, 11)) is t
    with pytest.raises(RuntimeError):
        R.resize_nearest(torch.zeros((1, 2, 2, 1), dtype=torch.uint8), (1, 1))


def run_masked(frames, masks, white):
    D = pkg("dataset")
    f, m = torch.tensor(np.ascontiguousarray(frames), device=DEV), torch.tensor(np.ascontiguousarray(masks), device=DEV)
    bg = [1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0]
    image, alpha = D.image_ingest_masked(f, m, bg)
    packed = D.image_ingest_masked(f, m, bg, out="bytes")
    torch.cuda.synchronize()
    B, H, W, _ = frames.shape
    assert image.shape == (B, 3, H, W) and alpha.shape == (B, H, W, 1) and image.dtype == alpha.dtype == torch.float32
    assert packed.shape == (B, H, W, 4) and packed.dtype == torch.uint8
    return image.cpu().numpy(), alpha.cpu().numpy(), packed.cpu().numpy()


def check_masked(frames, masks, white):
    image, alpha, packed = run_masked(frames, masks, white)
    for b in range(frames.shape[0]):
        want_i, want_a = CR.ingest_masked(frames[b], masks[b], white)
        assert np.array_equal(image[b], want_i) and np.array_equal(alpha[b], want_a), b
        assert np.array_equal(packed[b], CR.ingest_masked_bytes(frames[b], masks[b], white)), b


@pytest.mark.gpu
@pytest.mark.parametrize("white", [False, True])
def test_masked_ingest_exhaustive_byte_table(white):
    """All 256 bytes in every channel, under a clear mask (row 0) and under every non-zero mask value (row 1)."""
    rng = np.random.RandomState(11)
    c = np.arange(256, dtype=np.uint8)
    frame = np.stack([np.stack([c, rng.permutation(c), rng.permutation(c)], axis=1)] * 2)[None]  # (1, 2, 256, 3)
    mask = np.zeros((1, 2, 256, 1), np.uint8)
    mask[0, 1, :, 0] = np.maximum(c, 1)
    check_masked(frame, mask, white)
    image, alpha, _ = run_masked(frame, mask, white)
    assert np.array_equal(image[0, 0, 1], c.astype(np.float32) / np.float32(255.0)) and float(alpha[0, 1].min()) == 1.0
    assert np.all(image[0, :, 0] == (1.0 if white else 0.0)) and float(alpha[0, 0].max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(5, 7), (33, 19)])
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("Cm", [1, 3])
def test_masked_ingest_odd_sizes(W, H, C, Cm):
    """Pixel counts that are no multiple of four (the vector path's tail); only channel 0 of the mask counts; a frame's alpha is dropped."""
    rng = np.random.RandomState(W + H + C + Cm)
    frames = rng.randint(0, 256, (2, H, W, C)).astype(np.uint8)
    masks = rng.choice(np.array([0, 0, 1, 128, 255], np.uint8), (2, H, W, Cm))
    if Cm == 3:
        masks[..., 1:] = 255 - masks[..., :1]  # (set where channel 0 is clear: they must not count)
    for white in (False, True):
        check_masked(frames, masks, white)


@pytest.mark.gpu
def test_masked_ingest_refuses_host_tensors_and_mismatches():
    D = pkg("dataset")
    with pytest.raises(RuntimeError):
        D.image_ingest_masked(torch.zeros((1, 2, 2, 3), dtype=torch.uint8), torch.zeros((1, 2, 2, 1), dtype=torch.uint8), [0, 0, 0])
    f = torch.zeros((1, 2, 2, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="differ"):
        D.image_ingest_masked(f, torch.zeros((1, 2, 3, 1), dtype=torch.uint8, device=DEV), [0, 0, 0])
    with pytest.raises(ValueError, match="out must be"):
        D.image_ingest_masked(f, torch.zeros((1, 2, 2, 1), dtype=torch.uint8, device=DEV), [0, 0, 0], out="floats")


def model_params(kind, root, out, **kw):
    lp = pkg("train").ModelParams()
    lp.source_path, lp.model_path, lp.eval, lp.data_type = root, str(out), True, kind
    for k, v in kw.items():
        setattr(lp, k, v)
    return lp


def load(scenes, kind, out, **kw):
    root, items = scenes[kind]
    sc = pkg("dataset").Scene(model_params(kind, root, out, **kw), None, device=DEV)
    torch.cuda.synchronize()
    train, test = sc.getTrainCameras(), sc.getTestCameras()
    assert len(train) == F.N_TRAIN and len(test) == F.N_VAL
    by_fid = {round(it["cam"].fid, 6): it for it in items}
    assert sorted(round(float(c.fid), 6) for c in train) == sorted(round(it["cam"].fid, 6) for it in items if it["split"] == "train")
    return sc, [(c, by_fid[round(float(c.fid), 6)]) for c in train + test]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("white", [False, True])
def test_scene_images_and_masks_bit_exact(scenes, gold, tmp_path, kind, white):
    sc, cams = load(scenes, kind, tmp_path / "out", white_background=white)
    for cam, item in cams:
        want_i, want_m = CR.ingest_masked(item["frame"], gold[f"scene/{item['flavour']}/pixels"], white)
        assert (cam.image_width, cam.image_height) == (F.W, F.H)
        assert np.array_equal(cam.original_image.cpu().numpy(), want_i), item["flavour"]
        assert np.array_equal(cam.gt_alpha_mask.cpu().numpy(), want_m), item["flavour"]
        assert np.array_equal(want_m[..., 0] > 0, gold[f"scene/{item['flavour']}/gt0"])
        if kind == "NeuralActor":  # (its reader's own arithmetic, a round trip through v / 255.0: the shared kernel reproduces it)
            actor_i, actor_m = CR.planes(*CR.composite_bytes_neural_actor(item["frame"], gold[f"scene/{item['flavour']}/pixels"], white))
            assert np.array_equal(cam.original_image.cpu().numpy(), actor_i) and np.array_equal(cam.gt_alpha_mask.cpu().numpy(), actor_m)
        for name in ("world_view_transform", "full_proj_transform", "camera_center"):
            assert np.abs(getattr(cam, name).cpu().numpy() - getattr(item["cam"], name)).max() <= 1e-6, name
    assert os.path.exists(tmp_path / "out" / "input.ply") and os.path.exists(tmp_path / "out" / "cameras.json")
    assert sc.cameras_extent == pytest.approx(CR.extent([it["cam"].camera_center for _, it in cams if it["split"] == "train"]), rel=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("white", [False, True])
def test_nerfies_downsample(scenes, gold, tmp_path, white):
    """downsample = 2: the frame through Lanczos (an RGBA frame premultiplied, as Pillow does), the mask as Pillow resizes its mode --
    NEAREST for P and 1, Lanczos for L, RGB and RGBA -- then > 0; the intrinsics follow the image."""
    sc, cams = load(scenes, "Nerfies", tmp_path / "out", white_background=white, downsample=2.0)
    _, full = load(scenes, "Nerfies", tmp_path / "full", white_background=white)
    for (cam, item), (cam1, _) in zip(cams, full):
        half = gold[f"scene/{item['flavour']}/half"]
        want_i, want_m = CR.ingest_masked(RR.resize_rgba(item["frame"], (24, 20)), half, white)
        assert (cam.image_width, cam.image_height) == (24, 20)
        assert np.array_equal(cam.original_image.cpu().numpy(), want_i), item["flavour"]
        assert np.array_equal(cam.gt_alpha_mask.cpu().numpy(), want_m), item["flavour"]
        assert np.array_equal(want_m[..., 0] > 0, gold[f"scene/{item['flavour']}/half_gt0"])
        assert float(cam.fid) == float(cam1.fid)
        assert np.abs((cam.full_proj_transform - cam1.full_proj_transform).cpu().numpy()).max() <= 1e-6, "the frustum changed"
    for ci in sc.scene_info.train_cameras:
        assert (ci.width, ci.height) == (24, 20) and ci.K[0, 0] == pytest.approx(F.K_SQUARE[0, 0] / 2, abs=1e-12)


@pytest.mark.gpu
def test_iphone_and_neural_actor_ignore_downsample(scenes, tmp_path):
    for kind in ("iPhone", "NeuralActor"):
        _, cams = load(scenes, kind, tmp_path / kind, downsample=2.0)
        assert all((cam.image_width, cam.image_height) == (F.W, F.H) for cam, _ in cams)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_resolution_resizes_image_and_mask_together(scenes, gold, tmp_path, kind):
    """resolution = 2: the composited bytes and 255 x mask as a fourth, non-premultiplied channel through the bicubic filter, as
    Blender scenes resize their alpha (tests/test_scene_resize.py)."""
    _, cams = load(scenes, kind, tmp_path / "out", white_background=True, resolution=2)
    _, full = load(scenes, kind, tmp_path / "full", white_background=True)
    for (cam, item), (cam1, _) in zip(cams, full):
        packed = CR.ingest_masked_bytes(item["frame"], gold[f"scene/{item['flavour']}/pixels"], True)
        rgb, alpha = RR.resize(np.ascontiguousarray(packed[..., :3]), (24, 20), "bicubic"), RR.resize(np.ascontiguousarray(packed[..., 3]), (24, 20), "bicubic")
        assert cam.original_image.shape == (3, 20, 24) and cam.gt_alpha_mask.shape == (20, 24, 1)
        assert np.array_equal(cam.original_image.cpu().numpy(), np.ascontiguousarray((rgb.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)))
        assert np.array_equal(cam.gt_alpha_mask.cpu().numpy(), (alpha[..., None] / 255.0).astype(np.float32))
        assert np.abs((cam.full_proj_transform - cam1.full_proj_transform).cpu().numpy()).max() <= 1e-6, "the frustum changed"


@pytest.mark.gpu
def test_mask_of_another_size_or_missing_is_named(scenes, gold, tmp_path):
    import shutil
    root = str(tmp_path / "iphone")
    shutil.copytree(scenes["iPhone"][0], root)
    mask = os.path.join(root, "mask-tracking", "1x", "Annotations", "frame_002.png")
    frame = os.path.join(root, "rgb", "1x", "frame_002.png")
    with open(mask, "wb") as fh:
        fh.write(gold["file/P3/67x70/png"].tobytes())
    with pytest.raises(ValueError) as e:
        pkg("dataset").Scene(model_params("iPhone", root, tmp_path / "out"), None, device=DEV)
    assert mask in str(e.value) and frame in str(e.value) and "67 x 70" in str(e.value) and "48 x 40" in str(e.value)
    os.remove(mask)
    with pytest.raises(ValueError, match="missing") as e:
        pkg("dataset").Scene(model_params("iPhone", root, tmp_path / "out"), None, device=DEV)
    assert mask in str(e.value) and frame in str(e.value)


@pytest.mark.gpu
def test_mask_size_is_compared_before_downsample(scenes, tmp_path):
    """A 49 x 41 mask beside a 48 x 40 frame: both are 24 x 20 after downsample = 2, and the files still differ."""
    import shutil
    root = str(tmp_path / "nerfies")
    shutil.copytree(scenes["Nerfies"][0], root)
    mask = os.path.join(root, "mask-tracking", "2x", "Annotations", "frame_003.png")
    px = np.zeros((41, 49, 1), np.uint8)
    px[10:30, 10:30] = 200
    with open(mask, "wb") as fh:
        fh.write(_png_ref.wrap_png(_png_ref.filter_rows(px, [0] * 41), 49, 41, 1, colour=0))
    for d in (2.0, 1.0):
        with pytest.raises(ValueError) as e:
            pkg("dataset").Scene(model_params("Nerfies", root, tmp_path / "out", downsample=d), None, device=DEV)
        assert mask in str(e.value) and os.path.join(root, "rgb", "2x", "frame_003.png") in str(e.value)
        assert "49 x 41" in str(e.value) and "48 x 40" in str(e.value)


@pytest.mark.gpu
def test_training_on_the_iphone_scene_crosses_dpsr_iter(scenes, tmp_path):
    """About 60 iterations from prepared Gaussians, entering the mesh phase at iteration 30 on a 32^3 grid with the cube placed by
    dpsr_center / gaussian_ratio, the normal networks joining 10 iterations later."""
    T, S, syn = pkg("train"), pkg("scene"), pkg("synthetic")
    root, _ = scenes["iPhone"]
    dev = torch.device(DEV)
    g_np = syn.make_gaussians(3000, seed=0, kind="aniso", extent=0.7)
    g = S.GaussianModel(sh_degree=3, device=dev)
    g.load_raw(g_np["xyz"], g_np["features_dc"], g_np["features_rest"], g_np["scaling"] + 0.5, g_np["rotation"], g_np["opacity"] + 2.0)
    center = [0.1, -0.05, 0.02]
    lines = []
    cfg = T.merge_config(dict(source_path=root, model_path=str(tmp_path / "m"), data_type="iPhone", eval=True, white_background=True,
                              gaussian_center=center, gaussian_ratio=2.0, iterations=60, warm_up=5, dpsr_iter=30, normal_deform_delay=10,
                              grid_res=32, dpsr_sig=2.0, densify_from_iter=10 ** 9, log_every=30), log=lines.append)
    assert cfg["is_blender"] is False and cfg["dpsr_center"] == center and any("dpsr_center" in ln for ln in lines)
    res = T.training(cfg, gaussians=g, log=lambda *a: None)
    torch.cuda.synchronize()
    assert sorted(res["log"]) == list(range(1, 61))
    mesh_terms = {"mask_loss", "mesh_img_loss", "laplacian_loss"}
    for it, row in res["log"].items():
        assert all(np.isfinite(v) for v in row.values()), (it, row)
        assert (mesh_terms <= set(row)) == (it >= 30), (it, sorted(row))
    assert res["mesh"].real and res["mesh"].last_normal_init is not None and res["mesh"].dpsr.res == (32, 32, 32)
    assert g.gaussian_center.tolist() == [float(np.float32(v)) for v in center]
    assert g.gaussian_scale.tolist() == [1.0]  # gaussian_ratio / 2
    assert set(res["networks"]) == {"deform", "deform_back", "deform_normal", "deform_back_normal", "appearance"}
    for name, m in res["networks"].items():
        moved = [float(s["exp_avg"].abs().sum()) for s in m.optimizer.state.values() if "exp_avg" in s]
        assert moved and max(moved) > 0.0, f"{name} never stepped"
    test = res["test"]
    assert test is not None and test["views"].shape[0] == 2 and test["mesh"] is not None
    for which in ("gaussian", "mesh"):  # (ms_ssim is NaN by definition at this size: min(H, W) <= 160)
        assert all(np.isfinite(test[which][k]) for k in ("mse", "psnr", "ssim")), (which, test[which])
