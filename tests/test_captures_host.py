"""The host side of reading real captures: parse_png_any on Pillow-written mask files, the three readers of captures.py on scenes the
test writes (tests/_capture_fixture.py) against the poses they were written from and against tests/_capture_ref.py, the NEAREST index
table against Pillow's output, and the configuration keys that real captures bring (dpsr_center, nerfies_ratio)."""
import json
import os
import struct
import zlib

import numpy as np
import pytest

import _capture_fixture as F
import _capture_ref as CR
import _png_ref
from conftest import ROOT, pkg

KINDS = ("Nerfies", "iPhone", "NeuralActor")
# flavour -> (colour type, bit depth, channels)
FLAVOURS = {"1": (0, 1, 1), "L": (0, 8, 1), "P256": (3, 8, 1), "P3": (3, 2, 1), "P16": (3, 4, 1), "Pbits1": (3, 1, 1), "RGB": (2, 8, 3),
            "RGBA": (6, 8, 4)}


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


def file_keys(gold):
    return sorted(k[:-4] for k in gold.files if k.endswith("/png"))


def test_parse_png_any_on_every_golden_file(gold):
    P = pkg("png_io")
    keys = file_keys(gold)
    assert len(keys) == 8 * 5 + 8
    for key in keys:
        flavour = key.split("/")[1]
        colour, depth, ch = FLAVOURS[flavour]
        px = gold[key + "/pixels"]
        W, H, c, d, row_bytes, bpp, filtered = P.parse_png_any(gold[key + "/png"].tobytes())
        assert (W, H) == (px.shape[1], px.shape[0]) and (c, d) == (colour, depth), key
        assert row_bytes == -(-W * ch * depth // 8) and bpp == max(1, ch * depth // 8), key
        assert len(filtered) == H * (1 + row_bytes)
        assert P.mask_kind(c, d) == {"1": "index", "L": "grey", "RGB": "rgb", "RGBA": "rgba"}.get(flavour, "index")


def _rewrap(data, **head):
    """The file with IHDR fields replaced (and its CRC made right again)."""
    W, H, depth, colour, comp, filt, inter = struct.unpack(">IIBBBBB", data[16:29])
    f = dict(depth=depth, colour=colour, interlace=inter)
    f.update(head)
    body = struct.pack(">IIBBBBB", W, H, f["depth"], f["colour"], comp, filt, f["interlace"])
    return data[:12] + b"IHDR" + body + struct.pack(">I", zlib.crc32(b"IHDR" + body) & 0xFFFFFFFF) + data[33:]


def test_parse_png_any_refuses_by_name(gold):
    P = pkg("png_io")
    grey = gold["file/L/9x7/png"].tobytes()
    pal = gold["file/P3/9x7/png"].tobytes()
    for data, match in ((_rewrap(grey, depth=16), "bit depth 16"), (_rewrap(grey, colour=4), "colour type 4"),
                        (_rewrap(grey, interlace=1), "interlaced"), (grey[:-20], "truncated"), (grey[:40], "truncated"),
                        (grey[:50] + bytes([grey[50] ^ 1]) + grey[51:], "bad CRC"), (_rewrap(gold["file/RGB/9x7/png"].tobytes(), depth=4), "bit depth 4"),
                        (b"nope" + grey[4:], "not a PNG")):
        with pytest.raises(ValueError, match=match):
            P.parse_png_any(data)
    # a palette file needs its PLTE chunk
    at = pal.index(b"PLTE") - 4
    n = struct.unpack(">I", pal[at:at + 4])[0]
    with pytest.raises(ValueError, match="PLTE"):
        P.parse_png_any(pal[:at] + pal[at + 12 + n:])
    # a filter byte above 4 (one byte per pixel, written by the test-side encoder)
    px = np.arange(12, dtype=np.uint8).reshape(3, 4, 1)
    rows = bytearray(_png_ref.filter_rows(px, [0, 1, 2]))
    ok = _png_ref.wrap_png(bytes(rows), 4, 3, 1, colour=0)
    assert P.parse_png_any(ok)[:6] == (4, 3, 0, 8, 4, 1)
    rows[5] = 7
    with pytest.raises(ValueError, match="bad filter type 7 on row 1"):
        P.parse_png_any(_png_ref.wrap_png(bytes(rows), 4, 3, 1, colour=0))


def test_parse_png_still_refuses_grey_palette_and_grey_alpha(gold):
    P = pkg("png_io")
    for key, match in (("file/L/9x7", "colour type 0"), ("file/P256/9x7", "colour type 3"), ("file/1/9x7", "bit depth 1")):
        with pytest.raises(ValueError, match=match):
            P.parse_png(gold[key + "/png"].tobytes())
    with pytest.raises(ValueError, match="colour type 4"):
        P.parse_png(_rewrap(gold["file/L/9x7/png"].tobytes(), colour=4))


def test_nearest_index_table_equals_pillow(gold):
    R = pkg("resample")
    keys = sorted(k[:-3] for k in gold.files if k.startswith("resize/") and k.endswith("/in"))
    assert len(keys) == 24
    for key in keys:
        src, want = gold[key + "/in"], gold[key + "/out"]
        xs, ys = R.nearest_indices(src.shape[1], want.shape[1]), R.nearest_indices(src.shape[0], want.shape[0])
        assert xs.dtype == np.int32 and xs.max() < src.shape[1] and ys.max() < src.shape[0]
        assert np.array_equal(src[ys][:, xs], want), key
        assert np.array_equal(want > 0, gold[key + "/gt0"])
    # Pillow adds in / out per output pixel; the closed form int((i + 0.5) in / out) names another pixel where the product is an integer
    closed = lambda i, o: np.array([min(int((j + 0.5) * i / o), i - 1) for j in range(o)])
    differ = [(i, o) for i, o in ((8, 6), (16, 6), (24, 9), (270, 67), (540, 67), (536, 178), (536, 357))
              if not np.array_equal(R.nearest_indices(i, o), closed(i, o))]
    assert len(differ) == 7, differ
    src = gold["resize/270x540_67x135/P/in"]
    assert not np.array_equal(src[closed(540, 135)][:, closed(270, 67)], gold["resize/270x540_67x135/P/out"])


def test_neural_actor_round_trip_is_the_shared_composite():
    """Pins only the premise, in the test-side restatements: (v / 255.0) * 255.0 truncates back to v for every byte, so
    readNeuralActorCameras' composite is the other two readers'.  That the product sends NeuralActor scenes through the shared kernel
    is tests/test_captures_gpu.py's NeuralActor Scene test, which compares against composite_bytes_neural_actor."""
    frame = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    mask = (np.arange(256).reshape(16, 16) % 3 > 0)
    for white in (False, True):
        a, _ = CR.composite_bytes_neural_actor(frame, mask, white)
        b, _ = CR.composite_bytes(frame, mask, white)
        assert np.array_equal(a, b)
    full, _ = CR.composite_bytes_neural_actor(frame, np.ones((16, 16), bool), False)
    assert np.array_equal(full, frame)


def read(kind, root, **kw):
    return pkg("captures").READERS[kind](root, False, kw.pop("eval", True), **kw)


@pytest.mark.parametrize("kind", KINDS)
def test_reader_cameras_equal_the_poses_written(scenes, kind, tmp_path):
    D = pkg("dataset")
    root, items = scenes[kind]
    before = F.listing(root)
    info = read(kind, root, model_path=str(tmp_path))
    assert F.listing(root) == before, "the reader wrote into the dataset directory"
    assert len(info.train_cameras) == F.N_TRAIN and len(info.test_cameras) == F.N_VAL
    for ci, item in zip(info.train_cameras + info.test_cameras, items):
        cam, want = D.make_camera(ci), item["cam"]
        assert (ci.width, ci.height) == (F.W, F.H) and ci.K.shape == (3, 3) and ci.K.dtype == np.float64
        for name in ("world_view_transform", "full_proj_transform", "camera_center"):
            assert np.abs(getattr(cam, name) - getattr(want, name)).max() <= 1e-6, (kind, name)
        assert cam.fid == pytest.approx(want.fid, abs=1e-12) and cam.FoVx == pytest.approx(want.FoVx, abs=1e-12)
        assert cam.FoVy == pytest.approx(want.FoVy, abs=1e-12)
        assert os.path.exists(ci.mask_path) and os.path.exists(ci.image_path) and ci.mask_path != ci.image_path
    assert [c.uid for c in info.train_cameras + info.test_cameras] == (
        list(range(7)) if kind != "NeuralActor" else list(range(5)) + list(range(2)))
    # fids: time ids over their maximum, train ids first; NeuralActor's `time` itself
    fids = [c.fid for c in info.train_cameras + info.test_cameras]
    assert fids == ([t / 10 for t in F.TIME_IDS] if kind != "NeuralActor" else [k / 10.0 for k in range(7)])
    # getNerfppNorm over the training cameras
    centers = [item["cam"].camera_center for item in items]
    assert info.cameras_extent == pytest.approx(CR.extent(centers[:F.N_TRAIN]), rel=1e-6)
    # the point cloud: points.npy recentred (Nerfies), as it is (iPhone); seeded points in [-1, 1]^3 (NeuralActor); input.ply
    pts = info.point_cloud.points
    if kind == "NeuralActor":
        assert pts.shape == (100_000, 3) and pts.dtype == np.float32 and -1.0 <= pts.min() < -0.999 and 0.999 < pts.max() <= 1.0
        assert np.array_equal(pts, read(kind, root).point_cloud.points), "the default cloud is not seeded"
    else:
        assert pts.dtype == np.float32 and np.abs(pts - F.points()).max() <= 1e-6
    assert info.ply_path == os.path.join(str(tmp_path), "input.ply") and os.path.exists(info.ply_path)
    stored = D.fetch_ply(info.ply_path)
    assert np.array_equal(stored.points, pts) and np.array_equal(stored.colors, info.point_cloud.colors)
    assert 0.49 < info.point_cloud.colors.min() and info.point_cloud.colors.max() < 0.51  # SH2RGB(rand / 255)
    assert read(kind, root).ply_path is None, "no model_path: nothing is written"


@pytest.mark.parametrize("kind", KINDS)
def test_reader_pose_maths_is_the_reference_text(scenes, kind):
    root, _ = scenes[kind]
    info = read(kind, root)
    cams = info.train_cameras + info.test_cameras
    if kind == "NeuralActor":
        frames = []
        for split in ("train", "test"):
            with open(os.path.join(root, f"transforms_{split}.json")) as fh:
                frames += json.load(fh)["frames"]
        want = [CR.neural_actor_pose(f) for f in frames]
    else:
        with open(os.path.join(root, "dataset.json")) as fh:
            ids = json.load(fh)
        want = []
        for name in ids["train_ids"] + ids["val_ids"]:
            with open(os.path.join(root, "camera", name + ".json")) as fh:
                cj = json.load(fh)
            want.append(CR.nerfies_pose(cj, F.RATIO, F.CENTER, F.SCALE) if kind == "Nerfies" else CR.nerfies_pose(cj, 1.0))
    for ci, (R, T, K) in zip(cams, want):
        assert np.abs(ci.R - R).max() <= 1e-12 and np.abs(ci.T - T).max() <= 1e-12 and np.abs(ci.K - K).max() <= 1e-12
        assert ci.FoVx == pytest.approx(CR.focal2fov(K[0, 0], F.W), abs=1e-12) and ci.FoVy == pytest.approx(CR.focal2fov(K[1, 1], F.H), abs=1e-12)
        wvt, full, center = CR.camera_matrices(R, T, K, F.W, F.H)
        cam = pkg("dataset").make_camera(ci)
        assert np.abs(cam.world_view_transform - wvt).max() <= 1e-6 and np.abs(cam.full_proj_transform - full).max() <= 1e-6
        assert np.abs(cam.camera_center - center).max() <= 1e-6


@pytest.mark.parametrize("kind", KINDS)
def test_eval_split(scenes, kind):
    root, _ = scenes[kind]
    folded = read(kind, root, eval=False)
    split = read(kind, root, eval=True)
    assert len(folded.train_cameras) == 7 and folded.test_cameras == []
    assert [c.image_name for c in folded.train_cameras] == [c.image_name for c in split.train_cameras + split.test_cameras]
    centers = [item["cam"].camera_center for item in scenes[kind][1]]
    assert folded.cameras_extent == pytest.approx(CR.extent(centers), rel=1e-6)
    assert split.cameras_extent == pytest.approx(CR.extent(centers[:F.N_TRAIN]), rel=1e-6)


def test_nerfies_downsample_scales_the_intrinsics(scenes):
    root, _ = scenes["Nerfies"]
    full, half = read("Nerfies", root), read("Nerfies", root, downsample=2.0)
    odd = read("Nerfies", root, downsample=1.7)  # (int(48 / 1.7), int(40 / 1.7)) = (28, 23): the two axes scale differently
    for a, b, c in zip(full.train_cameras, half.train_cameras, odd.train_cameras):
        assert (b.width, b.height) == (24, 20) and (c.width, c.height) == (28, 23)
        assert np.allclose(b.K, np.diag([0.5, 0.5, 1.0]) @ a.K, rtol=0, atol=1e-12)
        assert np.allclose(c.K, np.diag([28 / 48, 23 / 40, 1.0]) @ a.K, rtol=0, atol=1e-12)
        assert b.FoVx == pytest.approx(a.FoVx, abs=1e-12) and b.FoVy == pytest.approx(a.FoVy, abs=1e-12), "the frustum must not change"
        assert c.FoVx == pytest.approx(a.FoVx, abs=1e-12) and c.FoVy == pytest.approx(a.FoVy, abs=1e-12)
        assert np.array_equal(a.R, b.R) and np.array_equal(a.T, b.T)
        # the same normalised projection from both sizes
        D = pkg("dataset")
        assert np.abs(D.make_camera(a).full_proj_transform - D.make_camera(b).full_proj_transform).max() <= 1e-6
    other = read("Nerfies", root, nerfies_ratio=0.5)
    assert np.array_equal(other.train_cameras[0].K, full.train_cameras[0].K)


def test_nerfies_falls_back_to_warp_id_and_iphone_ignores_time_id(tmp_path):
    syn = pkg("synthetic")
    F.write_nerfies_like(str(tmp_path / "n"), syn, "Nerfies", time_key="warp_id")
    info = read("Nerfies", str(tmp_path / "n"))
    assert [c.fid for c in info.train_cameras] == [t / 10 for t in F.TIME_IDS[:5]]
    F.write_nerfies_like(str(tmp_path / "i"), syn, "iPhone", time_key="time_id")
    with pytest.raises(ValueError, match="warp_id"):
        read("iPhone", str(tmp_path / "i"))


def test_missing_mask_and_wrong_mask_are_named(scenes, tmp_path, gold):
    import shutil
    root = str(tmp_path / "actor")
    shutil.copytree(scenes["NeuralActor"][0], root)
    mask = os.path.join(root, "training_mask", "Annotations", "000002.png")
    with open(mask, "wb") as fh:
        fh.write(gold["scene/L/png"].tobytes())
    with pytest.raises(ValueError, match="three or four channels") as e:
        read("NeuralActor", root)
    assert "000002.png" in str(e.value)
    os.remove(mask)
    with pytest.raises(ValueError, match="missing") as e:
        read("NeuralActor", root)
    assert mask in str(e.value) and os.path.join(root, "training", "000002.png") in str(e.value)


def test_dataset_stubs_stay_and_scene_types_are_known():
    D, C = pkg("dataset"), pkg("captures")
    assert set(C.READERS) == {"Nerfies", "iPhone", "NeuralActor"} and set(D.READERS) == set(C.READERS) | {"Blender"}
    info = D.CameraInfo(0, np.eye(3), np.zeros(3), 0.5, 0.5, "a.png", "a", 4, 4, 0.0)
    assert info.K is None and info.mask_path is None


def test_config_keys_of_real_captures():
    T = pkg("train")
    tiger = {"data_type": "iPhone", "gaussian_center": [-0.25, -0.25, -0.25], "gaussian_ratio": 2.0, "white_background": True,
             "grid_res": 256, "nerfies_ratio": 0.5}  # the values of the reference's configs/iphone/tiger.yaml that matter here
    path = os.path.join(ROOT, "oracle", "_ref", "configs", "iphone", "tiger.yaml")
    if os.path.exists(path):
        tiger = T.load_yaml(path)
    lines = []
    cfg = T.merge_config(tiger, log=lines.append)
    assert cfg["dpsr_center"] == [-0.25, -0.25, -0.25] and all(isinstance(v, float) for v in cfg["dpsr_center"])
    assert "gaussian_center" not in cfg and cfg["data_type"] == "iPhone"
    assert "[config] gaussian_center -> dpsr_center (the DPSR cube's centre for iPhone / NeuralActor captures)" in lines
    assert "nerfies_ratio" in cfg and T.ModelParams.nerfies_ratio == 0.5 and "nerfies_ratio" not in T.IGNORED_KEYS
    assert T.default_config()["dpsr_center"] is None
    lp, op, _ = T.split_config(cfg)
    kw = T.mesh_phase_options(lp, op, seed=1, center=cfg["dpsr_center"])
    assert kw["real"] is True and kw["gaussian_center"] == [-0.25, -0.25, -0.25]
    ms = pkg("trainer").MeshPhase(None, None, None, dpsr=object(), device="cpu", n_verts=4, **kw)
    assert ms.real and ms.gaussian_center == (-0.25, -0.25, -0.25)
    assert T.mesh_phase_options(lp, op)["gaussian_center"] is None
    assert pkg("trainer").MeshPhase(None, None, None, dpsr=object(), device="cpu", n_verts=4, **T.mesh_phase_options(lp, op)).gaussian_center == (0.0, 0.0, 0.0)
    # the command line, and what is not three numbers
    assert T.config_from_argv(["--dpsr_center", "[0.5, 0, -1]"], log=lambda *a: None)["dpsr_center"] == [0.5, 0.0, -1.0]
    for bad in ([1.0, 2.0], "centre", [1.0, 2.0, "z"], [1.0, 2.0, float("nan")], 3.0, [True, 0, 0]):
        with pytest.raises(ValueError, match="dpsr_center"):
            T.merge_config({"dpsr_center": bad}, log=lambda *a: None)
    with pytest.raises(ValueError, match="dpsr_center"):
        T.config_from_argv(["--dpsr_center", "1.5"])
