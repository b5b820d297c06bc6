"""Scene (dataset.py) with `downsample` and `resolution` on a non-square scene the test writes (tests/_scene_fixture.py): images and
masks bit for bit against the restatements (tests/_resample_ref.py, tests/_ingest_ref.py) in the reference's stage order, the camera
fields and cameras.json; and a short training run at a reduced resolution."""
import json
import math

import numpy as np
import pytest
import torch

import _ingest_ref
import _resample_ref as R
import _scene_fixture as F
from conftest import pkg

W, H = 40, 24


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("scene_resize")
    items = F.write_scene(str(root), pkg("synthetic"), n_train=4, n_test=2, W=W, H=H, points=F.ball_points(500))
    return str(root), items


def model_params(root, out, **kw):
    lp = pkg("train").ModelParams()
    lp.source_path, lp.model_path, lp.eval, lp.is_blender = root, str(out), True, True
    for k, v in kw.items():
        setattr(lp, k, v)
    return lp


def composite_then_bicubic(px, white, size):
    """`resolution`: the composited bytes (tests/_ingest_ref.py's, before its division) resized as an RGB image, the file's alpha as
    a single plane with the same filter; then the divisions by 255."""
    image, _ = _ingest_ref.ingest(px, white)
    rgb = np.rint(image.transpose(1, 2, 0).astype(np.float64) * 255.0).astype(np.uint8)
    assert np.array_equal(rgb.astype(np.float32) / np.float32(255.0), image.transpose(1, 2, 0))
    alpha = px[..., 3] if px.shape[2] == 4 else np.full(px.shape[:2], 255, np.uint8)
    rgb, alpha = R.resize(rgb, size, "bicubic"), R.resize(alpha, size, "bicubic")
    return (np.ascontiguousarray((rgb.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)),
            (alpha[..., None] / 255.0).astype(np.float32))


def fovy(w, h):
    return 2 * math.atan(math.tan(F.FOVX / 2) * h / w)


def load(scene_dir, out, white, **kw):
    D = pkg("dataset")
    root, items = scene_dir
    sc = D.Scene(model_params(root, out, white_background=white, **kw), None, device="cuda:0")
    by_fid = {round(c.fid, 6): px for c, px in items["train"] + items["test"]}
    cams = sc.getTrainCameras() + sc.getTestCameras()
    assert len(cams) == 6
    with open(out / "cameras.json") as fh:
        cams_json = json.load(fh)
    return sc, [(cam, by_fid[round(float(cam.fid), 6)]) for cam in cams], cams_json


def check_camera(cam, size, want_i, want_m, fov_y):
    assert (cam.image_width, cam.image_height) == size
    assert cam.original_image.shape == (3, size[1], size[0]) and cam.gt_alpha_mask.shape == (size[1], size[0], 1)
    assert np.array_equal(cam.original_image.cpu().numpy(), want_i)
    assert np.array_equal(cam.gt_alpha_mask.cpu().numpy(), want_m)
    assert cam.FoVx == F.FOVX and cam.FoVy == pytest.approx(fov_y, abs=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("white", [False, True])
def test_downsample(scene_dir, tmp_path, white):
    sc, cams, cams_json = load(scene_dir, tmp_path / "out", white, downsample=2.0)
    for cam, px in cams:
        want_i, want_m = _ingest_ref.ingest(R.resize_rgba(px, (20, 12)), white)
        check_camera(cam, (20, 12), want_i, want_m, fovy(20, 12))
    for ci in sc.scene_info.train_cameras + sc.scene_info.test_cameras:
        assert (ci.width, ci.height) == (20, 12) and ci.FoVx == F.FOVX and ci.FoVy == pytest.approx(fovy(20, 12), abs=1e-12)
    for e in cams_json:
        assert (e["width"], e["height"]) == (20, 12)
        assert e["fx"] == pytest.approx(20 / (2 * math.tan(F.FOVX / 2))) and e["fy"] == pytest.approx(12 / (2 * math.tan(fovy(20, 12) / 2)))


@pytest.mark.gpu
def test_downsample_to_a_non_integer_ratio(scene_dir, tmp_path):
    """int(40 / 1.5), int(24 / 1.5) = (26, 16): the aspect ratio, and with it FoVy, changes."""
    sc, cams, cams_json = load(scene_dir, tmp_path / "out", True, downsample=1.5)
    for cam, px in cams:
        want_i, want_m = _ingest_ref.ingest(R.resize_rgba(px, (26, 16)), True)
        check_camera(cam, (26, 16), want_i, want_m, fovy(26, 16))
    assert all((e["width"], e["height"]) == (26, 16) for e in cams_json)


@pytest.mark.gpu
@pytest.mark.parametrize("white", [False, True])
def test_resolution(scene_dir, tmp_path, white):
    sc, cams, cams_json = load(scene_dir, tmp_path / "out", white, resolution=2)
    for cam, px in cams:
        want_i, want_m = composite_then_bicubic(px, white, (20, 12))
        check_camera(cam, (20, 12), want_i, want_m, fovy(W, H))  # (the FoVs are the file's)
    for ci in sc.scene_info.train_cameras:
        assert (ci.width, ci.height) == (W, H)
    assert all((e["width"], e["height"]) == (W, H) for e in cams_json), "cameras.json carries the size before `resolution`"


@pytest.mark.gpu
def test_downsample_then_resolution(scene_dir, tmp_path):
    sc, cams, cams_json = load(scene_dir, tmp_path / "out", False, downsample=2.0, resolution=2)
    for cam, px in cams:
        want_i, want_m = composite_then_bicubic(R.resize_rgba(px, (20, 12)), False, (10, 6))
        check_camera(cam, (10, 6), want_i, want_m, fovy(20, 12))
    assert all((e["width"], e["height"]) == (20, 12) for e in cams_json)
    assert all((ci.width, ci.height) == (20, 12) for ci in sc.scene_info.train_cameras)


@pytest.mark.gpu
def test_resolution_as_a_width(scene_dir, tmp_path):
    """A `resolution` outside 1, 2, 4, 8 is a width: s = 40 / 30, (int(40 / s), int(24 / s)) = (30, 18)."""
    sc, cams, _ = load(scene_dir, tmp_path / "out", True, resolution=30)
    size = pkg("resample").target_size_resolution(W, H, 30)
    assert size == (30, 18)
    for cam, px in cams:
        want_i, want_m = composite_then_bicubic(px, True, size)
        check_camera(cam, size, want_i, want_m, fovy(W, H))


@pytest.mark.gpu
def test_nothing_resizes_is_the_plain_load(scene_dir, tmp_path):
    sc, cams, cams_json = load(scene_dir, tmp_path / "out", True, downsample=1.0, resolution=1)
    for cam, px in cams:
        want_i, want_m = _ingest_ref.ingest(px, True)
        check_camera(cam, (W, H), want_i, want_m, fovy(W, H))


@pytest.mark.gpu
def test_two_training_iterations_at_half_resolution(tmp_path):
    T = pkg("train")
    root = tmp_path / "scene"
    F.write_scene(str(root), pkg("synthetic"), n_train=4, n_test=1, W=48, H=48, points=F.ball_points(1000))
    cfg = T.merge_config(dict(source_path=str(root), model_path=str(tmp_path / "m"), eval=True, is_blender=True, white_background=False,
                              iterations=2, warm_up=1, dpsr_iter=10 ** 9, densify_from_iter=10 ** 9, log_every=2, resolution=2),
                         log=lambda *a: None)
    res = T.training(cfg, log=lambda *a: None)
    torch.cuda.synchronize()
    assert sorted(res["log"]) == [1, 2] and all(np.isfinite(v) for row in res["log"].values() for v in row.values())
    cams = res["scene"].getTrainCameras() + res["scene"].getTestCameras()
    assert all((c.image_width, c.image_height) == (24, 24) and c.original_image.shape == (3, 24, 24) and c.gt_alpha_mask.shape == (24, 24, 1)
               for c in cams)
    # testing() compares its renders with the 24 x 24 ground truth: another size would be refused by image_metrics
    assert res["test"] is not None and np.isfinite(res["test"]["gaussian"]["psnr"])
