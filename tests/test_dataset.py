"""dataset.read_blender_scene on a scene the test writes (tests/_scene_fixture.py): cameras against synthetic.make_camera, whose poses
the scene's transform matrices encode; fid, the eval split, cameras_extent against its closed form, the point clouds, and the
parts that are deliberately not built.  Host only."""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

import _png_ref
import _scene_fixture as F
from conftest import pkg


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("blender_scene")
    items = F.write_scene(str(root), pkg("synthetic"), n_train=6, n_test=2, W=48, H=48)
    return str(root), items


def test_cameras_equal_make_camera(scene_dir):
    D = pkg("dataset")
    root, items = scene_dir
    info = D.read_blender_scene(root, white_background=True, eval=True)
    assert len(info.train_cameras) == 6 and len(info.test_cameras) == 2
    for split, infos in (("train", info.train_cameras), ("test", info.test_cameras)):
        for k, (ci, (want, _)) in enumerate(zip(infos, items[split])):
            cam = D.make_camera(ci)
            assert (cam.image_width, cam.image_height) == (48, 48) and ci.uid == k and ci.image_name == f"r_{k:03d}"
            assert cam.fid == pytest.approx(want.fid, abs=1e-12) and ci.fid == cam.fid
            assert abs(cam.FoVx - want.FoVx) <= 1e-6 and abs(cam.FoVy - want.FoVy) <= 1e-6
            for name in ("world_view_transform", "full_proj_transform", "camera_center"):
                got, ref = getattr(cam, name), getattr(want, name)
                assert got.dtype == np.float32 and got.shape == ref.shape
                assert np.abs(got.astype(np.float64) - ref).max() <= 1e-6, (split, k, name)
            # R is kept transposed, T is the world-to-camera translation (dataset_readers.py:283-284)
            w2c = want.world_view_transform.T.astype(np.float64)
            assert np.abs(ci.R.T - w2c[:3, :3]).max() <= 1e-6 and np.abs(ci.T - w2c[:3, 3]).max() <= 1e-6


def test_eval_false_folds_the_test_frames_in(scene_dir):
    D = pkg("dataset")
    root, items = scene_dir
    info = D.read_blender_scene(root, white_background=False, eval=False)
    assert len(info.train_cameras) == 8 and info.test_cameras == []
    assert [c.fid for c in info.train_cameras] == pytest.approx([c.fid for c, _ in items["train"] + items["test"]])


@pytest.mark.parametrize("ev", [True, False])
def test_cameras_extent_closed_form(scene_dir, ev):
    D = pkg("dataset")
    root, items = scene_dir
    info = D.read_blender_scene(root, eval=ev)
    used = items["train"] + ([] if ev else items["test"])
    centers = np.stack([c.camera_center.astype(np.float64) for c, _ in used])
    mean = centers.mean(0)
    want = 1.1 * np.linalg.norm(centers - mean, axis=1).max()
    assert info.cameras_extent == pytest.approx(want, rel=1e-6)
    assert np.abs(info.translate + mean).max() <= 1e-6


def test_default_point_cloud_is_seeded_and_goes_to_model_path(scene_dir, tmp_path):
    D, ply = pkg("dataset"), pkg("ply_io")
    root, _ = scene_dir
    before = sorted(os.listdir(root))
    a = D.read_blender_scene(root, eval=True, model_path=str(tmp_path / "out"))
    b = D.read_blender_scene(root, eval=True)
    assert sorted(os.listdir(root)) == before, "the reader wrote into the dataset directory"
    assert a.ply_path == str(tmp_path / "out" / "input.ply") and b.ply_path is None
    pts, col = a.point_cloud.points, a.point_cloud.colors
    assert pts.shape == (100_000, 3) and pts.dtype == np.float32 and col.shape == (100_000, 3)
    assert np.array_equal(pts, b.point_cloud.points) and np.array_equal(col, b.point_cloud.colors)
    rng = np.random.RandomState(0)
    xyz = rng.random_sample((100_000, 3)) * 2.6 - 1.3
    shs = rng.random_sample((100_000, 3)) / 255.0
    assert np.array_equal(pts, xyz.astype(np.float32)) and np.abs(pts).max() <= 1.3
    assert np.array_equal(col, ((shs * 0.28209479177387814 + 0.5) * 255).astype(np.uint8) / 255.0)
    assert not np.any(a.point_cloud.normals)
    assert not np.array_equal(D.read_blender_scene(root, eval=True, seed=1).point_cloud.points, pts)
    v = ply.read_ply(a.ply_path)["vertex"]  # storePly's layout
    assert v.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue")
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), pts) and np.array_equal(v["red"] / 255.0, col[:, 0])


def test_points3d_ply_is_used_when_present(tmp_path):
    D = pkg("dataset")
    pts = F.ball_points(n=50)
    F.write_scene(str(tmp_path), pkg("synthetic"), n_train=2, n_test=1, W=12, H=12, points=pts)
    info = D.read_blender_scene(str(tmp_path), eval=True, model_path=str(tmp_path / "out"))
    assert info.ply_path == str(tmp_path / "points3d.ply") and not os.path.exists(tmp_path / "out" / "input.ply")
    assert np.array_equal(info.point_cloud.points, pts[0]) and np.array_equal(info.point_cloud.colors, pts[1] / 255.0)


def test_non_square_image_keeps_camera_angle_x(tmp_path):
    """The reference swaps the names (FovY = fovx; FovX = fovy); here FoVx is the file's angle and FoVy follows from the aspect."""
    D, syn = pkg("dataset"), pkg("synthetic")
    items = F.write_scene(str(tmp_path), syn, n_train=2, n_test=1, W=40, H=24)
    info = D.read_blender_scene(str(tmp_path), eval=True)
    for ci, (want, _) in zip(info.train_cameras, items["train"]):
        assert (ci.width, ci.height) == (40, 24)
        assert ci.FoVx == F.FOVX and ci.FoVy == pytest.approx(2 * math.atan(math.tan(F.FOVX / 2) * 24 / 40), abs=1e-12)
        assert ci.FoVy < ci.FoVx
        cam = D.make_camera(ci)
        assert np.abs(cam.full_proj_transform.astype(np.float64) - want.full_proj_transform).max() <= 1e-6


def test_what_is_not_built_raises_by_name(scene_dir):
    D = pkg("dataset")
    root, _ = scene_dir
    with pytest.raises(NotImplementedError, match="downsample"):
        D.read_blender_scene(root, downsample=2.0)
    info = D.read_blender_scene(root, eval=True)
    D.check_resolution(-1, info.train_cameras)
    D.check_resolution(1, info.train_cameras)
    for r in (2, 4, 8, 400):
        with pytest.raises(NotImplementedError, match="resolution"):
            D.check_resolution(r, info.train_cameras)
    with pytest.raises(NotImplementedError, match="resolution"):
        D.check_resolution(-1, [info.train_cameras[0]._replace(width=1601)])
    assert set(D.READERS) == {"Blender", "Nerfies", "iPhone", "NeuralActor"}
    for name in ("Nerfies", "iPhone", "NeuralActor"):
        args = SimpleNamespace(data_type=name, source_path=root)
        assert D.scene_type(args) == name
        with pytest.raises(NotImplementedError, match=name):
            D.READERS[name](root, False, True)
    assert D.scene_type(SimpleNamespace(data_type="", source_path=root)) == "Blender"
    with pytest.raises(NotImplementedError):
        D.scene_type(SimpleNamespace(data_type="Colmap", source_path=root))
    with pytest.raises(ValueError):
        D.scene_type(SimpleNamespace(data_type="", source_path=os.path.dirname(root)))


def test_cameras_json_entry(scene_dir):
    D = pkg("dataset")
    root, items = scene_dir
    ci = D.read_blender_scene(root, eval=True).train_cameras[1]
    e = D.camera_to_json(7, ci)
    want = items["train"][1][0]
    assert e["id"] == 7 and e["img_name"] == "r_001" and (e["width"], e["height"]) == (48, 48)
    assert np.abs(np.array(e["position"]) - want.camera_center).max() <= 1e-5
    assert e["fx"] == pytest.approx(48 / (2 * math.tan(F.FOVX / 2))) and e["fy"] == pytest.approx(e["fx"])
    json.dumps(e)


def test_the_fixture_files_decode_to_their_pixels(scene_dir):
    root, items = scene_dir
    with open(os.path.join(root, "train", "r_002.png"), "rb") as fh:
        assert np.array_equal(_png_ref.decode_png(fh.read()), items["train"][2][1])
