"""The numpy restatement of the visualisation passes (tests/_visualize_ref.py) checked against geometry, and the host-side camera
code of dg-mesh_amd/visualize.py (trajectory poses, pose -> camera) checked against the reference's poses
(tests/golden/trajectory_poses.npz, written by tests/golden/make_trajectory_golden.py).  No GPU."""
import math
import os

import numpy as np
import pytest
import torch

import _meshrast_ref as MR
import _visualize_ref as VR
from conftest import ROOT, pkg
from test_mesh_raster import _tilt, uv_sphere

GOLDEN = os.path.join(ROOT, "tests", "golden", "trajectory_poses.npz")


def test_vertex_normals_of_a_sphere_are_radial():
    """Area-weighted normals of uv_sphere(32, 24): every vertex normal is the outward radial direction to within the
    discretisation (the largest facet subtends pi / 24 rad, so the deviation is far below that angle); in float32 too."""
    v, f = uv_sphere(32, 24, r=1.7)
    v = v @ _tilt().T
    for dtype in (np.float64, np.float32):
        n = VR.vertex_normals(v, f, dtype)
        assert n.dtype == dtype and np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6)
        cos = (n.astype(np.float64) * v / 1.7).sum(1)
        print(f"{dtype.__name__}: min cos(normal, radial) {cos.min():.6f}")
        assert cos.min() > math.cos(0.25 * math.pi / 24)
    extra = np.vstack([v, [[9.0, 9.0, 9.0]]])
    f2 = np.vstack([f, [[0, 0, 5]], [[1, 2, len(extra)]], [[-1, 2, 3]]])  # zero-area, two out-of-range faces, one unreferenced vertex
    n2 = VR.vertex_normals(extra, f2)
    assert np.array_equal(n2[:-1], VR.vertex_normals(v, f)) and np.array_equal(n2[-1], np.zeros(3))


def _analytic_sphere(cam, px, py, r, light, m):
    """Phong colour (before the clamp) of the unit-normal sphere of radius r at the origin under pixel centre (px + .5, py + .5)."""
    W, H = cam.image_width, cam.image_height
    inv = np.linalg.inv(cam.full_proj_transform.astype(np.float64))
    ndc = np.array([(px + 0.5) / (0.5 * W) - 1.0, (py + 0.5) / (0.5 * H) - 1.0])
    a, b = np.array([*ndc, 0.2, 1.0]) @ inv, np.array([*ndc, 0.8, 1.0]) @ inv
    a, b = a[:3] / a[3], b[:3] / b[3]
    o, d = cam.camera_center.astype(np.float64), (b - a) / np.linalg.norm(b - a)
    bq, cq = o @ d, o @ o - r * r
    disc = bq * bq - cq
    if disc <= 0:
        return None
    p = o + (-bq - math.sqrt(disc)) * d
    n = p / r
    ndl = n @ light
    view = (o - p) / np.linalg.norm(o - p)
    spec = max(view @ (2 * ndl * n - light), 0.0) ** m["shininess"] if ndl > 0 else 0.0
    return m["ambient"] + m["diffuse"] * max(ndl, 0.0) + m["specular"] * spec


def test_headlight_on_a_sphere():
    """The restated shading of uv_sphere(48, 36) under the headlight, on a float64 brute-force rast: the pixel whose normal faces the
    camera is ambient + k_d + k_s before the clamp, the value falls monotonically along the centre row towards the silhouette and
    follows the analytic sphere; at the silhouette (n.l = 0) the rule gives ambient.  Discretisation: the mesh's interpolated
    normals deviate from the sphere's by < 0.25 (pi / 36)^2 ~ 2e-3 rad inside a facet and its surface lies up to
    1 - cos(pi / 48) ~ 2e-3 r inside the sphere, which moves a pixel's normal by ~2e-3 / sqrt(1 - rho^2) near the rim; 0.02 covers
    both for every pixel more than one pixel inside the silhouette."""
    syn = pkg("synthetic")
    H = W = 65
    cam = syn.make_camera(W, H, radius=4.0)
    v, f = uv_sphere(48, 36, r=1.0)
    v = v @ _tilt().T
    pos = torch.tensor(np.hstack([v, np.ones((len(v), 1))]) @ cam.full_proj_transform.astype(np.float64))
    tri = torch.tensor(f)
    ids, zw, _ = MR.rasterize_ids(pos, tri, H, W)
    u, w1, z = MR.barycentrics(pos, tri, ids, H, W)
    rast = torch.stack([u, w1, z, ids.to(torch.float64)], -1).numpy()
    m = VR.MATERIAL
    light = VR.headlight(v, cam.camera_center)
    img = VR.shade(v, VR.vertex_normals(v, f), f, rast, light, cam.camera_center, clamp=False)
    top = m["ambient"] + m["diffuse"] + m["specular"]
    cy = cx = W // 2
    print(f"centre pixel {img[cy, cx, 0]:.6f} vs ambient + k_d + k_s = {top:.6f}")
    assert abs(img[cy, cx, 0] - top) < 2e-3 and np.array_equal(img[..., 0], img[..., 1])
    covered = np.nonzero(ids[cy].numpy() > 0)[0]
    row = img[cy, cx:covered.max() + 1, 0]
    assert len(row) > 8 and (ids[cy, cx:covered.max() + 1] > 0).all()
    assert (np.diff(row) <= 1e-3).all(), row
    for k, val in enumerate(row[:-1]):
        ref = _analytic_sphere(cam, cx + k, cy, 1.0, light, m)
        assert ref is not None and abs(val - ref) < 0.02, (k, val, ref)
    assert row[-1] < row[0] - 0.2 and row[-1] >= m["ambient"] - 1e-12
    assert np.array_equal(img[0, 0], np.ones(3)) and img[ids.numpy() > 0].min() >= m["ambient"] - 1e-12
    # at grazing incidence the rule is ambient exactly; a back-facing normal gets no diffuse and no highlight
    one = np.array([[[1.0, 0.0, 0.5, 1.0]]])
    tv, tf = np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 1, 0]]), np.array([[0, 1, 2]])
    for nrm, expect in (((0.0, 0, 1), top), ((0.0, 1, 0), m["ambient"]), ((0.0, 0, -1), m["ambient"])):
        got = VR.shade(tv, np.tile(nrm, (3, 1)), tf, one, np.array([0.0, 0, 1]), np.array([0.0, 0, 5.0]), clamp=False)[0, 0, 0]
        assert abs(got - expect) < 1e-12, (nrm, got, expect)


def test_compose_bytes():
    blk = np.zeros((3, 2, 2), np.float32)
    blk[0] = [[0.1, 0.2], [0.3, 0.4]]            # mean 0.25 -> 63.75 -> 63
    blk[1] = [[1.0, 1.0], [1.0, 254.5 / 255]]    # just below 1 -> 254
    blk[2] = [[-3.0, 0.0], [0.0, 0.0]]           # negative mean -> 0
    assert VR.compose([blk], 2).tolist() == [[[63, 254, 0]]]
    full = VR.compose([blk, np.transpose(blk, (1, 2, 0))], 1)
    assert full.shape == (2, 4, 3) and np.array_equal(full[:, :2], full[:, 2:])
    assert full[:, :2, 0].tolist() == [[25, 51], [76, 102]] and full[1, 1, 1] == 254 and full[0, 0, 2] == 0
    odd = np.array([0.0, 1.0, 0.999999, 254.5 / 255, -1.0, 7.0, np.nan, 0.5], np.float32)
    img = np.broadcast_to(odd[None, :, None], (1, 8, 3)).copy()
    assert VR.compose([img], 1)[0, :, 0].tolist() == [0, 255, 254, 254, 0, 255, 0, 127]


def test_trajectory_poses_equal_the_reference():
    V = pkg("visualize")
    g = np.load(GOLDEN)
    for key in ("a", "b"):
        args = (float(g[key + "/radius"]), float(g[key + "/elevation"]), int(g[key + "/total_frames"]))
        ref = g[key + "/poses"]
        for name, mine in (("visualize", V.trajectory_poses(*args, look_at=g[key + "/look_at"])),
                           ("restatement", VR.trajectory_poses(*args, look_at=g[key + "/look_at"]))):
            err = np.abs(mine - ref).max()
            print(f"{key} {name}: max |pose - reference| {err:.3e}")
            assert mine.shape == ref.shape and err <= 1e-12
    with pytest.raises(ValueError):
        V.trajectory_poses(1.0, 1.0, 4)
    with pytest.raises(ValueError):
        V.trajectory_poses(1.0, -2.0, 4)


@pytest.mark.parametrize("key", ["a", "b"])
def test_trajectory_cameras_look_at_the_target(key):
    """The look-at point projects to the image centre (to 1e-4 px, through the float32 matrices) and camera_center is the eye; the
    view matrix equals the restated conversion of the reference's pose."""
    V, syn = pkg("visualize"), pkg("synthetic")
    g = np.load(GOLDEN)
    W, H = 176, 144
    template = syn.make_camera(W, H, fid=0.25)
    n, look = int(g[key + "/total_frames"]), g[key + "/look_at"]
    cams = V.trajectory_cameras(float(g[key + "/radius"]), float(g[key + "/elevation"]), n, template, look_at=look)
    assert len(cams) == n
    for i, cam in enumerate(cams):
        pose = g[key + "/poses"][i]
        assert (cam.image_width, cam.image_height, cam.FoVx, cam.FoVy) == (W, H, template.FoVx, template.FoVy)
        assert cam.fid == i / n and cam.world_view_transform.dtype == np.float32
        assert np.abs(cam.camera_center - pose[:3, 3]).max() <= 1e-6 * 4
        assert np.abs(cam.world_view_transform - VR.world_view_from_pose(pose)).max() <= 4 * 2.0 ** -24 * 4
        sx, sy = VR.project_pixels(cam.full_proj_transform, W, H, look)
        print(f"{key}[{i}]: look-at at ({sx:.6f}, {sy:.6f}) px")
        assert abs(sx - W / 2) < 1e-4 and abs(sy - H / 2) < 1e-4
        # a point above the target (world +z) lands above it in the image (smaller row: row 0 is the top, as the training cameras)
        _, sy_up = VR.project_pixels(cam.full_proj_transform, W, H, look + np.array([0.0, 0.0, 0.3]))
        assert sy_up < sy - 1.0
    same = V.camera_from_pose(g[key + "/poses"][0], template)
    assert same.fid == template.fid
