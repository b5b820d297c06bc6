"""csrc/surface.hip on the GPU against its fp32 statement tests/_surface_ref.py (qualified against float64 by
tests/test_surface_host.py): face, d2 and bary of correspondence.closest_on_mesh are compared BIT FOR BIT, on the grid path (finite
max_dist) and on the brute force (inf); interpolate and palette likewise.  The statement's bounded answer is its unbounded one with
the rows at d2 >= max_d2 blanked (the minimum over the faces with d2 < max_d2 is the overall minimum when that is below the bound, and
nothing otherwise), so one dense evaluation per input serves every bound."""
import math

import numpy as np
import pytest
import torch

import _surface_ref as SR
from conftest import pkg

DEV = "cuda"


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def run(points, verts, faces, max_dist=math.inf):
    C = pkg("correspondence")
    face, d2, bary = C.closest_on_mesh(dev(points, torch.float32).reshape(-1, 3), dev(verts, torch.float32).reshape(-1, 3),
                                       dev(faces, torch.int32).reshape(-1, 3), max_dist)
    assert face.dtype == torch.int32 and d2.dtype == torch.float32 and bary.shape == (len(points), 3)
    return face.cpu().numpy(), d2.cpu().numpy(), bary.cpu().numpy()


def blank(ref, max_dist):
    """The statement's answer under a bound, from its unbounded one (module docstring)."""
    face, d2, bary = (a.copy() for a in ref)
    out = ~(d2 < np.float32(pkg("correspondence").max_d2_of(max_dist)))
    face[out], d2[out], bary[out] = -1, np.inf, 0
    return face, d2, bary


def same(got, ref, what):
    nf = (got[0] != ref[0]).sum()
    nd = (bits(got[1]) != bits(ref[1])).sum()
    nb = (bits(got[2]) != bits(ref[2])).any(1).sum()
    print(f"{what}: N {len(ref[0])}, found {(ref[0] >= 0).sum()}; differing face {nf}, d2 {nd}, bary {nb}")
    assert nf == 0 and nd == 0 and nb == 0, what


def mean_edge(verts, faces):
    e = np.concatenate([verts[faces[:, 0]] - verts[faces[:, 1]], verts[faces[:, 1]] - verts[faces[:, 2]]])
    return float(np.sqrt((e.astype(np.float64) ** 2).sum(1)).mean())


@pytest.fixture(scope="module")
def torus_case():
    verts, faces, points = SR.torus_input()
    return verts, faces, points, SR.closest32(points, verts, faces)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [0.5, 2.0, 10.0, math.inf])
def test_torus_input_bit_equal(torus_case, scale):
    verts, faces, points, ref = torus_case
    max_dist = scale * mean_edge(verts, faces)
    got = run(points, verts, faces, max_dist)
    want = blank(ref, max_dist)
    if scale == 0.5:
        assert 0 < (want[0] >= 0).sum() < len(points)  # the bound cuts
    same(got, want, f"torus 40x20, max_dist {scale} mean edges")
    again = run(points, verts, faces, max_dist)
    assert all(np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)
               for a, b in zip(got, again)), "a second call returned other bits"


@pytest.mark.gpu
def test_sizes_at_the_tile_edges():
    """F and N around the 256-face LDS tile, the 64-lane wave and the 256-thread workgroup, on both paths."""
    verts, faces = SR.torus(16, 9)
    rng = np.random.RandomState(3)
    pts = rng.uniform(-1.5, 1.5, (257, 3)).astype(np.float32)
    max_dist = 0.6
    for F in (1, 2, 255, 256, 257):
        ref = SR.closest32(pts, verts, faces[:F])
        for N in (1, 63, 64, 65, 257):
            sub = tuple(a[:N] for a in ref)
            same(run(pts[:N], verts, faces[:F]), sub, f"brute F {F} N {N}")
            same(run(pts[:N], verts, faces[:F], max_dist), blank(sub, max_dist), f"grid F {F} N {N}")


@pytest.mark.gpu
def test_empty_inputs():
    verts, faces = SR.torus(6, 4)
    pts = np.zeros((5, 3), np.float32)
    for max_dist in (math.inf, 1.0):
        face, d2, bary = run(pts, verts, faces[:0], max_dist)
        assert (face == -1).all() and np.isinf(d2).all() and not bary.any()
        face, d2, bary = run(pts[:0], verts, faces, max_dist)
        assert face.shape == (0,) and d2.shape == (0,) and bary.shape == (0, 3)
        face, d2, bary = run(pts, verts[:0], faces, max_dist)
        assert (face == -1).all() and np.isinf(d2).all()
    face, d2, bary = run(pts, verts, faces, 0.0)
    assert (face == -1).all() and np.isinf(d2).all() and not bary.any()


@pytest.mark.gpu
def test_refused_faces_and_one_huge_face():
    """50 zero-area faces, two with an index out of range and one face spanning the whole box: the refused faces are never chosen
    (some lie closer to queries than any real face), and the huge face inflates the cell edge to its own size -- every face lands in
    a handful of cells, which is slow and still exact."""
    verts, faces = SR.torus(12, 8)
    rng = np.random.RandomState(4)
    V = len(verts)
    extra_v = np.float32([[-2, -2, -1], [2, -2, -1], [0, 2, 1]])
    rep = rng.randint(0, V, (50, 2))
    zero_area = np.stack([rep[:, 0], rep[:, 1], rep[:, 0]], 1)
    bad = np.array([[0, 1, V + 3], [-1, 2, 3]])
    huge = np.array([[V, V + 1, V + 2]])
    faces2 = np.concatenate([zero_area[:25], faces[:100], bad, huge, faces[100:], zero_area[25:]]).astype(np.int32)
    verts2 = np.concatenate([verts, extra_v])
    ok = SR.face_ok(verts2, faces2)
    assert (~ok).sum() == 52
    pts = np.concatenate([rng.uniform(-2, 2, (600, 3)), verts[rep[:, 0]] * 0.5 + verts[rep[:, 1]] * 0.5]).astype(np.float32)
    ref = SR.closest32(pts, verts2, faces2)
    assert ok[ref[0]].all() and (ref[0] == 127).sum() > 10
    same(run(pts, verts2, faces2), ref, "refused faces, brute")
    for max_dist in (0.05, 0.4):
        same(run(pts, verts2, faces2, max_dist), blank(ref, max_dist), f"refused faces + huge face, max_dist {max_dist}")


@pytest.mark.gpu
def test_tiny_faces_in_a_large_box():
    """64 faces of size 1e-3 scattered over a box of 10: thousands of cells per axis hashed into 64 buckets (collisions), cell
    coordinates far from the origin."""
    rng = np.random.RandomState(5)
    c = rng.uniform(-5, 5, (64, 3))
    verts = (c[:, None, :] + 1e-3 * rng.standard_normal((64, 3, 3))).reshape(-1, 3).astype(np.float32)
    faces = np.arange(192, dtype=np.int32).reshape(64, 3)
    pts = np.concatenate([c[rng.randint(0, 64, 400)] + 1e-3 * rng.standard_normal((400, 3)), rng.uniform(-5, 5, (100, 3))]).astype(np.float32)
    ref = SR.closest32(pts, verts, faces)
    for max_dist in (2e-3, 5e-2):
        want = blank(ref, max_dist)
        assert 300 < (want[0] >= 0).sum() < 500
        same(run(pts, verts, faces, max_dist), want, f"tiny faces, max_dist {max_dist}")


@pytest.mark.gpu
def test_all_queries_in_one_cell(torus_case):
    verts, faces, _, _ = torus_case
    rng = np.random.RandomState(6)
    pts = (np.float32([1.4, 0.0, 0.02]) + 1e-3 * rng.standard_normal((300, 3))).astype(np.float32)
    ref = SR.closest32(pts, verts, faces)
    max_dist = 2 * mean_edge(verts, faces)
    want = blank(ref, max_dist)
    assert (want[0] >= 0).all()
    same(run(pts, verts, faces, max_dist), want, "one cell")


@pytest.mark.gpu
def test_larger_run():
    """torus 80 x 40 (F 6400) against 4096 queries under a bound: several scan tiles' worth of buckets, 16 workgroups of queries."""
    verts, faces = SR.torus(80, 40)
    rng = np.random.RandomState(7)
    f = faces[rng.randint(0, len(faces), 4096)]
    b = rng.dirichlet((1, 1, 1), 4096)
    pts = (verts[f[:, 0]] * b[:, 0:1] + verts[f[:, 1]] * b[:, 1:2] + verts[f[:, 2]] * b[:, 2:3] + 0.05 * rng.standard_normal((4096, 3))).astype(np.float32)
    ref = SR.closest32(pts, verts, faces)
    max_dist = mean_edge(verts, faces)
    want = blank(ref, max_dist)
    assert 1000 < (want[0] >= 0).sum() < 4096
    same(run(pts, verts, faces, max_dist), want, "torus 80x40")


@pytest.mark.gpu
def test_face_permutation(torus_case):
    """Under a permutation of the faces d2 and bary keep their bits and the indices map through it -- except on equal-d2 ties, where
    the smaller NEW index wins and only d2 is compared."""
    verts, faces, points, _ = torus_case
    perm = np.random.RandomState(8).permutation(len(faces))
    max_dist = 2 * mean_edge(verts, faces)
    for md in (max_dist, math.inf):
        a, b = run(points, verts, faces, md), run(points, verts, faces[perm], md)
        assert np.array_equal(bits(a[1]), bits(b[1]))
        found = a[0] >= 0
        assert np.array_equal(found, b[0] >= 0)
        mapped = np.where(found, perm[np.where(found, b[0], 0)], -1)
        tie = mapped != a[0]
        D = SR.pair_d2(points[tie], verts, faces, np.float32)
        rows = np.arange(tie.sum())
        print(f"permutation, max_dist {md}: {tie.sum()} queries moved to another face")
        assert np.array_equal(D[rows, mapped[tie]], D[rows, a[0][tie]]) and np.array_equal(D[rows, a[0][tie]], a[1][tie])
        assert np.array_equal(bits(a[2][~tie]), bits(b[2][~tie]))


@pytest.mark.gpu
def test_interpolate_and_palette_bit_equal(torus_case):
    C = pkg("correspondence")
    verts, faces, points, ref = torus_case
    face, _, bary = blank(ref, 0.5 * mean_edge(verts, faces))
    assert (face < 0).any() and (face >= 0).any()
    rng = np.random.RandomState(9)
    for attr in (verts, rng.standard_normal((len(verts), 5)).astype(np.float32), np.arange(len(verts), dtype=np.float32)):
        for fill in (math.nan, -2.5):
            got = C.interpolate(dev(attr), dev(faces), dev(face), dev(bary), fill=fill).cpu().numpy()
            want = SR.interp32(attr, faces, face, bary, fill).reshape(got.shape)
            assert got.shape == (len(face),) + attr.shape[1:] and np.array_equal(bits(got), bits(want))
    closest = C.interpolate(dev(verts), dev(faces), dev(ref[0]), dev(ref[2])).cpu().numpy()
    err = np.abs(((points - closest).astype(np.float64) ** 2).sum(1) - ref[1]).max()
    print(f"interpolate(verts) against d2: max |difference| {err:.3e}")
    assert err <= 1e-6
    xyz = np.concatenate([points, np.float32([[np.nan, 0, 0], [0, np.nan, 0], [0.1, 0.2, np.nan], [np.inf, 0, 0], [-np.inf, 0, 0]])])
    center, scale = np.float32([0.05, -0.1, 0.0]), np.float32(1.7)
    for mode, cells in (("rgb", 8), ("checker", 8), ("checker", 5), ("checker", 1)):
        got = C.palette(dev(xyz), dev(center), dev(scale).reshape(1), mode=mode, cells=cells).cpu().numpy()
        want = SR.palette32(xyz, center, scale, mode, cells)
        assert np.array_equal(bits(got), bits(want)), (mode, cells)
        assert np.array_equal(got[len(points):len(points) + 3], np.float32([[1, 0, 1]] * 3))
    host = C.palette(dev(xyz), tuple(float(c) for c in center), float(scale), mode="checker").cpu().numpy()
    assert np.array_equal(bits(host), bits(SR.palette32(xyz, center, scale, "checker", 8)))
    assert C.palette(dev(xyz[:0]), center, scale).shape == (0, 3)
