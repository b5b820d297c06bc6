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
    permuted(verts, faces, points, "torus 40x20")


def permuted(verts, faces, points, what):
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
        print(f"permutation of {what}, max_dist {md}: {tie.sum()} queries moved to another face")
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


# ---- thin faces: marching-cubes spheres, split tori, sliver soups, micro triangles (tests/_surface_ref.py, qualified on the host by
# tests/test_surface_host.py) ---------------------------------------------------------------------------------------------------------------
def twice(points, verts, faces, max_dist, want, what):
    got = run(points, verts, faces, max_dist)
    same(got, want, what)
    again = run(points, verts, faces, max_dist)
    assert np.array_equal(got[0], again[0]) and np.array_equal(bits(got[1]), bits(again[1])) and np.array_equal(bits(got[2]), bits(again[2])), \
        what + ": a second call returned other bits"
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SR.SLIVER_CASES))
def test_thin_faces_bit_equal(name):
    """The brute force and the grid at 0.5, 2 and 10 mean edge lengths -- and, where the input has one sliver height h, at 3 h, between
    that height and the long edge -- against the statement, each twice.  Every bound leaves some queries unmatched and some not."""
    c = SR.sliver_case(name)
    verts, faces, points, ref = c["verts"], c["faces"], c["points"], c["ref"]
    ok = SR.face_ok(verts, faces)
    got = twice(points, verts, faces, math.inf, ref, f"{name}, brute force")
    assert ok[got[0][got[0] >= 0]].all()
    edge = mean_edge(verts, faces)
    bounds = [(f"{k} mean edges", k * edge) for k in (0.5, 2.0, 10.0)]
    if name in SR.SLIVER_HEIGHT:
        bounds.append(("3 h", 3 * SR.SLIVER_HEIGHT[name]))
    for label, max_dist in bounds:
        want = blank(ref, max_dist)
        assert 0 < (want[0] >= 0).sum() < len(points), label  # the bound cuts
        got = twice(points, verts, faces, max_dist, want, f"{name}, max_dist {label} = {max_dist:.3e}")
        assert ok[got[0][got[0] >= 0]].all()


@pytest.mark.gpu
def test_micro_triangles_follow_the_candidate_rule():
    """Edges from 1e-9 to 1e-22: |n|^2 normal, denormal and 0 in fp32.  The faces the device ever chooses are candidates of the
    statement (len > 0 with denormals kept: a kernel that flushed them would refuse the 63 faces with a denormal |n|^2), every one of
    them is chosen by some query, and where the nearest geometry is a refused face the answer is the statement's other face."""
    c = SR.sliver_case("micro")
    verts, faces, points, ref = c["verts"], c["faces"], c["points"], c["ref"]
    ok = SR.face_ok(verts, faces)
    near64 = SR.closest64(points, verts, faces)[0]
    print(f"micro: {ok.sum()} of {len(faces)} faces are candidates; the float64 nearest face is a refused one for {(~ok[near64]).sum()} "
          f"of {len(points)} queries")
    assert (~ok[near64]).sum() > 100
    for max_dist in (math.inf, 10 * mean_edge(verts, faces)):
        got = run(points, verts, faces, max_dist)
        chosen = np.unique(got[0][got[0] >= 0])
        assert ok[chosen].all()
        same(got, blank(ref, max_dist), f"micro, max_dist {max_dist:.3e}")
        if math.isinf(max_dist):
            assert len(chosen) == ok.sum()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mc_sphere_1e-6", "split_torus_1e-6"])
def test_face_permutation_thin_faces(name):
    c = SR.sliver_case(name)
    permuted(c["verts"], c["faces"], c["points"], name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SR.SLIVER_CASES))
def test_face_geometry_shares_the_candidate_rule(name):
    """anchor.face_geometry on the same inputs: the normal is 0 exactly where the fp32 length of cross(v1 - v0, v2 - v0) is 0 in a
    numpy statement of its arithmetic -- the len > 0 rule that surface.hip takes over, denormal lengths included -- and the centroids
    ((v0 + v1) + v2) / 3 keep their bits."""
    c = SR.sliver_case(name)
    verts, faces = c["verts"], c["faces"]
    a, b, cc = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = b - a, cc - a
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        unit = np.where(ln[:, None] > 0, n / np.where(ln > 0, ln, np.float32(1))[:, None], np.float32(0))
        cent = ((a + b) + cc) / np.float32(3)
    got_c, got_n = (t.cpu().numpy() for t in pkg("anchor").face_geometry(dev(verts), dev(faces)))
    flat = (got_n == 0).all(1)
    print(f"{name}: {flat.sum()} of {len(faces)} normals are 0, the statement's length is 0 for {(ln == 0).sum()}; normals differing in "
          f"bits {(bits(got_n) != bits(unit)).any(1).sum()}, centroids {(bits(got_c) != bits(cent)).any(1).sum()}")
    assert np.array_equal(flat, ln == 0)
    assert np.array_equal(SR.face_ok(verts, faces), ~flat & np.isfinite(ln))  # the rule surface.hip shares
    assert np.array_equal(bits(got_c), bits(cent))
