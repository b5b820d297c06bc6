"""Host-side qualification of tests/_surface_ref.py, the fp32 statement that csrc/surface.hip is held to bit for bit
(tests/test_surface_kernels.py), and the parts of dg-mesh_amd/correspondence.py that need no device.

The fp32 statement cannot agree with float64 on the INDEX of the closest face: a query above a shared edge or vertex has two or more
faces at the same distance up to rounding (417 of the 4200 queries below differ).  What it must get right is the distance, and the
face it picks must be as close as the closest up to rounding.  Both are measured in units of E(d) = eps S (d + eps S) (eps = 2^-24, S
the largest |coordinate|, d the float64 distance): the rounding of a squared distance whose terms are differences of coordinates of
size S.  Measured with this file's restatement on exactly this seeded input (numpy on the CPU):
    |min d2 (fp32) - min d2 (fp64)| / E(d)                       2.33   (over all N x F pairs: 7.68)
    (fp64 d2 of the face fp32 chose - fp64 min d2) / E(d)        0.70
The assertions allow twice the measured values; the slack is for numpy builds, the inputs are seeded."""
import math

import numpy as np
import pytest
import torch

import _surface_ref as SR
from conftest import pkg

EPS = 2.0 ** -24
K_MIN, K_CHOSEN = SR.K_MIN, SR.K_CHOSEN


@pytest.fixture(scope="module")
def qualified():
    verts, faces, points = SR.torus_input()
    return verts, faces, points, SR.closest32(points, verts, faces), SR.closest64(points, verts, faces)


def test_input_is_the_stated_one(qualified):
    verts, faces, points, _, _ = qualified
    assert verts.shape == (800, 3) and faces.shape == (1600, 3) and points.shape == (4200, 3)
    assert verts.dtype == np.float32 and points.dtype == np.float32 and faces.dtype == np.int32
    assert SR.face_ok(verts, faces).all()
    # a closed manifold: every undirected edge is used by exactly two faces
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1)
    assert (np.unique(e, axis=0, return_counts=True)[1] == 2).all()


def test_fp32_statement_against_fp64(qualified):
    verts, faces, points, (f32, d32, b32), (f64, d64, b64) = qualified
    d = np.sqrt(d64)
    E = SR.error_unit(verts, points, d)
    r_min = np.abs(d32.astype(np.float64) - d64) / E
    D64 = SR.pair_d2(points, verts, faces, np.float64)
    r_chosen = (D64[np.arange(len(points)), f32] - d64) / E
    print(f"fp32 vs fp64: min d2 ratio {r_min.max():.3f} (bound {K_MIN}), chosen-face excess ratio {r_chosen.max():.3f} "
          f"(bound {K_CHOSEN}), argmin differs for {(f32 != f64).sum()} of {len(points)}")
    assert (f32 >= 0).all() and (f64 >= 0).all() and np.isfinite(d32).all()
    assert r_min.max() <= K_MIN
    assert r_chosen.min() >= 0 and r_chosen.max() <= K_CHOSEN


def test_barycentrics_are_a_point_of_the_face(qualified):
    """bary within [-4 eps, 1 + 4 eps] ((1 - v) - w rounds twice at magnitude <= 1, v + w may exceed 1 by the rounding of den), and
    the point they rebuild in float64 lies at the float64 distance up to 8 eps S: v, w and (1 - v) - w carry two roundings of eps
    each, every one displacing the point by at most eps S (measured: 0.86 eps S)."""
    verts, faces, points, (f32, d32, b32), (_, d64, _) = qualified
    assert b32.min() >= -4 * EPS and b32.max() <= 1 + 4 * EPS
    v = verts.astype(np.float64)
    f = faces[f32]
    b = b32.astype(np.float64)
    q = v[f[:, 0]] * b[:, 0:1] + v[f[:, 1]] * b[:, 1:2] + v[f[:, 2]] * b[:, 2:3]
    S = max(np.abs(verts).max(), np.abs(points).max())
    err = np.abs(np.sqrt(((points.astype(np.float64) - q) ** 2).sum(1)) - np.sqrt(d64))
    print(f"rebuilt point: |distance - fp64 distance| max {err.max() / (EPS * S):.3f} eps S")
    assert err.max() <= 8 * EPS * S
    # the special queries: on a vertex, an edge midpoint or a centroid the distance is of rounding size
    assert np.sqrt(d64[3000:3300]).max() == 0.0 and np.sqrt(d64[3300:3900]).max() <= 4 * EPS * S


def test_strict_bound():
    """A face at exactly d2 == max_d2 is not reported; the next float above admits it."""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    p = np.array([[0.25, 0.25, 0.5], [0.25, 0.25, -0.75]], np.float32)
    face, d2, bary = SR.closest32(p, verts, faces)
    assert face.tolist() == [0, 0] and d2.tolist() == [0.25, 0.5625] and np.array_equal(bary[0], np.float32([0.5, 0.25, 0.25]))
    face, d2, bary = SR.closest32(p, verts, faces, max_d2=np.float32(0.25))
    assert face.tolist() == [-1, -1] and np.isinf(d2).all() and not bary.any()
    face, d2, _ = SR.closest32(p, verts, faces, max_d2=np.nextafter(np.float32(0.25), np.float32(1)))
    assert face.tolist() == [0, -1] and d2[0] == 0.25 and np.isinf(d2[1])
    C = pkg("correspondence")
    assert C.max_d2_of(0.5) == 0.25 and C.max_d2_of(math.inf) == math.inf and C.max_d2_of(0.1) == float(np.float32(0.1 * 0.1))


def test_every_region_and_its_barycentrics():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    p = np.array([[-1, -1, 0], [2, -0.5, 0], [-0.5, 2, 0], [0.5, -1, 0], [-1, 0.5, 0], [1, 1, 0], [0.25, 0.5, 2]], np.float32)
    _, d2, bary = SR.closest32(p, verts, faces)
    want = np.float32([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5], [0.25, 0.25, 0.5]])
    assert np.array_equal(bary, want) and d2.tolist() == [2.0, 1.25, 1.25, 1.0, 1.0, 0.5, 4.0]


def test_refused_faces_are_never_chosen():
    """Zero-area faces (repeated index, collinear corners), out-of-range indices and a face with a non-finite corner: no query picks
    them, at any distance, even where they would be closer than every real face."""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [0, 0, 5], [1, 0, 5], [0, 1, 5], [np.inf, 0, 0], [np.nan, 1, 1]], np.float32)
    faces = np.array([[0, 0, 1], [0, 1, 3], [0, 1, 9], [-1, 1, 2], [0, 1, 7], [0, 2, 8], [4, 5, 6]], np.int32)
    assert SR.face_ok(verts, faces).tolist() == [False] * 6 + [True]
    p = np.array([[0.2, 0.2, 0.1], [0.5, 0.0, 0.0], [0.3, 0.3, 5.5]], np.float32)
    face, d2, _ = SR.closest32(p, verts, faces)
    assert face.tolist() == [6, 6, 6] and np.allclose(d2, [4.9 ** 2, 25.0, 0.25])
    face, d2, bary = SR.closest32(p, verts, faces[:6])
    assert (face == -1).all() and np.isinf(d2).all() and not bary.any()
    face, _, _ = SR.closest32(p, verts[:0], faces)
    assert (face == -1).all()


def test_ties_go_to_the_smaller_face_index():
    verts, faces = SR.torus(8, 6)
    two = np.concatenate([faces, faces])
    p = np.random.RandomState(1).uniform(-1.5, 1.5, (200, 3)).astype(np.float32)
    a, b = SR.closest32(p, verts, faces), SR.closest32(p, verts, two)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    perm = np.random.RandomState(2).permutation(len(faces))
    c = SR.closest32(p, verts, faces[perm])
    assert np.array_equal(a[1], c[1])


def test_palette_parity_at_cell_borders():
    """u cells is exact at the borders k / 8 of an 8-cell checker: the border itself belongs to the upper cell, the float below it to
    the lower; u = 1 is cell 8."""
    c, s = np.zeros(3, np.float32), np.float32(1.0)
    below = lambda x: np.nextafter(np.float32(x), np.float32(-9))
    u = np.float32([[0.75, 0.0, 0.0], [below(0.75), 0.0, 0.0], [0.125, 0.125, 0.0], [1.0, 1.0, 1.0], [0.999, 0.0, 0.0], [5.0, -7.0, 0.5]])
    x = (u - np.float32(0.5)) * np.float32(2.0)  # exact (the differences are Sterbenz's): u -> x -> u round-trips for these values
    rgb, chk = SR.palette32(x, c, s, "rgb"), SR.palette32(x, c, s, "checker", 8)
    uc = np.clip(u, 0, 1)
    assert np.array_equal(rgb[[0, 2, 3, 5]], uc[[0, 2, 3, 5]])
    odd = [False, True, False, False, True, False]  # k = 6, 5, 2, 24, 7, 8 + 0 + 4
    for row, o in enumerate(odd):
        assert np.array_equal(chk[row], rgb[row] * (np.float32(0.55) if o else np.float32(1))), row
    lost = SR.palette32(np.float32([[np.nan, 0, 0], [0, 0, np.nan]]), c, s, "checker")
    assert np.array_equal(lost, np.float32([[1, 0, 1], [1, 0, 1]]))
    assert np.array_equal(SR.palette32(np.float32([[1, 2, 3]]), np.float32([1, 2, 3]), np.float32(0.0)), np.float32([[1, 0, 1]]))


def test_interp32_rows():
    verts, faces = SR.torus(6, 4)
    face = np.array([0, -1, 5, len(faces)], np.int32)
    bary = np.float32([[1, 0, 0], [0.2, 0.3, 0.5], [0.25, 0.25, 0.5], [1, 0, 0]])
    out = SR.interp32(verts, faces, face, bary, fill=-7.0)
    assert np.array_equal(out[0], verts[faces[0, 0]]) and (out[[1, 3]] == -7.0).all()
    f = faces[5]
    assert np.array_equal(out[2], (verts[f[0]] * np.float32(0.25) + verts[f[1]] * np.float32(0.25)) + verts[f[2]] * np.float32(0.5))
    assert np.isnan(SR.interp32(verts[:, 0], faces, face, bary)[1]).all()


def test_python_layer_refuses_without_a_device():
    C = pkg("correspondence")
    verts, faces = SR.torus(6, 4)
    v, f, p = torch.tensor(verts), torch.tensor(faces), torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        C.closest_on_mesh(p, v, f)
    with pytest.raises(RuntimeError, match="no CPU path"):
        C.interpolate(v, f, torch.zeros(5, dtype=torch.int32), torch.zeros(5, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        C.palette(p, (0, 0, 0), 1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        C.to_canonical(p, 0.5, None)
    with pytest.raises(ValueError, match="max_dist"):
        C.closest_on_mesh(p, v, f, max_dist=-1.0)
    with pytest.raises(ValueError, match="max_dist"):
        C.closest_on_mesh(p, v, f, max_dist=math.nan)
    with pytest.raises(ValueError, match="mode"):
        C.palette(p, (0, 0, 0), 1.0, mode="stripes")
    with pytest.raises(ValueError, match="cells"):
        C.palette(p, (0, 0, 0), 1.0, mode="checker", cells=0)
    with pytest.raises(ValueError, match="mode must be one of"):
        C.export_correspondence(None, None, None, None, "unused", mode="sideways")
    with pytest.raises(ValueError, match="n_tracks"):
        C.export_correspondence(None, None, None, None, "unused", n_tracks=0)
    with pytest.raises(RuntimeError, match="MeshPhase with a DPSR module"):
        C.export_correspondence(None, None, None, None, "unused")


def test_c_abi_argument_errors_without_gpu():
    """Sizes and NULL pointers are refused before any launch; the scratch size is a pure function of (N, F) that covers the 8 F
    references, the 48-byte corners and the table."""
    L = pkg("_lib")
    lib = L.lib()
    assert lib.dgm_surf_closest_scratch_bytes(-1, 5) == 0 and lib.dgm_surf_closest_scratch_bytes(5, -1) == 0
    a, b = lib.dgm_surf_closest_scratch_bytes(1000, 5000), lib.dgm_surf_closest_scratch_bytes(1000, 5000)
    assert a == b and a >= 5000 * (8 * 4 + 48) + 3 * 8192 * 4 + 4 * 1000 * 4
    assert lib.dgm_surf_closest_scratch_bytes(1000, 5001) >= a
    assert lib.dgm_surf_closest(0, 0, 0, None, None, None, 1.0, None, None, None, None, None) == 0
    assert lib.dgm_surf_closest(-1, 0, 0, None, None, None, 1.0, None, None, None, None, None) != 0
    assert b"surf_closest" in lib.dgm_last_error()
    assert lib.dgm_surf_closest(5, 3, 1, None, None, None, 1.0, None, None, None, None, None) != 0
    assert b"NULL" in lib.dgm_last_error()
    assert lib.dgm_surf_interp(0, 0, 0, 3, None, None, None, None, 0.0, None, None) == 0
    assert lib.dgm_surf_interp(4, 3, 1, 0, None, None, None, None, 0.0, None, None) != 0
    assert lib.dgm_corr_palette(0, None, None, None, 1, 8, None, None) == 0
    assert lib.dgm_corr_palette(4, None, None, None, 2, 8, None, None) != 0 and b"mode" in lib.dgm_last_error()
    assert lib.dgm_corr_palette(4, None, None, None, 1, 0, None, None) != 0 and b"cells" in lib.dgm_last_error()
    assert lib.dgm_corr_palette(4, None, None, None, 1, 8, None, None) != 0 and b"NULL" in lib.dgm_last_error()
