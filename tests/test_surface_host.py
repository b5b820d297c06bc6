"""Host-side qualification of tests/_surface_ref.py, the fp32 statement that csrc/surface.hip is held to bit for bit
(tests/test_surface_kernels.py), and the parts of dg-mesh_amd/correspondence.py that need no device.

The fp32 statement cannot agree with float64 on the INDEX of the closest face: a query above a shared edge or vertex has two or more
faces at the same distance up to rounding (417 of the 4200 queries below differ).  What it must get right is the distance, and the
face it picks must be as close as the closest up to rounding.  Both are measured in units of E(d) = eps S (d + eps S) (eps = 2^-24, S
the largest |coordinate|, d the float64 distance): the rounding of a squared distance whose terms are differences of coordinates of
size S.  Measured with this file's restatement on exactly this seeded input (numpy on the CPU):
    |min d2 (fp32) - min d2 (fp64)| / E(d)                       2.33   (over all N x F pairs: 7.68)
    (fp64 d2 of the face fp32 chose - fp64 min d2) / E(d)        0.70
The assertions allow twice the measured values; the slack is for numpy builds, the inputs are seeded.

Thin faces.  A torus has none; a marching-cubes mesh has them wherever the isosurface grazes a lattice node, and there the rounding of
the products that form va, vb, vc exceeds |n|^2, so v and w of the interior rule are not accurate.  The second half of this file
holds the statement to what the kernel's candidate-set argument needs of it on such input, and measures
its accuracy there.  Inputs (tests/_surface_ref.py, seeded; V / F; faces with thinness = height / longest edge below 1e-3 / 1e-5):
    mc_sphere(delta), delta 1e-3, 1e-5, 1e-6       678 / 1352     0 / 0 (thinnest 1.64e-3: 48 below 2e-3), 96 / 0, 96 / 72; edges down to 8.4e-8
    split_torus(h), h 1e-4, 1e-6, 1e-7             1200 / 2400    400 / 0, 400 / 400, 400 / 400
    sliver_soup(500, 1e-2, h, S), h 1e-5, 3e-7,    1500 / 500     245 to 500 / 0 to 500; at h below the float32 spacing up to 48 faces
      3e-8, S 1, 10                                               are collinear in float32 and refused
    micro_triangles()                              624 / 208      |n|^2 normal for 12 faces, denormal for 63, zero for 133
each with sliver_queries: 3 x 400 points on thin faces displaced by 0, 1e-6, 1e-4, 1200 near faces, every vertex, 16 far points.
Measured with numpy on the CPU, over all 5.0e7 (query, candidate face) pairs:
    q leaves the face's exact AABB by at most            1.92 * 2^-24 S_face   (the argument allows 16, the box is widened by 32)
    v, w and (1 - v) - w of every pair lie in            [-1.0 eps, 1]         (asserted: [-4 eps, 1 + 4 eps])
    pairs with a NaN or infinite dist2                   none, except 74 + 19 on 45 micro triangles with a denormal |n|^2, where
                                                         den = 1 / ((va + vb) + vc) overflows; such a pair is never reported
    a query on a mesh vertex gets dist2 == 0             every vertex of the six meshes; corner A of every candidate face
    zero-displacement queries answered by a thin face    236, 141, 103 (mc_sphere), 42, 94, 127 (split_torus) of 400 (guard: 25)
    |fp32 - fp64 distance| of the mesh-wide minimum, in eps S (S per query) and in max(eps S, height of the chosen face):
        mc_sphere      847, 41, 7.2 eps S       0.32, 0.39, 0.39            (absolute: 4.0e-5, 1.9e-6, 3.4e-7)
        split_torus    528, 5.3, 1.2 eps S      0.36, 0.46, 0.52            (absolute: 4.4e-5, 4.4e-7, 2.3e-7)
        sliver_soup    71 to 73 160 eps S       4.3 to 73 160               (absolute: 4.2e-5 to 4.4e-3, up to 0.44 of the long edge)
The unit that stays bounded on the meshes is the second: the fp32 distance is off by up to half the height of the sliver it picks
(or eps S), because a neighbour across the sliver's long edges answers where the sliver's own v and w fail.  E(d) is the wrong unit
there (up to 5e5 E(d) at d = 0), and K_MIN / K_CHOSEN are not asserted on these inputs.  An ISOLATED sliver has no such neighbour: below
a thinness of about sqrt(eps) its closest point can be anywhere along it, in either unit without a bound; asserted there is what
the range of the barycentrics gives -- the fp32 distance is never below the true one by more than 8 eps S (measured 1.25) and never
above it by more than the longest edge of the closest face (measured 0.44 of it)."""
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


# ---- thin faces (module docstring, "Thin faces") --------------------------------------------------------------------------------------------
SLIVER, MESHES, SOUPS = list(SR.SLIVER_CASES), list(SR.MESH_CASES), list(SR.SOUP_CASES)
K_HEIGHT = 2 * 0.52  # |fp32 distance - fp64 distance| / max(eps S, height of the chosen face) on the six meshes: twice the measured
FLT_MIN = np.float32(2.0 ** -126)
_f64 = {}


def sliver64(name):
    """The float64 statement's answer on SR.sliver_case(name), once per process."""
    if name not in _f64:
        c = SR.sliver_case(name)
        _f64[name] = SR.closest64(c["points"], c["verts"], c["faces"])
    return _f64[name]


def normal_len2(verts, faces):
    """|n|^2 in fp32 by face_ok's operations."""
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        nx, ny, nz = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        return (nx * nx + ny * ny) + nz * nz


def longest_edge(verts, f):
    a, b, c = (verts[f[:, k]].astype(np.float64) for k in range(3))
    return np.sqrt(np.maximum(np.maximum(((b - a) ** 2).sum(1), ((c - b) ** 2).sum(1)), ((a - c) ** 2).sum(1)))


def test_sliver_inputs_are_the_stated_ones():
    assert np.float32(1e-40) * np.float32(1) != 0, "this numpy flushes denormals: the statement would not be the kernel's"
    for name in MESHES + SOUPS:
        verts, faces = SR.SLIVER_CASES[name]()
        assert verts.dtype == np.float32 and faces.dtype == np.int32
        th = SR.thinness(verts, faces)
        n = [(th < t).sum() for t in (1e-3, 1e-5)]
        e = np.sqrt(((verts[faces] - verts[faces[:, [1, 2, 0]]]).astype(np.float64) ** 2).sum(-1))
        print(f"{name}: V {len(verts)} F {len(faces)}, candidates {SR.face_ok(verts, faces).sum()}, thinness < 1e-3: {n[0]}, < 1e-5: {n[1]}, "
              f"thinnest {th.min():.2e}, shortest edge {e.min():.1e}")
        if name.startswith("mc"):
            assert verts.shape == (678, 3) and faces.shape == (1352, 3)
            edges = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1)
            assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()  # closed
            assert n == {"mc_sphere_1e-3": [0, 0], "mc_sphere_1e-5": [96, 0], "mc_sphere_1e-6": [96, 72]}[name]
            assert (th < SR.THIN.get(name, 1e-3)).sum() >= 48
        elif name.startswith("split"):
            assert verts.shape == (1200, 3) and faces.shape == (2400, 3) and n[0] == 400
            assert np.array_equal(verts[:800], SR.torus(40, 20)[0])
        else:
            assert verts.shape == (1500, 3) and faces.shape == (500, 3) and n[0] >= 245
    verts, faces = SR.micro_triangles()
    n2 = normal_len2(verts, faces)
    ok = SR.face_ok(verts, faces)
    classes = [(n2 >= FLT_MIN).sum(), ((n2 > 0) & (n2 < FLT_MIN)).sum(), (n2 == 0).sum()]
    print(f"micro: V {len(verts)} F {len(faces)}, |n|^2 normal {classes[0]}, denormal {classes[1]}, zero {classes[2]}; candidates {ok.sum()}")
    assert faces.shape == (208, 3) and np.abs(verts).max() <= 1e-3 and min(classes) >= 10
    assert np.array_equal(ok, n2 > 0)  # (sqrt of a positive denormal is positive: the rule accepts every denormal |n|^2)
    for name in SLIVER:
        assert len(SR.sliver_case(name)["points"]) == 2400 + len(SR.sliver_case(name)["verts"]) + SR.N_FAR


@pytest.mark.parametrize("name", SLIVER)
def test_sliver_structure(name):
    """What the candidate-set argument of DESIGN.md section 4.14 needs of the pair arithmetic, on thin faces:
      * bary within [-4 eps, 1 + 4 eps];
      * over every (query, candidate face) pair that can be reported (finite dist2), q leaves the face's exact AABB by at most
        16 * 2^-24 S_face, the constant of the argument (the boxes are widened by 32);
      * no candidate pair with a NaN dist2.  Not so on the micro triangles: where (va + vb) + vc, which is |n|^2 up to rounding, falls
        below 2^-128, den = 1 / that overflows, v and w are inf or 0 * inf, dist2 is inf or NaN and the face cannot be reported for
        that query.  Asserted there: only faces with a denormal |n|^2 do that;
      * a query equal to a mesh vertex gets dist2 == 0 exactly and a chosen face with a corner of those bits.  By the arithmetic that
        holds for corner A of a candidate face (rule 1: v = w = 0, q = a).  For corner B (rule 2) q = a + fl(b - a), which is b only
        where that difference and sum are exact: fl(b - a) is off by at most 2 eps S per axis and the sum rounds by eps S, 3 sqrt(3)
        eps S in all; likewise C by rule 4 -- unless rule 3 takes it first: at p = c, vc is |n|^2 up to rounding, on a sliver of
        either sign, and the answer is then the foot of c on ab, the face's height over ab away.  On the six meshes every vertex
        is at dist2 == 0 (asserted); of an isolated triangle corner A is, and B and C lie within 6 eps S, C's height more."""
    c = SR.sliver_case(name)
    verts, faces, points, (f32, d32, b32), chk = c["verts"], c["faces"], c["points"], c["ref"], c["check"]
    V = len(verts)
    ok = SR.face_ok(verts, faces)
    n2 = normal_len2(verts, faces)
    vq = slice(2400, 2400 + V)
    at_a, at_any = np.zeros(V, bool), np.zeros(V, bool)
    at_a[faces[ok, 0]], at_any[faces[ok].ravel()] = True, True
    zero = d32[vq] == 0
    corner = (verts[faces[np.maximum(f32[vq], 0)]] == points[vq][:, None, :]).all(2).any(1) & (f32[vq] >= 0)
    S = float(np.abs(verts).max())
    a, b, cc = (verts[faces[:, k]].astype(np.float64) for k in range(3))
    over_ab = np.sqrt((np.cross(b - a, cc - a) ** 2).sum(1)) / np.maximum(np.sqrt(((b - a) ** 2).sum(1)), 1e-300)
    allow = np.zeros(V)
    np.maximum.at(allow, faces[ok, 2], over_ab[ok])
    far = float(((np.sqrt(d32[vq].astype(np.float64)) - allow)[at_any]).max())
    print(f"{name}: bary in [{b32.min() / EPS:.2f} eps, 1 + {(b32.max() - 1) / EPS:.2f} eps], over all pairs in [{chk.bary_min / EPS:.2f} eps, "
          f"1 + {(chk.bary_max - 1) / EPS:.2f} eps] (bound 4); q leaves the AABB by "
          f"{chk.excursion:.3f} 2^-24 S_face (bound 16) over {chk.pairs} pairs; NaN dist2 {chk.nan_pairs}, inf {chk.inf_pairs}, on "
          f"{len(chk.bad_faces)} faces; vertices at dist2 == 0: {zero.sum()} of {V} ({at_any.sum()} on a candidate, {at_a.sum()} as its "
          f"corner A), the farthest of a candidate at its height as corner C + {far / (EPS * S):.2f} eps S (bound 6)")
    assert (f32 >= 0).all() and ok[f32].all()
    assert b32.min() >= -4 * EPS and b32.max() <= 1 + 4 * EPS
    assert chk.bary_min >= -4 * EPS and chk.bary_max <= 1 + 4 * EPS  # (of every pair, not only of the chosen ones)
    assert chk.excursion <= 16
    bad = np.array(sorted(chk.bad_faces), np.int64)
    if name == "micro":
        assert (n2[bad] < FLT_MIN).all()
    else:
        assert chk.nan_pairs == 0 and chk.inf_pairs == 0
    assert zero[at_a].all() and corner[at_a].all() and far <= 6 * EPS * S
    if name in MESHES:
        assert zero.all() and corner.all()


@pytest.mark.parametrize("name", MESHES)
def test_sliver_queries_reach_thin_faces(name):
    """The guard: of the 400 queries on thin faces without displacement at least 25 get a thin face as their answer -- the tests of
    this input cannot pass by never choosing one.  (A seed that gives fewer is replaced; the 25 stay.)"""
    c = SR.sliver_case(name)
    th = SR.thinness(c["verts"], c["faces"])
    thin = SR.THIN.get(name, 1e-3)
    n = int((th[c["ref"][0][:SR.N_ON]] < thin).sum())
    print(f"{name}: {n} of {SR.N_ON} chosen faces have thinness < {thin:g} (at least 25)")
    assert n >= 25


@pytest.mark.parametrize("name", SLIVER)
def test_sliver_accuracy_against_fp64(name):
    """|fp32 distance - fp64 distance| of the mesh-wide minimum, in units of (i) eps S and (ii) max(eps S, height of the face fp32
    chose).  (ii) stays bounded on the six meshes and is asserted there at twice the measured 0.52 (module docstring); (i) does not.
    On isolated slivers neither does, and what is asserted is what the arithmetic gives: bary is within rounding of [0, 1], so q is a
    point of the face and the fp32 distance no smaller than the true one up to 8 eps S, and no larger than it by more than the longest
    edge of the closest face.  The micro triangles are printed only: float64 accepts all 208 faces, fp32 75 of them."""
    c = SR.sliver_case(name)
    verts, faces, points, (f32, d32, _) = c["verts"], c["faces"], c["points"], c["ref"]
    f64, d64, _ = sliver64(name)
    S = np.maximum(np.abs(verts).max(), np.abs(points).max(1)).astype(np.float64)  # (per query: the far group would set it for all)
    diff = np.sqrt(d32.astype(np.float64)) - np.sqrt(d64)
    E = EPS * S * (np.sqrt(d64) + EPS * S)
    height = SR.thinness(verts, faces)[f32] * longest_edge(verts, faces[f32])
    r_s, r_h = np.abs(diff) / (EPS * S), np.abs(diff) / np.maximum(EPS * S, height)
    edge = longest_edge(verts, faces[f64])
    print(f"{name}: |fp32 - fp64 distance| max {np.abs(diff).max():.2e} = {r_s.max():.2f} eps S = {r_h.max():.2f} max(eps S, height) "
          f"(bound {K_HEIGHT} on the meshes); fp32 - fp64 in [{(diff / (EPS * S)).min():.2f} eps S, {(diff / edge).max():.3f} longest edges]; "
          f"|d2 (fp32) - d2 (fp64)| max {(np.abs(d32 - d64) / E).max():.1f} E(d); argmin differs for {(f32 != f64).sum()} of {len(points)}")
    if name in MESHES:
        assert r_h.max() <= K_HEIGHT
    elif name in SOUPS:  # (over the queries whose float64 face is a candidate in fp32 too)
        both = SR.face_ok(verts, faces)[f64]
        assert (diff / (EPS * S)).min() >= -8 and ((diff - edge) / (EPS * S))[both].max() <= 8
