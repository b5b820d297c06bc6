"""GPU tests of mesh repair (dg-mesh_amd/mesh_repair.py, csrc/mesh_repair.hip) against the numpy restatement tests/_repair_ref.py.
Every case runs twice; the two runs and the reference are compared byte for byte: faces', flipped, verts' (the centroids too) and
every count.  The arithmetic is specified to the rounding (integer volume sums, one fp64 sum in loop order per centroid), so there is
no tolerance anywhere except the winding number at a sphere's centre, which is mesh_inside's own (8 x what the fp32 statement of its
definition loses against fp64 on the same mesh)."""
import numpy as np
import pytest
import torch

import _edges_ref as E
import _inside_ref as I
import _repair_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu


def M():
    return pkg("mesh_repair")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
    assert a.tobytes() == b.tobytes(), f"{what}: {int((a.view(np.uint8) != b.view(np.uint8)).sum())} bytes differ"


def as_mesh(verts, faces):
    return np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)


def check_orient(verts, faces, outward=True):
    """orient_faces twice against the reference -> the reference's (faces', flipped, info)."""
    verts, faces = as_mesh(verts, faces)
    ref = R.orient(verts, faces, outward)
    for run in range(2):
        f, flipped, info = M().orient_faces(dev(verts), dev(faces), outward=outward)
        assert info == ref[2], f"counts (run {run}): {info} against {ref[2]}"
        assert flipped.dtype == torch.bool
        same(host(flipped), ref[1], f"flipped (run {run})")
        same(host(f), ref[0], f"faces (run {run})")
    return ref


def check_fill(verts, faces, max_hole_edges=1000):
    verts, faces = as_mesh(verts, faces)
    ref = R.fill(verts, faces, max_hole_edges)
    for run in range(2):
        v, f, info = M().fill_holes(dev(verts), dev(faces), max_hole_edges=max_hole_edges)
        assert info == ref[2], f"counts (run {run}): {info} against {ref[2]}"
        same(host(v), ref[0], f"verts (run {run})")
        same(host(f), ref[1], f"faces (run {run})")
    return ref


def check_repair(verts, faces, **kw):
    """repair_mesh (one edge table, the flip bits) against the reference's orient-then-fill on the oriented mesh."""
    verts, faces = as_mesh(verts, faces)
    ref = R.repair(verts, faces, kw.get("orient", True), kw.get("outward", True), kw.get("max_hole_edges", 1000))
    for run in range(2):
        v, f, info = M().repair_mesh(dev(verts), dev(faces), **kw)
        assert info == ref[2], f"counts (run {run}): {info} against {ref[2]}"
        same(host(v), ref[0], f"verts (run {run})")
        same(host(f), ref[1], f"faces (run {run})")
    return ref


def E_flip(faces, which):
    return R.flip_some(faces, which)


def consistent(faces, V):
    return E.edge_table(faces, V)["info"]["misoriented_edges"] == 0


# ---- orientation -------------------------------------------------------------------------------------------------------------------
def test_icosphere_with_a_third_flipped():
    verts, faces = E.icosphere(3)
    which = np.random.default_rng(11).random(len(faces)) < 1 / 3
    out, flipped, info = check_orient(verts, E_flip(faces, which))
    same(out, faces, "the sphere is restored")
    assert (flipped == which).all() and info["faces_flipped"] == int(which.sum()) and info["components"] == info["closed_components"] == 1
    # face 0 may itself be among the flipped: then the volume rule, not the count, turns the component
    assert info["components_inverted"] == int(which[0])


def test_icosphere_inside_out_only_the_volume_rule_acts():
    verts, faces = E.icosphere(3)
    inverted = E_flip(faces, np.ones(len(faces), bool))
    out, flipped, info = check_orient(verts, inverted)
    same(out, faces, "turned outwards")
    assert flipped.all() and info["components_inverted"] == 1 and info["outward_skipped"] == 0
    out, flipped, info = check_orient(verts, inverted, outward=False)  # consistent already: nothing to do
    same(out, inverted, "left inside out")
    assert not flipped.any() and info["components_inverted"] == 0


def test_torus():
    verts, faces = E.torus()
    which = np.random.default_rng(2).random(len(faces)) < 0.4
    out, _, info = check_orient(verts, E_flip(faces, which))
    assert consistent(out, len(verts)) and E.enclosed_volume(verts, out) > 0 and info["closed_components"] == 1


def test_open_patch_minority_and_tie():
    verts, faces = E.grid_patch(7, 11)
    F = len(faces)  # 120
    rng = np.random.default_rng(3)
    minority = np.zeros(F, bool)
    minority[rng.permutation(F)[:F // 4]] = True
    out, flipped, info = check_orient(verts, E_flip(faces, minority))
    same(out, faces, "the minority is flipped back")
    assert info["closed_components"] == 0 and info["components_inverted"] == 0
    for keep_first in (True, False):  # exactly half: the orientation that keeps face 0 wins
        half = np.zeros(F, bool)
        half[rng.permutation(np.arange(1, F))[:F // 2 - (0 if keep_first else 1)]] = True
        half[0] = not keep_first
        assert half.sum() == F // 2
        out, flipped, info = check_orient(verts, E_flip(faces, half))
        assert not flipped[0] and info["faces_flipped"] == F // 2 and consistent(out, len(verts))
        same(flipped, half if keep_first else ~half, "the tie keeps the smallest face")


def test_moebius_strip_is_left_alone():
    verts, faces = R.moebius()
    out, flipped, info = check_orient(verts, faces)
    same(out, faces, "unchanged")
    assert not flipped.any() and info["unorientable_components"] == 1 and info["components"] == 1 and info["closed_components"] == 0


@pytest.mark.parametrize("name", ["bow_tie", "fan", "same_winding_pair"])
def test_small_bad_meshes(name):
    verts, faces = getattr(E, name)()
    out, flipped, info = check_orient(verts, faces)
    want = {"bow_tie": (2, 0), "fan": (3, 0), "same_winding_pair": (1, 1)}[name]  # (components, flips)
    assert (info["components"], info["faces_flipped"]) == want
    if name == "same_winding_pair":
        assert flipped.tolist() == [False, True] and consistent(out, len(verts))  # a tie: face 0 stays


def test_closed_inverted_sphere_beside_an_open_patch():
    sv, sf = E.icosphere(2)
    pv, pf = E.grid_patch(4, 5)
    verts = np.concatenate([pv + np.float32([3, 0, 0]), sv])
    rng = np.random.default_rng(8)
    some = np.zeros(len(pf), bool)
    some[rng.permutation(len(pf))[:5]] = True
    faces = np.concatenate([E_flip(pf, some), E_flip(sf + len(pv), np.ones(len(sf), bool))])
    out, flipped, info = check_orient(verts, faces)
    same(out, np.concatenate([pf, sf + len(pv)]), "both restored")
    assert (info["components"], info["closed_components"], info["components_inverted"]) == (2, 1, 1)


def test_permuted_faces_give_the_same_flip_set():
    verts, faces = E.icosphere(3)
    which = np.random.default_rng(12).random(len(faces)) < 0.3
    flippedfaces = E_flip(faces, which)
    _, flipped, _ = check_orient(verts, flippedfaces)
    perm = np.random.default_rng(13).permutation(len(faces))
    _, flipped_p, _ = check_orient(verts, flippedfaces[perm])
    same(flipped_p, flipped[perm], "the flip set, mapped back through the permutation")


def test_invalid_faces_are_passed_through():
    verts, faces = E.icosphere(2)
    V = len(verts)
    which = np.random.default_rng(14).random(len(faces)) < 0.3
    bad = np.array([[-1, 0, 1], [0, 1, V], [2, 2, 3], [4, 4, 4]], np.int32)
    at = [0, 17, 17, 200]
    mixed = np.insert(E_flip(faces, which), at, bad, axis=0)
    out, flipped, info = check_orient(verts, mixed)
    invalid = ~E.valid_faces(mixed, V)
    assert invalid.sum() == 4 and not flipped[invalid].any()
    same(out[invalid], mixed[invalid], "invalid faces untouched")
    same(out[~invalid], faces, "the sphere is restored")


def test_non_finite_vertex_skips_the_volume_rule():
    verts, faces = E.icosphere(1)
    verts = verts.copy()
    verts[5, 1] = np.nan
    _, _, info = check_orient(verts, E_flip(faces, np.arange(len(faces)) % 3 == 0))
    assert info["outward_skipped"] == 1 and info["components_inverted"] == 0


# ---- holes -------------------------------------------------------------------------------------------------------------------------
def watertight(verts, faces):
    return pkg("mesh_topology").topology_report(dev(verts), dev(faces))


def centre_winding_is_one(verts, faces):
    """The winding number at the sphere's centre is +1 within mesh_inside's own tolerance (tests/test_mesh_inside.py): 8 x the largest
    |w32 - w64| of the numpy fp32 statement of its definition, taken over the centre and 255 queries in the mesh's box."""
    queries = np.concatenate([np.zeros((1, 3), np.float32), I.box_queries(verts, 255, seed=1)])
    w64, w32 = I.winding(queries, verts, faces, np.float64), I.winding(queries, verts, faces, np.float32)
    tol = 8.0 * float(np.abs(w32.astype(np.float64) - w64).max())
    w = host(pkg("mesh_inside").winding_number(dev(queries), dev(verts), dev(faces))).astype(np.float64)
    print(f"winding number at the centre: device {w[0]!r}, fp64 {w64[0]!r}; device max |w - w64| {np.abs(w - w64).max():.3e}, tolerance {tol:.3e}")
    assert abs(w64[0] - 1.0) <= 1e-12  # the fp64 statement on a closed mesh wound outwards
    assert np.abs(w - w64).max() <= tol and abs(w[0] - 1.0) <= tol


def test_triangular_holes():
    verts, faces = R.icosphere_without_faces()
    v, f, info = check_fill(verts, faces)
    assert (info["holes_filled"], info["verts_added"], info["faces_added"], info["boundary_edges"]) == (3, 0, 3, 9)
    full = E.icosphere(2)[1]
    assert sorted(map(tuple, np.sort(f, 1))) == sorted(map(tuple, np.sort(full, 1)))  # the removed faces are back
    v, f, _ = check_repair(verts, faces)
    rep = watertight(v, f)
    assert rep["watertight"] and rep["genus"] == 0
    centre_winding_is_one(v, f)


def test_vertex_stars_removed():
    verts, faces = R.icosphere_without_stars()
    v, f, info = check_fill(verts, faces)
    assert (info["holes_filled"], info["verts_added"], info["faces_added"], info["boundary_edges"]) == (3, 3, 17, 17)  # 5 + 6 + 6
    v, f, _ = check_repair(verts, faces)
    rep = watertight(v, f)
    assert rep["watertight"] and rep["genus"] == 0 and rep["verts_used"] == len(v) - 3  # the old centres stay, unused
    centre_winding_is_one(v, f)


@pytest.mark.parametrize("limit", [999, 1000, 1001])
def test_wheel_rim_at_the_limit(limit):
    verts, faces = E.wheel(1000)
    perm = np.random.default_rng(6).permutation(len(verts))  # new label of every vertex: the leader sits somewhere on the rim
    pv = np.empty_like(verts)
    pv[perm] = verts
    pf = perm[faces].astype(np.int32)
    v, f, info = check_fill(pv, pf, limit)
    filled = limit >= 1000
    assert (info["holes_filled"], info["holes_too_long"], info["faces_added"], info["verts_added"]) == ((1, 0, 1000, 1) if filled else (0, 1, 0, 0))
    if filled:
        assert watertight(v, f)["watertight"]


def test_touching_holes_are_skipped_and_counted():
    verts, faces = R.touching_holes()
    v, f, info = check_fill(verts, faces)
    assert (info["boundary_edges"], info["edges_on_open_chains"], info["holes_filled"], info["faces_added"]) == (6, 6, 0, 0)
    same(f, faces, "unchanged")


def test_isolated_triangles_become_pillows():
    verts, faces = R.isolated_triangles(1400)  # 4200 boundary half-edges: past one scan tile of 4096
    v, f, info = check_repair(verts, faces)
    assert (info["boundary_edges"], info["holes_filled"], info["faces_added"], info["verts_added"]) == (4200, 1400, 1400, 0)
    same(f[1400:], faces[:, [1, 0, 2]], "every triangle gets its mirror image")
    rep = watertight(v, f)
    assert rep["watertight"] and rep["components"] == 1400


def test_marching_cubes_sphere_cut_by_the_grid_box():
    n = 24
    i = torch.arange(n, dtype=torch.float32, device="cuda")
    x, y, z = torch.meshgrid(i, i, i, indexing="ij")
    c = (n - 1) / 2.0
    field = torch.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - 0.55 * n  # pokes through all six sides
    verts, faces = (host(t) for t in pkg("marching_cubes").marching_cubes(field.contiguous()))
    _, cycles, chain_edges = R.holes(faces, len(verts))
    rims = sorted(len(c) for c in cycles)
    print(f"marching cubes at {n}^3: V {len(verts)} F {len(faces)} rims {rims}")
    assert len(rims) == 6 and chain_edges == 0 and rims[0] >= 4
    v, f, info = check_repair(verts, faces, max_hole_edges=rims[0] - 1)
    assert info["holes_filled"] == 0 and info["holes_too_long"] == 6 and len(f) == len(faces)
    v, f, info = check_repair(verts, faces, max_hole_edges=rims[-1])
    assert info["holes_filled"] == 6 and info["verts_added"] == 6
    rep = watertight(v, f)
    assert rep["watertight"] and rep["genus"] == 0


def test_repair_orients_then_fills_on_one_edge_table():
    """A punctured sphere with a third of its faces flipped: the rim's half-edges follow the flip bits."""
    verts, faces = R.icosphere_without_stars(3, (0, 632, 634, 641))
    which = np.random.default_rng(15).random(len(faces)) < 1 / 3
    v, f, info = check_repair(verts, E_flip(faces, which))
    assert info["holes_filled"] == 4 and info["faces_flipped"] in (int(which.sum()), int((~which).sum()))
    rep = watertight(v, f)
    assert rep["watertight"] and rep["genus"] == 0
    check_repair(verts, E_flip(faces, which), orient=False)  # the broken rims are skipped and counted


def test_apply_carries_attributes():
    verts, faces = R.icosphere_without_stars()
    color = np.random.default_rng(16).random((len(verts), 3)).astype(np.float32)
    spec = M().RepairSpec()
    v, f, c, none = M().apply(spec, dev(verts), dev(faces), dev(color), None)
    rv, rf, _ = R.repair(verts, faces)
    same(host(v), rv, "verts")
    same(host(f), rf, "faces")
    assert none is None and c.shape == (len(rv), 3)
    same(host(c[:len(verts)]), color, "given rows")
    for k in range(len(verts), len(rv)):
        rim = rf[(rf[:, 2] == k), 1]
        np.testing.assert_allclose(host(c[k]), color[rim].mean(0), rtol=0, atol=1e-6)  # a mean of 5 or 6 numbers in [0, 1], fp32
    assert M().apply(None, v, f, c) == (v, f, c)


# ---- empty meshes, arguments -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["no_vertices", "no_faces", "all_faces_invalid", "faces_without_vertices"])
def test_empty_meshes(case):
    verts, faces = {"no_vertices": (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)),
                    "no_faces": (np.ones((5, 3), np.float32), np.zeros((0, 3), np.int32)),
                    "all_faces_invalid": (np.ones((5, 3), np.float32), np.array([[0, 0, 1], [-1, 2, 3], [1, 2, 5], [4, 4, 4]], np.int32)),
                    "faces_without_vertices": (np.zeros((0, 3), np.float32), np.array([[0, 1, 2]], np.int32))}[case]
    out, flipped, info = check_orient(verts, faces)
    same(out, faces, "faces")
    assert not flipped.any() and info["components"] == 0 and info["outward_skipped"] == 1
    assert check_orient(verts, faces, outward=False)[2]["outward_skipped"] == 0
    v, f, info = check_fill(verts, faces)
    assert info == dict.fromkeys(R.FILL_FIELDS, 0)
    v, f, info = check_repair(verts, faces)
    same(v, verts, "verts")
    same(f, faces, "faces")


def test_argument_errors():
    v = torch.zeros((4, 3), device="cuda")
    f = torch.zeros((2, 3), dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="int32"):
        M().orient_faces(v, f.long())
    with pytest.raises(RuntimeError, match="float32"):
        M().fill_holes(v.double(), f)
    with pytest.raises(ValueError, match=r"\(F, 3\)"):
        M().repair_mesh(v, f.reshape(3, 2))
    for bad in (-1, 2.5, 2 ** 31):
        with pytest.raises(ValueError, match="max_hole_edges"):
            M().fill_holes(v, f, max_hole_edges=bad)
