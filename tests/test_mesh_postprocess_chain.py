"""GPU tests of the mesh post-processing chain on its own intermediate meshes: marching cubes, mesh_clean, mesh_smooth, mesh_simplify,
mesh_repair in the order of visualize.export_dynamic_mesh and MeshPhase.extract_mesh, then every consumer of the repaired mesh.

The field is tests/_chain_fixture.chain_field (five bodies and noise at 24^3).  THE INPUT OF STAGE k + 1 IS THE DEVICE'S OUTPUT OF
STAGE k, and the reference of stage k + 1 is evaluated on that same device output: tolerances never compound, and every stage is
judged exactly as its own test file judges it -- the comparisons are imported from those files, none is written here:
  marching cubes   test_marching_cubes._bit_exact              vertices and faces bit-equal
  clean            test_mesh_clean.check_mesh                  labels, table, keep mask, compaction byte for byte
  smooth           test_mesh_smooth.run / same                 byte for byte
  simplify         test_mesh_simplify.check                    faces and index maps byte for byte, vertices within its 2 ulp
  repair           test_mesh_repair.check_orient / check_fill / check_repair   byte for byte
  edge table       test_mesh_edges.check                       byte for byte (run on every intermediate mesh)
and on the repaired mesh (non-manifold edges, rims left open, an added rim vertex, ragged V and F)
  rays             test_mesh_ray.same_bits / check_against_fp64, 1000 rays, both paths, unbounded and [0.25, 1.5)
  winding number   test_mesh_inside's TOL_FACTOR x the fp32 restatement's deviation; classification outside MARGIN
  closest point    test_surface_kernels.same against closest32; test_correspondence's K_MIN / K_CHOSEN against closest64
  atlas            test_mesh_atlas.check at cell 6 and at a size that is no multiple of the cell
  AO bake          test_mesh_ray.ao_case (the fp64 count of the same rays)
Every helper runs its stage twice and compares the runs byte for byte; where a helper runs once, the test calls it twice.  The
conditions of tests/test_mesh_postprocess_chain_host.py are asserted again on the device's meshes."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import _chain_fixture as C
import _edges_ref as E
import _inside_ref as IR
import _meshclean_ref as RC
import _ray_ref as RAY
import _repair_ref as RR
import _simplify_ref as RS
import _surface_ref as SR
import _texture_ref as TX
import test_marching_cubes as TMC
import test_mesh_atlas as TAT
import test_mesh_clean as TCL
import test_mesh_edges as TED
import test_mesh_inside as TIN
import test_mesh_ray as TRY
import test_mesh_repair as TRP
import test_mesh_simplify as TSI
import test_mesh_smooth as TSM
import test_surface_kernels as TSK
from conftest import pkg
from test_redzone import L, run_case
from test_visualize import _record_psr, scene  # noqa: F401  (the tiny mesh-phase scene of the visualize tests, as a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = list(C.CASES)
N_QUERIES = 1000
AO_SAMPLES, AO_POINTS = 4, 600


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)  # (a copy: the shared meshes are read-only)


def host(t):
    return t.cpu().numpy()


same = TRP.same


# ---- the device's chain: raw calls, nothing asserted here; the tests hold every stage to its reference ---------------------------------
@functools.lru_cache(maxsize=None)
def device_head():
    """-> (field, mc, clean, smooth): the device's meshes (numpy, read-only), each stage fed the device's output of the one before."""
    field = C.reference_head()[0]
    v, f = TMC._gpu(field, 0.0, None, False)
    mc = (C.to_unit_box(v, C.N), f)
    cv, cf = (host(t) for t in pkg("mesh_clean").clean_mesh(dev(mc[0]), dev(mc[1]), **C.CLEAN))
    sv = host(pkg("mesh_smooth").smooth_mesh(dev(cv), dev(cf), **C.SMOOTH))
    out = (field, mc, (cv, cf), (sv, cf))
    for mesh in out[1:]:
        for a in mesh:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def device_tail(case):
    """-> (simplify, repair, repair's info): the device's meshes of a case."""
    sv, sf = device_head()[3]
    gv, gf = (host(t) for t in pkg("mesh_simplify").simplify_mesh(dev(sv), dev(sf), **C.CASES[case]))
    rv, rf, info = pkg("mesh_repair").repair_mesh(dev(gv), dev(gf))
    out = ((gv, gf), (host(rv), host(rf)), info)
    for mesh in out[:2]:
        for a in mesh:
            a.setflags(write=False)
    return out


def device_counts(verts, faces):
    return pkg("mesh_topology").EdgeTable("mesh_edges", dev(faces), len(verts)).info


def show(case, name, verts, faces, info, more=""):
    print(f"{case} {name}: V {len(verts)} F {len(faces)}; boundary {info['boundary_edges']} non-manifold {info['nonmanifold_edges']} "
          f"misoriented {info['misoriented_edges']} {more}")


# ---- the stages ---------------------------------------------------------------------------------------------------------------------------
def test_marching_cubes_on_the_field():
    field, (mv, mf) = device_head()[:2]
    v, f, _ = TMC._bit_exact(field, 0.0, None, False)
    v2, f2, _ = TMC._bit_exact(field, 0.0, None, False)
    same(v2, v, "vertices: run 1 against run 0")
    same(f2, f, "faces: run 1 against run 0")
    same(C.to_unit_box(v, C.N), mv, "the chain's vertices")
    same(f, mf, "the chain's faces")
    ref, rep = TED.check(mv, mf)
    show("all", "mc", mv, mf, ref["info"], f"components {rep['components']}")
    assert len(mf) > 4096  # more than one scan tile
    assert device_counts(mv, mf) == ref["info"] and ref["info"]["nonmanifold_edges"] == 0 and ref["info"]["boundary_edges"] > 0
    assert np.abs(mv).max() <= 1 and mv.dtype == np.float32


def test_clean_on_the_marching_cubes_mesh():
    _, (mv, mf), (cv, cf) = device_head()[:3]
    lab, tab = TCL.check_mesh(mv, mf, criteria=(C.CLEAN, {}, {"largest": True}, {"min_faces": 30, "min_diameter_frac": 0.1}))
    rv, rf, _, _ = RC.clean(mv, mf, **C.CLEAN)
    same(cv, rv, "the chain's vertices")
    same(cf, rf, "the chain's faces")
    ref, rep = TED.check(cv, cf)
    show("all", "clean", cv, cf, ref["info"], f"components {len(tab['label'])} -> {rep['components']}")
    assert 1 < rep["components"] < len(tab["label"]) and 0 < len(cf) < len(mf)  # the floaters went, several bodies stay
    assert rep["verts_used"] == len(cv)


def test_smooth_on_the_cleaned_mesh():
    _, _, (cv, cf), (sv, sf) = device_head()
    got = TSM.run(cv, cf, **C.SMOOTH)
    TSM.same(got, E.smooth(cv, cf, **C.SMOOTH), "taubin fixed x 3")
    same(got, sv, "the chain's vertices")
    for boundary in ("curve", "free"):  # the rim the grid box cuts moves under these two
        TSM.same(TSM.run(cv, cf, boundary=boundary, **C.SMOOTH), E.smooth(cv, cf, boundary=boundary, **C.SMOOTH), boundary)
    rim = (E.edge_table(cf, len(cv))["vert_flag"] & 2) != 0
    assert rim.sum() > 0 and np.array_equal(sv[rim], cv[rim]) and (sv[~rim] != cv[~rim]).any()
    print(f"all smooth: V {len(sv)} F {len(sf)}; rim vertices {int(rim.sum())}, largest move {float(np.abs(sv - cv).max()):.3e}")


@pytest.mark.parametrize("case", CASES)
def test_simplify_on_the_smoothed_mesh(case):
    sv, sf = device_head()[3]
    (gv, gf), _, _ = device_tail(case)
    kw = C.CASES[case]
    TSI.WORST["ulp"] = 0.0
    ref, got, info = TSI.check(sv, sf, **kw)
    print(f"{case} simplify: worst {TSI.WORST['ulp']:.2f} ulp of the box's largest coordinate (bound 2)")
    same(got["verts"], gv, "the chain's vertices")
    same(got["faces"], gf, "the chain's faces")
    if "target_faces" in kw:
        assert info["grid"] == ref["grid"] and tuple(info["grids_tried"]) == tuple(ref["grids_tried"]) and len(info["grids_tried"]) > 1
        assert len(gf) <= kw["target_faces"]
        print(f"{case} simplify: grid {info['grid']} after {info['count_passes']} passes")
    table, rep = TED.check(gv, gf)
    show(case, "simplify", gv, gf, table["info"], f"components {rep['components']}")
    assert device_counts(gv, gf) == table["info"] and table["info"]["nonmanifold_edges"] > 0 and 0 < len(gf) < 2000


@pytest.mark.parametrize("case", CASES)
def test_repair_on_the_simplified_mesh(case):
    (gv, gf), (rv, rf), dev_info = device_tail(case)
    of, flipped, orient_info = TRP.check_orient(gv, gf)
    TRP.check_orient(gv, gf, outward=False)
    TRP.check_fill(gv, gf)  # on the faces as they came: the rims that misoriented faces break are skipped and counted
    TRP.check_fill(gv, of)
    v, f, info = TRP.check_repair(gv, gf)
    TRP.check_repair(gv, gf, orient=False)
    same(v, rv, "the chain's vertices")
    same(f, rf, "the chain's faces")
    assert dev_info == info
    rims = sorted(len(c) for c in RR.holes(of, len(gv))[1])
    assert rims and rims[0] >= 3
    _, _, short = TRP.check_repair(gv, gf, max_hole_edges=rims[-1] - 1)  # the longest rim is then too long
    assert short["holes_too_long"] >= 1 and short["holes_filled"] == info["holes_filled"] - rims.count(rims[-1])
    print(f"{case} repair on V {len(gv)} F {len(gf)}: {info}; rims {rims}")
    assert info["components"] > 1 and info["holes_filled"] >= 1 and info["edges_on_open_chains"] > 0
    assert info["faces_flipped"] == int(flipped.sum()) == orient_info["faces_flipped"]
    table, rep = TED.check(rv, rf)
    show(case, "repair", rv, rf, table["info"], f"components {rep['components']} verts_used {rep['verts_used']}")
    assert device_counts(rv, rf) == table["info"] and table["info"]["misoriented_edges"] == 0 and table["info"]["nonmanifold_edges"] > 0
    assert len(rv) == len(gv) + info["verts_added"] and len(rf) == len(gf) + info["faces_added"] and info["verts_added"] >= 1


def test_conditions_that_one_case_must_meet():
    tails = {case: device_tail(case) for case in CASES}
    assert any(device_counts(*t[0])["misoriented_edges"] > 0 for t in tails.values())
    assert any(t[2]["faces_flipped"] > 0 for t in tails.values())
    # what the device produced is what the pure reference chain produces: faces equal, vertices within simplify's bound
    for case, ((gv, gf), (rv, rf), _) in tails.items():
        ref = C.reference_chain(case)
        same(gf, ref[3]["faces"], f"{case}: simplified faces against the reference chain")
        same(rf, ref[4]["faces"], f"{case}: repaired faces against the reference chain")
        assert np.abs(gv.astype(np.float64) - ref[3]["verts"]).max() <= TSI.tolerance(*device_head()[3])[0]


# ---- the consumers, on the repaired mesh -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_one_smooth_step_and_the_report_on_the_repaired_mesh(case):
    """The edge table and the report were held byte for byte in test_repair_on_the_simplified_mesh; one Laplacian step is one
    smooth_step (factor lam), with every boundary rule: lists over edges of three and more faces, rim vertices on open chains."""
    rv, rf = device_tail(case)[1]
    table = E.edge_table(rf, len(rv))
    assert ((table["vert_flag"] & 2) != 0).any() and ((table["vert_flag"] & 4) != 0).any()
    for boundary in E.BOUNDARIES:
        got = TSM.run(rv, rf, iterations=1, method="laplacian", boundary=boundary)
        TSM.same(got, E.smooth_step(rv, table, 0.5, boundary), f"one step, {boundary}")
    got = TSM.run(rv, rf, iterations=1)  # one Taubin iteration: two steps
    TSM.same(got, E.smooth_step(E.smooth_step(rv, table, 0.5, "fixed"), table, -0.53, "fixed"), "lam then mu")


@functools.lru_cache(maxsize=None)
def ray_case(case):
    verts, faces = device_tail(case)[1]
    o, d = RAY.random_rays(N_QUERIES, seed=len(case))
    refs = [RAY.cast(o, d, verts, faces, t_min, t_max, dt) for t_min, t_max in ((0.0, math.inf), (0.25, 1.5)) for dt in (np.float32, np.float64)]
    for a in (o, d) + tuple(x for r in refs for x in r):
        a.setflags(write=False)
    return (verts, faces, o, d) + tuple(refs)


@pytest.mark.parametrize("path", TRY.PATHS)
@pytest.mark.parametrize("case", CASES)
def test_rays_on_the_repaired_mesh(case, path):
    verts, faces, o, d, ref32, ref64, bound32, bound64 = ray_case(case)
    M = pkg("mesh_ray")
    v, f, od, dd = dev(verts), dev(faces), dev(o), dev(d)
    acc = TRY.accel_of(path, v, f)
    if path == "accel":
        assert acc.accel.numel() == L().dgm_ray_accel_bytes(len(faces)) and len(faces) % 256 != 0  # ragged against the chunk
    for t_min, t_max, r32, r64 in ((0.0, math.inf, ref32, ref64), (0.25, 1.5, bound32, bound64)):
        what = f"{case} / {path} in [{t_min}, {t_max})"
        got = TRY.cast(od, dd, v, f, acc, t_min, t_max)
        TRY.same_bits(got, r32, what)
        TRY.same_bits(TRY.cast(od, dd, v, f, acc, t_min, t_max), got, what + ": a second run")
        assert np.array_equal(M.occluded(od, dd, v, f, t_min, t_max, acc).cpu().numpy(), got[0] >= 0)
        TRY.check_against_fp64(what, verts, faces, o, d, got, r32, r64, t_min, t_max)
    hit = ref64[0] >= 0
    assert 0.1 < hit.mean() < 1.0 and 0 < (bound64[0] >= 0).sum() < hit.sum()  # hits and misses; the interval cuts


@pytest.mark.parametrize("case", CASES)
def test_winding_number_and_signed_distance_on_the_repaired_mesh(case):
    MI = pkg("mesh_inside")
    verts, faces = device_tail(case)[1]
    queries = IR.box_queries(verts, N_QUERIES, seed=len(case))
    w64, w32 = IR.winding(queries, verts, faces, np.float64), IR.winding(queries, verts, faces, np.float32)
    p, v, f = dev(queries), dev(verts), dev(faces)
    w = MI.winding_number(p, v, f)
    got = host(w)
    ref_err = float(np.abs(w32.astype(np.float64) - w64).max())
    tol = TIN.TOL_FACTOR * ref_err
    err = float(np.abs(got.astype(np.float64) - w64).max())
    near = np.abs(w64 - 0.5) < TIN.MARGIN
    print(f"{case} winding: F {len(faces)} N {len(queries)}: device max |w - w64| {err:.3e}; numpy fp32 statement {ref_err:.3e}, tolerance {tol:.3e}; "
          f"w64 in [{w64.min():.2f}, {w64.max():.2f}]; {near.mean():.1%} of the queries within {TIN.MARGIN} of the threshold")
    assert np.isfinite(got).all() and tol > 0 and err <= tol
    assert near.mean() <= 0.02
    inside = host(MI.contains(p, v, f))
    assert (inside[~near] == (w64 >= 0.5)[~near]).all() and (inside == (got >= 0.5)).all() and 0 < inside.sum() < len(inside)
    bits = lambda a, b: bool((a.view(torch.int32) == b.view(torch.int32)).all())
    assert bits(MI.winding_number(p, v, f), w) and bits(MI.winding_number(p[:65].contiguous(), v, f), w[:65])
    sd = MI.signed_distance(p, v, f)
    assert bits(MI.signed_distance(p, v, f), sd) and bool(torch.isfinite(sd).all())
    assert (host(sd.abs()).view(np.uint32) == np.sqrt(SR.closest32(queries, verts, faces)[1]).view(np.uint32)).all()
    assert (host(sd < 0) == inside).all()


@pytest.mark.parametrize("case", CASES)
def test_closest_point_on_the_repaired_mesh(case):
    verts, faces = device_tail(case)[1]
    queries = IR.box_queries(verts, N_QUERIES, seed=len(case) + 1)
    ref = SR.closest32(queries, verts, faces)
    edge = TSK.mean_edge(verts, faces)
    for scale in (math.inf, 2.0, 0.5):  # the brute force; the hash grid with a bound that cuts
        max_dist = scale * edge
        want = TSK.blank(ref, max_dist)
        got = TSK.run(queries, verts, faces, max_dist)
        TSK.same(got, want, f"{case}: max_dist {scale} mean edges")
        TSK.same(TSK.run(queries, verts, faces, max_dist), got, f"{case}: max_dist {scale} mean edges, a second run")
        if scale == 0.5:
            assert 0 < (want[0] >= 0).sum() < len(queries)
    face, d2, _ = TSK.run(queries, verts, faces)
    _, d64, _ = SR.closest64(queries, verts, faces)
    unit = SR.error_unit(verts, queries, np.sqrt(d64))
    D64 = SR.pair_d2(queries, verts, faces, np.float64)
    r_min = np.abs(d2.astype(np.float64) - d64) / unit
    r_chosen = (D64[np.arange(len(queries)), face] - d64) / unit
    print(f"{case} closest point: min d2 ratio {r_min.max():.3f} (bound {SR.K_MIN}), chosen-face excess {r_chosen.max():.3f} (bound {SR.K_CHOSEN}); "
          f"distances up to {np.sqrt(d64.max()):.2e}")
    assert (face >= 0).all() and r_min.max() <= SR.K_MIN and r_chosen.max() <= SR.K_CHOSEN


@pytest.mark.parametrize("case", CASES)
def test_atlas_on_the_repaired_mesh(case):
    MT = pkg("mesh_texture")
    verts, faces = device_tail(case)[1]
    F = len(faces)
    attr = np.concatenate([verts, np.random.default_rng(F).standard_normal((len(verts), 2)).astype(np.float32)], 1)  # positions and two more
    by_cell = MT.build_atlas(F, cell=6)
    assert by_cell.size == 6 * TX.per_row(F)
    _, ids, _ = TAT.check(by_cell, attr, faces, f"{case} cell 6")
    assert set(np.unique(ids)) - {-1} == set(range(F))  # every face owns texels
    ragged = MT.build_atlas(F, size=by_cell.size + 5)  # the same cell, a margin of 5 texels
    assert ragged.cell == 6 and ragged.size % ragged.cell == 5
    _, ids, _ = TAT.check(ragged, attr, faces, f"{case} size {ragged.size}")
    assert (ids[by_cell.size:] == -1).all() and (ids[:, by_cell.size:] == -1).all()


@pytest.mark.parametrize("case", CASES)
def test_ambient_occlusion_bake_on_the_repaired_mesh(case):
    """bake_ambient_occlusion is ambient_occlusion at the owned texels (the texel's rank is the point's index); the first AO_POINTS of
    them keep their index when they are cast alone, so test_mesh_ray.ao_case holds exactly the bake's rays to the fp64 count; a
    strided choice over the whole atlas is held to it as points of their own."""
    MT, M = pkg("mesh_texture"), pkg("mesh_ray")
    verts, faces = device_tail(case)[1]
    v, f = dev(verts), dev(faces)
    ao, uv, atlas = MT.bake_ambient_occlusion(v, f, cell=6, samples=AO_SAMPLES)
    assert ao.shape == (atlas.size, atlas.size, 1) and atlas == MT.build_atlas(len(faces), cell=6)
    assert torch.equal(MT.bake_ambient_occlusion(v, f, cell=6, samples=AO_SAMPLES)[0], ao)
    assert torch.equal(MT.bake_ambient_occlusion(v, f, cell=6, samples=AO_SAMPLES, accel=None)[0], ao)
    assert TAT.same_bits(uv, TX.atlas_uv(len(faces), atlas.size, atlas.cell, np.float32))
    pos, face_id = MT.atlas_interpolate(atlas, v, f)
    owned = (face_id.reshape(-1) >= 0).nonzero().reshape(-1)
    corner = v[f[face_id.reshape(-1)[owned].long()].long()]
    normal = torch.linalg.cross(corner[:, 1] - corner[:, 0], corner[:, 2] - corner[:, 0])
    points = pos.reshape(-1, 3)[owned].contiguous()
    flat = normal.abs().sum(1) == 0
    direct = M.ambient_occlusion(points, normal, v, f, AO_SAMPLES)
    assert torch.equal(ao.reshape(-1)[owned], direct) and (ao.reshape(-1)[face_id.reshape(-1) < 0] == 1).all()
    assert 0 <= float(ao.min()) < 0.9 and float(ao.max()) == 1  # the blobs and the sheet shadow each other
    usable = (~flat).nonzero().reshape(-1)
    print(f"{case} ambient occlusion: atlas {atlas.size}, {len(owned)} owned texels, {int(flat.sum())} on faces without area")
    assert len(owned) > 2 * AO_POINTS and not bool(flat[:AO_POINTS].any())  # no face without area among the first: they keep their indices
    got = TRY.ao_case(host(points[:AO_POINTS]), host(normal[:AO_POINTS]), verts, faces, AO_SAMPLES)
    assert np.array_equal(got.astype(np.float32), host(direct[:AO_POINTS]))
    spread = usable[::max(1, len(usable) // AO_POINTS)][:AO_POINTS]
    TRY.ao_case(host(points[spread]), host(normal[spread]), verts, faces, AO_SAMPLES, seed=3)


# ---- attributes through the whole chain ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_attributes_through_the_whole_chain(case):
    """The four apply functions in production order with a colour per vertex: the references' index maps, evaluated on the device's
    mesh of the stage before, say where every final colour comes from; an added rim vertex has the fp32 mean of its rim."""
    mv, mf = device_head()[1]
    colour = np.random.default_rng(17).random((len(mv), 3)).astype(np.float32)
    mesh = (dev(mv), dev(mf), dev(colour))
    mesh = pkg("mesh_clean").apply(C.CLEAN, *mesh)
    rv, rf, rvi, _ = RC.clean(mv, mf, **C.CLEAN)
    expect = colour[rvi]
    same(host(mesh[0]), rv, "cleaned vertices")
    same(host(mesh[1]), rf, "cleaned faces")
    same(host(mesh[2]), expect, "colours after clean")
    before = mesh
    mesh = pkg("mesh_smooth").apply(C.SMOOTH, *mesh)
    assert mesh[1] is before[1] and mesh[2] is before[2]
    same(host(mesh[0]), E.smooth(rv, rf, **C.SMOOTH), "smoothed vertices")
    sv, sf = host(mesh[0]), host(mesh[1])
    mesh = pkg("mesh_simplify").apply(C.CASES[case], *mesh)
    ref = RS.simplify(sv, sf, **C.CASES[case])
    expect = expect[ref["vert_index"]]
    same(host(mesh[1]), ref["faces"], "simplified faces")
    same(host(mesh[2]), expect, "colours after simplify: the representative's")
    gv, gf = host(mesh[0]), host(mesh[1])
    assert np.abs(gv.astype(np.float64) - ref["verts"]).max() <= TSI.tolerance(sv, sf)[0]
    mesh = pkg("mesh_repair").apply({}, *mesh)
    rv, rf, info = RR.repair(gv, gf)
    same(host(mesh[0]), rv, "repaired vertices")
    same(host(mesh[1]), rf, "repaired faces")
    got = host(mesh[2])
    assert got.shape == (len(rv), 3) and info["verts_added"] >= 1
    same(got[:len(gv)], expect, "colours after repair: the given rows")
    for k in range(len(gv), len(rv)):
        rim = rf[rf[:, 2] == k, 1]
        assert len(rim) >= 4
        np.testing.assert_allclose(got[k], expect[rim].mean(0), rtol=0, atol=1e-6)  # a mean of numbers in [0, 1], fp32
    again = pkg("mesh_repair").apply({}, *pkg("mesh_simplify").apply(C.CASES[case], *pkg("mesh_smooth").apply(C.SMOOTH, *before)))
    same(host(again[0]), host(mesh[0]), "vertices: run 1 against run 0")
    same(host(again[1]), host(mesh[1]), "faces: run 1 against run 0")
    same(host(again[2])[:len(gv)], expect, "colours: run 1 against run 0")


# ---- one export with every option on ------------------------------------------------------------------------------------------------------
def test_export_dynamic_mesh_with_every_option(scene, tmp_path):  # noqa: F811
    """clean, smooth, simplify, repair and texture (with ambient occlusion) at once: the PLY is byte-identical to the four apply calls
    made by hand, in the documented order, on the mesh the plain export wrote, and the textured file holds the same mesh.  (DPSR's
    splat sums with float atomics: the field of the first export is replayed into the others.)"""
    V, EV, io, O = pkg("visualize"), pkg("evaluate"), pkg("ply_io"), pkg("obj_io")
    g, m = scene["g"], scene["mesh"]
    args = (g, scene["deform"], scene["deform_back"], m)
    smooth, simplify, repair = {"iterations": 3}, {"grid": 12}, {}
    fields, orig = _record_psr(m)
    try:
        (plain,) = V.export_dynamic_mesh(*args, str(tmp_path / "plain"), frames=1)
        m.psr = lambda *a, **k: fields[0]
        (full,) = V.export_dynamic_mesh(*args, str(tmp_path / "full"), frames=1, clean=C.CLEAN, smooth=smooth, simplify=simplify, repair=repair,
                                        texture={"cell": 6, "ao_samples": 4})
        (again,) = V.export_dynamic_mesh(*args, str(tmp_path / "again"), frames=1, clean=C.CLEAN, smooth=smooth, simplify=simplify, repair=repair,
                                         texture={"cell": 6, "ao_samples": 4})
        fid = torch.zeros(1, device=g.get_xyz.device)
        with torch.no_grad():
            _, d_xyz, d_normal = V._deformations(g, scene["deform"], m.deform_normal, fid)
            mesh = EV.mesh_and_colors(m, g, scene["deform_back"], d_xyz, d_normal, fid)
    finally:
        m.psr = orig
    io.write_mesh_ply(str(tmp_path / "replayed.ply"), *mesh[:2], vertex_colors=mesh[2])
    assert open(plain, "rb").read() == open(tmp_path / "replayed.ply", "rb").read()  # the mesh the plain export wrote
    sizes = [tuple(int(t.shape[0]) for t in mesh[:2])]
    for module, spec in (("mesh_clean", C.CLEAN), ("mesh_smooth", smooth), ("mesh_simplify", simplify), ("mesh_repair", repair)):
        mesh = pkg(module).apply(spec, *mesh)
        sizes.append(tuple(int(t.shape[0]) for t in mesh[:2]))
    io.write_mesh_ply(str(tmp_path / "by_hand.ply"), *mesh[:2], vertex_colors=mesh[2])
    written = open(full, "rb").read()
    assert written == open(tmp_path / "by_hand.ply", "rb").read() and written != open(plain, "rb").read()
    assert written == open(again, "rb").read()
    v1, f1, c1 = io.read_mesh_ply(full, return_colors=True)
    rep =E.edge_table(f1, len(v1))["info"]
    print(f"export: (V, F) plain, clean, smooth, simplify, repair {sizes}; written mesh: {rep}")
    assert sizes[1][1] <= sizes[0][1] and sizes[2] == sizes[1] and sizes[3][1] < sizes[2][1] and sizes[4][1] >= sizes[3][1]
    assert c1.shape == (len(v1), 4) and len(f1) == sizes[4][1] and len(v1) == sizes[4][0]
    folder = tmp_path / "full" / "dynamic_mesh_textured"
    assert sorted(os.listdir(folder)) == ["frame_0.mtl", "frame_0.obj", "frame_0.png"]
    v2, f2, uv, tex = O.read_mesh_obj(str(folder / "frame_0.obj"))
    size = 6 * TX.per_row(len(f1))
    assert np.array_equal(v2, v1) and np.array_equal(f2, f1) and uv.shape == (len(f1), 3, 2) and tex.shape == (size, size, 3) and tex.max() > 1
    assert {n: open(folder / n, "rb").read() for n in os.listdir(folder)} == \
        {n: open(tmp_path / "again" / "dynamic_mesh_textured" / n, "rb").read() for n in os.listdir(folder)}


# ---- mesh_post.apply is the four calls, and the other three exports make it ---------------------------------------------------------------
def by_hand(mesh, clean=None, smooth=None, simplify=None, repair=None):
    """The four apply calls in the documented order, spelt out."""
    mesh = pkg("mesh_clean").apply(clean, *mesh)
    mesh = pkg("mesh_smooth").apply(smooth, *mesh)
    mesh = pkg("mesh_simplify").apply(simplify, *mesh)
    return pkg("mesh_repair").apply(repair, *mesh)


@pytest.mark.parametrize("which", ["all", "clean", "smooth", "simplify", "repair", "none"])
def test_mesh_post_is_the_four_calls_by_hand(which):
    """mesh_post.apply on the marching-cubes mesh with a colour per vertex: vertices, faces and colours byte for byte those of the
    four calls, with every stage on (simplify at grid16), with each stage alone and with none."""
    mv, mf = device_head()[1]
    assert (len(mv), len(mf)) == (2196, 4330)
    colour = np.random.default_rng(17).random((len(mv), 3)).astype(np.float32)
    specs = {"clean": C.CLEAN, "smooth": C.SMOOTH, "simplify": C.CASES["grid16"], "repair": {}}
    on = specs if which == "all" else {k: v for k, v in specs.items() if k == which}
    mesh = (dev(mv), dev(mf), dev(colour))
    got = pkg("mesh_post").apply(*mesh, **on)
    want = by_hand(mesh, **on)
    assert len(got) == len(want) == 3
    for g, w, name in zip(got, want, ("vertices", "faces", "colours")):
        same(host(g), host(w), f"{which}: {name}")
    print(f"{which}: V {len(mv)} F {len(mf)} -> V {got[0].shape[0]} F {got[1].shape[0]}")
    if which == "none":
        assert all(g is m for g, m in zip(got, mesh))
    else:
        assert any(g.shape != m.shape or not torch.equal(g, m) for g, m in zip(got, mesh))  # the stage did something


EXPORT_SPECS = dict(clean=C.CLEAN, smooth={"iterations": 3}, simplify={"grid": 12}, repair={})


def replay(mesh, fields):
    """mesh.psr hands out the recorded fields again, in call order (DPSR's splat sums with float atomics)."""
    left = iter(fields)
    mesh.psr = lambda *a, **k: next(left)


def test_extract_mesh_with_every_option(scene):  # noqa: F811
    g, m = scene["g"], scene["mesh"]
    fields, orig = _record_psr(m)
    try:
        plain = m.extract_mesh(g, scene["deform"], m.deform_normal, t=0.0)
        replay(m, fields)
        full = m.extract_mesh(g, scene["deform"], m.deform_normal, t=0.0, **EXPORT_SPECS)
    finally:
        m.psr = orig
    want = by_hand(plain, **EXPORT_SPECS)
    assert len(full) == 2 and full[1].shape[0] < plain[1].shape[0]
    same(host(full[0]), host(want[0]), "vertices")
    same(host(full[1]), host(want[1]), "faces")


def test_testing_writes_the_mesh_with_every_option(scene, tmp_path):  # noqa: F811
    EV, io, SC = pkg("evaluate"), pkg("ply_io"), pkg("scene")
    g, m, cam = scene["g"], scene["mesh"], scene["cameras"][0]
    kw = dict(pipe=SC.PipelineParams(), background=torch.ones(3, device=DEV), mesh=m, save_meshes=True)
    fields, orig = _record_psr(m)
    try:
        EV.testing(g, scene["deform"], scene["deform_back"], [cam], out_dir=str(tmp_path / "plain"), **kw)
        replay(m, fields)
        EV.testing(g, scene["deform"], scene["deform_back"], [cam], out_dir=str(tmp_path / "full"), **EXPORT_SPECS, **kw)
        replay(m, fields)
        with torch.no_grad():
            mesh = EV.mesh_and_colors(m, g, scene["deform_back"], None, None, cam.fid)
    finally:
        m.psr = orig
    written = lambda name: open(tmp_path / name / "test_results" / "dynamic_mesh" / "frame_0.ply", "rb").read()
    io.write_mesh_ply(str(tmp_path / "replayed.ply"), *mesh[:2], vertex_colors=mesh[2])
    assert written("plain") == open(tmp_path / "replayed.ply", "rb").read()  # the mesh the plain run wrote
    mesh = by_hand(mesh, **EXPORT_SPECS)
    io.write_mesh_ply(str(tmp_path / "by_hand.ply"), *mesh[:2], vertex_colors=mesh[2])
    assert written("full") == open(tmp_path / "by_hand.ply", "rb").read() and written("full") != written("plain")


def test_export_correspondence_with_every_option(scene, tmp_path):  # noqa: F811
    """mode "canonical": a frame's colours are the palette of its own vertices' canonical positions, which the test forms itself."""
    CO, io = pkg("correspondence"), pkg("ply_io")
    g, m = scene["g"], scene["mesh"]
    args = (g, scene["deform"], scene["deform_back"], m)
    fields, orig = _record_psr(m)
    try:
        plain = CO.export_correspondence(*args, str(tmp_path / "plain"), frames=1, mode="canonical", n_tracks=64)["paths"][0]
        assert len(fields) == 2  # mesh(t_ref), then the frame's
        replay(m, fields)
        full = CO.export_correspondence(*args, str(tmp_path / "full"), frames=1, mode="canonical", n_tracks=64, **EXPORT_SPECS)["paths"][0]
    finally:
        m.psr = orig
    fid = torch.zeros(1, device=DEV)
    with torch.no_grad():
        verts, faces = (t.contiguous() for t in m.surface(g, fields[1]))
        colour = CO.palette(CO.to_canonical(verts, fid, scene["deform_back"]), g.gaussian_center, g.gaussian_scale, "checker", 8)
    io.write_mesh_ply(str(tmp_path / "replayed.ply"), verts, faces, vertex_colors=colour)
    assert open(plain, "rb").read() == open(tmp_path / "replayed.ply", "rb").read()  # the mesh the plain export wrote
    mesh = by_hand((verts, faces, colour), **EXPORT_SPECS)
    io.write_mesh_ply(str(tmp_path / "by_hand.ply"), *mesh[:2], vertex_colors=mesh[2])
    written = open(full, "rb").read()
    assert written == open(tmp_path / "by_hand.ply", "rb").read() and written != open(plain, "rb").read()


# ---- the chain between guard zones --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_chain_between_guard_zones(case):
    """test_redzone.run_case on the whole chain: every stage's output is handed out at its exact size between guards (0xFF and 0x00
    bodies) and is the next stage's input; every guard holds afterwards, the outputs equal the plain run's byte for byte, and every
    scratch buffer is seen at exactly its size function's value for these ragged sizes."""
    MC, CL, SM, SI, RP = (pkg(n) for n in ("marching_cubes", "mesh_clean", "mesh_smooth", "mesh_simplify", "mesh_repair"))
    MR, MI, CO, MT, TP = (pkg(n) for n in ("mesh_ray", "mesh_inside", "correspondence", "mesh_texture", "mesh_topology"))
    field, mc, clean, smooth = device_head()
    simplified, repaired, info = device_tail(case)
    n, c = C.N, (C.N - 1) / 2.0
    o, d = RAY.random_rays(257, seed=2)
    queries = IR.box_queries(repaired[0], 257, seed=3)
    assert MI.batch_rows(len(repaired[1])) >= len(queries)  # one launch: the scratch is the size function's at (N, F)
    max_dist = 2.0 * TSK.mean_edge(*repaired)

    def call(i):
        v, f = MC.marching_cubes(i["field"], None, 0.0, False)
        v = ((v.double() - c) / (n / 2.0)).float()  # (to_unit_box: fp64, rounded once)
        cv, cf, cvi, cfi = CL.clean_mesh(v, f, return_index=True, **C.CLEAN)
        sv = SM.smooth_mesh(cv, cf, **C.SMOOTH)
        gv, gf, gvi, gfi, gvm = SI.simplify_mesh(sv, cf, return_index=True, **C.CASES[case])
        rv, rf, _ = RP.repair_mesh(gv, gf)
        table = TP.EdgeTable("mesh_edges", rf, int(rv.shape[0]))
        t = table.emit(edges=True, faces=True, adjacency=True, kind=True)
        mesh = MR.RayMesh(rv, rf)
        rays = list(MR.ray_cast(i["o"], i["d"], rv, rf, 0.0, math.inf, mesh)) + [MR.occluded(i["o"], i["d"], rv, rf, 0.25, 1.5, mesh)]
        near, far = CO.closest_on_mesh(i["q"], rv, rf, max_dist=max_dist), CO.closest_on_mesh(i["q"], rv, rf)
        atlas = MT.build_atlas(int(rf.shape[0]), cell=6)
        return [v, f, cv, cf, cvi, cfi, sv, gv, gf, gvi, gfi, gvm, rv, rf, t["edges"], t["edge_faces"], t["edge_count"], t["adj"], t["adj_kind"],
                table.adj_offset, table.vert_flag, mesh.accel] + rays + [MI.winding_number(i["q"], rv, rf), SM.smooth_mesh(rv, rf, iterations=1)] \
            + list(near) + list(far) + list(MT.atlas_interpolate(atlas, rv, rf))

    sized = lambda name, *a: (name, getattr(L(), name)(*a))
    (mV, mF), (cV, cF), (gV, gF), (rV, rF) = ((len(m[0]), len(m[1])) for m in (mc, clean, simplified, repaired))
    sizes = [sized("dgm_mc_scratch_bytes", n, n, n),
             sized("dgm_mesh_cc_scratch_bytes", mV, mF), sized("dgm_mesh_cc_select_scratch_bytes"), sized("dgm_mesh_compact_scratch_bytes", mV, mF),
             sized("dgm_mesh_edges_scratch_bytes", cV, cF),
             sized("dgm_mesh_simplify_scratch_bytes", cV, cF), sized("dgm_mesh_compact_scratch_bytes", cV, cF),
             sized("dgm_mesh_edges_scratch_bytes", gV, gF), sized("dgm_mesh_orient_scratch_bytes", gV, gF),
             sized("dgm_mesh_fill_scratch_bytes", gV, info["boundary_edges"]),
             sized("dgm_mesh_edges_scratch_bytes", rV, rF), sized("dgm_ray_accel_bytes", rF), sized("dgm_ray_build_scratch_bytes", rF),
             sized("dgm_wind_scratch_bytes", len(queries), rF), sized("dgm_surf_closest_scratch_bytes", len(queries), rF)]
    print(f"{case}: scratch sizes {sizes}")
    run_case(call, {"field": dev(field), "o": dev(o), "d": dev(d), "q": dev(queries)}, sizes)
