"""GPU tests of mesh simplification (dg-mesh_amd/mesh_simplify.py, csrc/mesh_simplify.hip) against the numpy reference
tests/_simplify_ref.py.  faces', vert_index, face_index, vert_map and the counts are compared byte for byte; verts' within 2 fp32 ulp
of the box's largest absolute coordinate (both sides are fp64 until the last rounding; the system's condition number is at most
3 / regularization, so the solvers differ by about 1e-12 relative: what remains is the last rounding, plus one ulp where the fp64
values straddle a rounding boundary).  Every case runs twice and the two runs are compared byte for byte, verts' included."""
import os
import sys

import numpy as np
import pytest
import torch

import _meshclean_ref as RC
import _simplify_ref as R
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

WORST = {"ulp": 0.0}


def M():
    return pkg("mesh_simplify")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
    assert a.tobytes() == b.tobytes(), f"{what}: {int((a.view(np.uint8) != b.view(np.uint8)).sum())} bytes differ"


def tolerance(verts, faces):
    """2 fp32 ulp of the largest absolute coordinate of the box (of the vertices the valid faces use)."""
    bx = R.box(verts, faces)
    top = np.float32(0.0) if bx is None else np.float32(max(np.abs(bx[0]).max(), np.abs(bx[1]).max()))
    return 2.0 * float(np.spacing(top)), float(np.spacing(top))


def check(verts, faces, **kw):
    """simplify_mesh against the reference, twice; -> the reference's result and the device's (numpy)."""
    verts, faces = np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    ref = R.simplify(verts, faces, **kw)
    tol, ulp = tolerance(verts, faces)
    dv, df = dev(verts), dev(faces)
    first = None
    for run in range(2):
        out = M().simplify_mesh(dv, df, return_index=True, return_info=True, **kw)
        got = dict(zip(("verts", "faces", "vert_index", "face_index", "vert_map"), (host(t) for t in out[:5])))
        info = out[5]
        assert got["verts"].shape[1:] == (3,) and got["faces"].shape[1:] == (3,)
        assert (len(got["verts"]), len(got["faces"])) == (len(ref["verts"]), len(ref["faces"])), f"counts (run {run})"
        for k in ("faces", "vert_index", "face_index", "vert_map"):
            same(got[k], ref[k], f"{k} (run {run})")
        assert got["verts"].dtype == np.float32
        if len(ref["verts"]):
            err = float(np.abs(got["verts"].astype(np.float64) - ref["verts"].astype(np.float64)).max())
            print(f"verts' max |device - reference| = {err:.3e} = {err / ulp:.2f} ulp of the box's largest coordinate (bound 2)")
            WORST["ulp"] = max(WORST["ulp"], err / ulp)
            assert err <= tol, f"verts' differ by {err / ulp:.2f} ulp (run {run})"
        if ref["cell"] is not None:
            assert info["cell"] == ref["cell"]
        if first is None:
            first = got
        else:
            for k in got:
                same(got[k], first[k], f"{k}: run 1 against run 0")
    print(f"worst so far: {WORST['ulp']:.2f} ulp")
    return ref, first, info


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
def soup(V, F, seed):
    """V random points in the unit cube and F random index triples (not always different): many small clusters, duplicates, nulls."""
    rng = np.random.RandomState(seed)
    return rng.rand(V, 3).astype(np.float32), rng.randint(0, max(V, 1), (F, 3)).astype(np.int32)


def patch(nx, ny, seed=0, amp=0.05):
    """A height field over [0, 1]^2 cut into nx x ny squares of two triangles."""
    rng = np.random.RandomState(seed)
    x, y = np.meshgrid(np.arange(nx + 1) / nx, np.arange(ny + 1) / ny, indexing="ij")
    z = 0.2 * np.sin(3 * x) * np.cos(2 * y) + amp * rng.rand(*x.shape)
    verts = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    a = (i * (ny + 1) + j).reshape(-1)
    faces = np.concatenate([np.stack([a, a + ny + 1, a + ny + 2], 1), np.stack([a, a + ny + 2, a + 1], 1)], 1).reshape(-1, 3)
    return verts, faces.astype(np.int32)


def strip(n_faces):
    V = n_faces + 2
    i = np.arange(n_faces)
    verts = np.stack([np.arange(V, dtype=np.float32) * 0.25, (np.arange(V) % 2).astype(np.float32),
                      (0.1 * np.sin(np.arange(V) * 0.05)).astype(np.float32)], 1)
    return verts, np.stack([i, i + 1, i + 2], 1).astype(np.int32)


def shuffled(verts, faces, seed):
    perm = np.random.RandomState(seed).permutation(len(verts))
    out = np.empty_like(verts)
    out[perm] = verts
    return out, perm[np.asarray(faces, np.int64)].astype(np.int32)


def tile():
    return pkg("mesh_clean").tile()


SIZES = {f"V{v}": (lambda v=v: soup(v, 2 * v + 1, v) + ({"grid": 3},)) for v in (0, 1, 63, 64, 65)}
SIZES.update({f"F{f}": (lambda f=f: soup(40, f, 100 + f) + ({"grid": 2},)) for f in (0, 1, 63, 64, 65)})
SIZES.update({f"F=T{o:+d}": (lambda o=o: (patch(46, 46)[0], patch(46, 46)[1][:tile() + o], {"grid": 12})) for o in (-1, 0, 1)})
SIZES["V=T+1 soup"] = lambda: soup(tile() + 1, 2 * tile() + 5, 7) + ({"grid": 9},)


@pytest.mark.parametrize("name", list(SIZES))
def test_sizes(name):
    assert tile() == 4096
    verts, faces, kw = SIZES[name]()
    check(verts, faces, **kw)


def test_empty_mesh():
    v, f, vi, fi, vm = M().simplify_mesh(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"), grid=4,
                                         return_index=True)
    assert v.shape == (0, 3) and f.shape == (0, 3) and vi.shape == (0,) and fi.shape == (0,) and vm.shape == (0,)
    assert v.dtype == torch.float32 and all(t.dtype == torch.int32 for t in (f, vi, fi, vm))


STRIPS = {
    "ascending": lambda: strip(4097),
    "descending": lambda: (strip(4097)[0][::-1].copy(), (4098 - strip(4097)[1]).astype(np.int32)),
    "permuted": lambda: shuffled(*strip(4097), seed=3),
}


@pytest.mark.parametrize("name", list(STRIPS))
def test_strips(name):
    verts, faces = STRIPS[name]()
    ref, _, _ = check(verts, faces, cell=0.75)  # the two rows fall into different cells, one or two vertices of a row into each
    assert 0 < len(ref["faces"]) < len(faces)
    check(verts, faces, grid=300)  # about fourteen consecutive vertices per cell: every face is null


@pytest.mark.parametrize("grid", [4, 8, 16])
def test_icosphere(grid):
    verts, faces = R.icosphere(4)
    assert len(faces) == 5120
    ref, got, info = check(verts, faces, grid=grid)
    assert 0 < len(ref["faces"]) < 5120 and info["grid"] == grid and max(info["dims"]) in (grid, grid + 1)
    check(*shuffled(verts, faces, seed=grid), grid=grid)


def test_subdivided_cube():
    verts, faces = R.subdivided_cube(4)
    ref, got, _ = check(verts, faces, grid=2)
    corners = (verts[ref["vert_index"]] >= 0.5).astype(np.float64)
    assert got["verts"].shape == (8, 3) and np.abs(got["verts"] - corners).max() < 2e-3  # (the members' mean is 0.107 away)
    check(verts, faces, grid=2, regularization=1e-13)
    verts, faces = R.subdivided_cube(8)
    check(verts, faces, grid=4)  # (the vertices at 1.0 lie exactly on the box maximum: index n - 1)
    check(verts, faces, cell=0.25)
    check(verts, faces, grid=3)


def test_plane_patch_stays_on_its_plane():
    """z = 0.5 x + 0.25 y + 0.125 over a lattice of multiples of 1 / 64: every input vertex is on the plane exactly."""
    nx = ny = 48
    x, y = np.meshgrid(np.arange(nx + 1) / 64.0, np.arange(ny + 1) / 64.0, indexing="ij")
    verts = np.stack([x, y, 0.5 * x + 0.25 * y + 0.125], -1).reshape(-1, 3).astype(np.float32)
    faces = patch(nx, ny)[1]
    assert np.array_equal(verts[:, 2].astype(np.float64), 0.5 * verts[:, 0].astype(np.float64) + 0.25 * verts[:, 1] + 0.125)
    tol, ulp = tolerance(verts, faces)
    for kw in ({"grid": 7}, {"grid": 16}, {"cell": 0.11}):
        ref, got, _ = check(verts, faces, **kw)
        v = got["verts"].astype(np.float64)
        off = np.abs(v[:, 2] - (0.5 * v[:, 0] + 0.25 * v[:, 1] + 0.125)).max()
        print(f"plane: max distance along z {off:.3e} = {off / ulp:.2f} ulp")
        assert len(v) > 0 and off <= tol


def test_long_list_all_in_one_cell():
    verts, faces = soup(2600, 5000, 11)
    ref, got, _ = check(verts, faces, cell=10.0)
    assert got["faces"].shape == (0, 3) and got["verts"].shape == (0, 3) and (got["vert_map"] == -1).all()
    assert ref["lists"].tolist() == [int(R.valid_faces(verts, faces).sum())] and ref["lists"][0] > 4900


def test_long_list_fan_around_one_vertex():
    n = 5000
    ang = 2 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], 1)
    hub = n // 2
    verts = np.insert(ring, hub, [0.0, 0.0, 0.5], axis=0).astype(np.float32)
    ids = np.delete(np.arange(n + 1), hub)
    faces = np.stack([np.full(n, hub), ids, np.roll(ids, -1)], 1).astype(np.int32)
    ref, got, _ = check(verts, faces, cell=0.4)
    assert ref["lists"].max() == n and (ref["lists"] == n).sum() == 1  # the hub's cell holds only it: one list of all 5 000 faces
    new_hub = ref["vert_map"][hub]
    assert new_hub >= 0 and ref["vert_index"][new_hub] == hub and (ref["vert_map"] == new_hub).sum() == 1
    assert np.abs(got["verts"][new_hub] - np.array([0.0, 0.0, 0.5])).max() < 1e-2  # the apex of the cone
    check(*shuffled(verts, faces, seed=2), cell=0.4)


def test_filters():
    verts, faces = R.icosphere(2)
    V = len(verts)
    verts = np.concatenate([verts, np.array([[np.nan, 0, 0], [0, np.inf, 0], [0.1, 0.2, 0.3]], np.float32)])
    bad = np.array([[0, 0, 1], [5, 5, 5], [3, 4, 3],  # degenerate
                    faces[0], faces[1][::-1], faces[2][[1, 2, 0]],  # duplicated, also with reversed winding
                    [0, 1, V], [2, V + 1, 3],  # a non-finite corner
                    [0, 1, V + 3], [-1, 2, 3], [2 ** 31 - 1, 0, 1], [0, -(2 ** 31), 1]], np.int32)  # out of range
    rng = np.random.RandomState(4)
    mixed = np.concatenate([faces, bad])[rng.permutation(len(faces) + len(bad))]
    for kw in ({"grid": 4}, {"grid": 40}):
        ref, got, _ = check(verts, mixed, **kw)
        assert got["vert_map"][V:].tolist() == [-1, -1, -1]
    # at a grid that merges nothing, exactly the 320 different faces survive
    assert len(ref["faces"]) == 320 and len(ref["verts"]) == V


def test_stray_unused_vertex_changes_nothing():
    verts, faces = R.icosphere(3)
    _, a, _ = check(verts, faces, grid=6)
    far = np.concatenate([verts, np.array([[1e6, -1e6, 1e6]], np.float32)])
    _, b, _ = check(far, faces, grid=6)
    for k in ("verts", "faces", "vert_index", "face_index"):
        same(a[k], b[k], k)
    same(b["vert_map"][:-1], a["vert_map"], "vert_map")
    assert b["vert_map"][-1] == -1


def test_cell_smaller_than_every_edge_merges_nothing():
    """The integer outputs equal mesh_clean.clean_mesh without criteria.  The positions are PLACED, not copied: an inner vertex is the
    common point of its faces' planes and stays where it is up to rounding, a vertex on the patch's border has too few planes and
    is drawn towards its faces' centroids; by the definition none moves by more than 1.5 h per axis (half a cell to the centre,
    then the clamp)."""
    verts, faces = patch(30, 30, seed=5)
    faces = np.concatenate([faces, np.array([[0, 0, 1], [0, 1, 2000]], np.int32)])  # an invalid and an out-of-range face
    h = np.float32(1e-3)
    ref, got, _ = check(verts, faces, cell=float(h))
    cv, cf, cvi, cfi = pkg("mesh_clean").compact(dev(verts), dev(faces), dev(RC.valid_faces(faces, len(verts)).astype(np.uint8)))
    same(got["faces"], host(cf), "faces against clean_mesh")
    same(got["vert_index"], host(cvi), "vert_index against clean_mesh")
    same(got["face_index"], host(cfi), "face_index against clean_mesh")
    moved = np.abs(got["verts"].astype(np.float64) - host(cv).astype(np.float64)).max()
    print(f"moved by at most {moved:.3e} (h = {float(h):g})")
    assert moved <= 1.5 * float(h) + tolerance(verts, faces)[0]
    v2, f2 = pkg("mesh_clean").clean_mesh(dev(verts), dev(faces[:-1]))
    same(got["faces"], host(f2), "faces against clean_mesh()")


def test_tiny_cell_welds_duplicated_positions():
    """A triangle soup (every face with its own three vertices) of an icosphere of diameter 1 at cell 1e-6: pymeshlab's
    meshing_merge_close_vertices case."""
    verts, faces = R.icosphere(2)
    verts = (verts * np.float32(0.5)).astype(np.float32)
    soup_v = verts[faces.reshape(-1)]
    soup_f = np.arange(3 * len(faces), dtype=np.int32).reshape(-1, 3)
    ref, got, info = check(soup_v, soup_f, cell=1e-6)
    assert got["verts"].shape == (len(verts), 3) and got["faces"].shape == (len(faces), 3) and max(info["dims"]) > 900000
    # the welded mesh is closed again
    f = got["faces"].astype(np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    assert (np.unique(e[:, 0] * len(verts) + e[:, 1], return_counts=True)[1] == 2).all()
    with pytest.raises(ValueError, match=r"2\^20"):
        M().simplify_mesh(dev(soup_v), dev(soup_f), cell=1e-7)


@pytest.mark.parametrize("target", [100, 1000, 5000])
def test_target_faces(target):
    verts, faces = R.icosphere(4)
    ref, got, info = check(verts, faces, target_faces=target)
    assert len(got["faces"]) <= target
    assert info["grid"] == ref["grid"] and info["grids_tried"] == ref["grids_tried"]
    assert info["count_passes"] == len(info["grids_tried"]) <= 10
    print(f"target {target}: grid {info['grid']} after {info['count_passes']} passes -> {len(got['faces'])} faces")


def test_target_faces_out_of_reach_raises():
    verts, faces = R.icosphere(2)
    with pytest.raises(ValueError, match="not reached"):
        M().simplify_mesh(dev(verts), dev(faces), target_faces=3)


def test_apply_gathers_attributes_at_the_representative():
    verts, faces = R.icosphere(3)
    ref = R.simplify(verts, faces, grid=5)
    colour = np.random.RandomState(0).rand(len(verts), 3).astype(np.float32)
    v, f, c, none = M().apply({"grid": 5}, dev(verts), dev(faces), dev(colour), None)
    same(host(f), ref["faces"], "faces")
    same(host(c), colour[ref["vert_index"]], "colours")
    assert none is None and v.shape == (len(ref["verts"]), 3)


def test_cli_round_trips_a_ply(tmp_path, capsys):
    io = pkg("ply_io")
    verts, faces = R.icosphere(3)
    colour = np.random.RandomState(1).rand(len(verts), 3).astype(np.float32)
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    io.write_mesh_ply(src, verts, faces, vertex_colors=colour)
    v0, f0, c0 = io.read_mesh_ply(src, return_colors=True)
    assert M().main([src, dst, "--grid", "6"]) == 0
    assert "grid 6" in capsys.readouterr().out
    v1, f1, c1 = io.read_mesh_ply(dst, return_colors=True)
    ref = R.simplify(v0, f0, grid=6)
    same(f1, ref["faces"], "faces")
    same(c1, c0[ref["vert_index"]], "colours")
    assert np.abs(v1.astype(np.float64) - ref["verts"]).max() <= tolerance(v0, f0)[0]
    # a file without colours stays without
    io.write_mesh_ply(src, verts, faces)
    assert M().main([src, dst, "--target_faces", "200"]) == 0
    v2, f2, c2 = io.read_mesh_ply(dst, return_colors=True)
    assert c2 is None and 0 < len(f2) <= 200


def test_export_dynamic_mesh_and_extract_mesh_simplify(tmp_path):
    """export_dynamic_mesh(simplify=None) writes what it wrote before; with simplify the written mesh is the reference's simplification
    of that file, colours taken at the representatives; extract_mesh applies `clean` first.  (DPSR's splat accumulates with float
    atomics: the field of the first export is replayed into the others.)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_trainer_dp_gpu import make_mesh_trainer
    T, V, io, EV = pkg("trainer"), pkg("visualize"), pkg("ply_io"), pkg("evaluate")
    base = make_mesh_trainer(0, 1, res=48, P=2000, W=64, H=64, n_frames=1)
    g = base.g
    mesh = T.MeshPhase(*base.mesh.networks(), dpsr=base.mesh.dpsr, n_verts=4000, scale=1.0, device=g.get_xyz.device,
                       mesh_source="diffmc", mesh_losses="render")
    mesh.bind(g)
    fields, orig = [], mesh.psr

    def record(*a, **k):
        fields.append(orig(*a, **k))
        return fields[-1]

    mesh.psr = record
    (plain,) = V.export_dynamic_mesh(g, base.deform, base.deform_back, mesh, str(tmp_path / "a"), frames=1, simplify=None)
    mesh.psr = lambda *a, **k: fields[0]
    (default,) = V.export_dynamic_mesh(g, base.deform, base.deform_back, mesh, str(tmp_path / "b"), frames=1)
    assert open(plain, "rb").read() == open(default, "rb").read()
    fid = torch.zeros(1, device=g.get_xyz.device)
    _, d_xyz, d_normal = V._deformations(g, base.deform, mesh.deform_normal, fid)
    verts, faces, colors = EV.mesh_and_colors(mesh, g, base.deform_back, d_xyz, d_normal, fid)
    io.write_mesh_ply(str(tmp_path / "c.ply"), verts, faces, vertex_colors=colors)
    assert open(plain, "rb").read() == open(tmp_path / "c.ply", "rb").read()  # the unsimplified path, byte for byte
    (small,) = V.export_dynamic_mesh(g, base.deform, base.deform_back, mesh, str(tmp_path / "d"), frames=1, simplify={"grid": 32})
    v0, f0, c0 = io.read_mesh_ply(plain, return_colors=True)
    v1, f1, c1 = io.read_mesh_ply(small, return_colors=True)
    ref = R.simplify(v0, f0, grid=32)
    assert 0 < len(f1) < len(f0)
    same(f1, ref["faces"], "exported faces")
    same(c1, c0[ref["vert_index"]], "exported colours")
    assert np.abs(v1.astype(np.float64) - ref["verts"]).max() <= tolerance(v0, f0)[0]
    # clean first, then simplify
    spec = M().SimplifySpec(grid=16)
    ev, ef = mesh.extract_mesh(g, base.deform, mesh.deform_normal, t=0.0, clean={"largest": True}, simplify=spec)
    cv, cf, _, _ = RC.clean(v0, f0, largest=True)
    both = R.simplify(cv, cf, grid=16)
    same(host(ef), both["faces"], "extract_mesh faces")
    assert np.abs(host(ev).astype(np.float64) - both["verts"]).max() <= tolerance(cv, cf)[0]
    only = mesh.extract_mesh(g, base.deform, mesh.deform_normal, t=0.0, simplify=spec)[1]
    same(host(only), R.simplify(v0, f0, grid=16)["faces"], "extract_mesh faces, simplify alone")
    print(f"exported mesh: V {len(v0)} F {len(f0)} -> V {len(v1)} F {len(f1)}")
