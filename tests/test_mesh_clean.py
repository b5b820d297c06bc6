"""GPU tests of mesh cleaning (dg-mesh_amd/mesh_clean.py, csrc/mesh_clean.hip) against the numpy reference tests/_meshclean_ref.py.
Everything is integers, comparisons and copies, so every comparison is equality of bytes: labels, all table columns, the keep
mask, verts', faces' and both index maps, and every case is run twice."""
import os
import sys

import numpy as np
import pytest
import torch

import _meshclean_ref as R
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

CRITERIA = ({}, {"largest": True}, {"min_faces": 3}, {"min_diameter_frac": 0.25}, {"largest": True, "min_faces": 2, "min_diameter_frac": 0.1},
            {"min_faces": 1 << 30})


def M():
    return pkg("mesh_clean")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
    assert a.tobytes() == b.tobytes(), f"{what}: {int((a.view(np.uint8) != b.view(np.uint8)).sum())} bytes differ"


def check_mesh(verts, faces, criteria=CRITERIA):
    """labels, table, and for every set of criteria the keep mask and the compaction, bit for bit against the reference; twice."""
    verts, faces = np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    V = len(verts)
    lab = R.labels(faces, V)
    tab = R.table(verts, faces, lab)
    refs = [(c, R.keep_mask(verts, faces, lab, **c)) for c in criteria]
    refs = [(c, k, R.compact(verts, faces, k)) for c, k in refs]
    dv, df = dev(verts), dev(faces)
    for run in range(2):
        got = M().connected_components(df, V)
        same(host(got), lab, f"labels (run {run})")
        t = M().component_table(dv, df, got)
        for k in ("label", "faces", "verts", "bbox_min", "bbox_max"):
            same(host(t[k]), tab[k], f"table[{k}] (run {run})")
        for c, keep, (rv, rf, rvi, rfi) in refs:
            same(host(M().keep_mask(dv, df, got, **c)), keep, f"keep {c} (run {run})")
            v, f, vi, fi = M().clean_mesh(dv, df, return_index=True, **c)
            assert v.shape[1:] == (3,) and f.shape[1:] == (3,)
            for name, a, b in (("verts'", v, rv), ("faces'", f, rf), ("vert_index", vi, rvi), ("face_index", fi, rfi)):
                same(host(a), b, f"{name} {c} (run {run})")
    return lab, tab


def soup(V, F, seed, group=9):
    """An index soup of several components: the vertices fall into runs of up to `group`, a face picks three (not always different)
    vertices of one run; then the vertex ids are shuffled.  Some coordinates are repeated and some are -0.0 / +0.0."""
    rng = np.random.RandomState(seed)
    cuts = np.unique(np.concatenate([[0], rng.randint(0, V, max(V // group, 1)), [V]]))  # sorted run boundaries, 0 and V among them
    run = rng.randint(0, len(cuts) - 1, F)
    start, size = cuts[run], cuts[run + 1] - cuts[run]
    faces = (start[:, None] + rng.randint(0, 1 << 30, (F, 3)) % size[:, None]).astype(np.int64)
    perm = rng.permutation(V)
    verts = rng.randn(V, 3).astype(np.float32)
    verts[rng.randint(0, V, V // 4 + 1)] = verts[rng.randint(0, V, V // 4 + 1)]
    verts[rng.randint(0, V, V // 8 + 1), rng.randint(0, 3, V // 8 + 1)] = rng.choice(np.array([0.0, -0.0], np.float32), V // 8 + 1)
    return verts, perm[faces].astype(np.int32).reshape(F, 3)


def shuffled(verts, faces, seed):
    perm = np.random.RandomState(seed).permutation(len(verts))
    out = np.empty_like(verts)
    out[perm] = verts
    return out, perm[np.asarray(faces, np.int64)].astype(np.int32)


def strip(n_faces):
    V = n_faces + 2
    i = np.arange(n_faces)
    verts = np.stack([np.arange(V, dtype=np.float32) * 0.5, (np.arange(V) % 2).astype(np.float32), np.zeros(V, np.float32)], 1)
    return verts, np.stack([i, i + 1, i + 2], 1).astype(np.int32)


def tetrahedra(n, spacing=3.0):
    base = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    tf = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    verts = (base[None] + spacing * np.arange(n, dtype=np.float32)[:, None, None] * np.array([1, 0, 0], np.float32)).reshape(-1, 3)
    return verts, (tf[None] + 4 * np.arange(n, dtype=np.int32)[:, None, None]).reshape(-1, 3)


def tile():
    return M().tile()


# name -> builder, resolved when the case runs (the tile is the library's)
SIZE_CASES = {f"V{v}": (lambda v=v: soup(v, 2 * v + 1, v)) for v in (1, 2, 63, 64, 65, 255, 256, 257)}
SIZE_CASES.update({f"V=T{o:+d}": (lambda o=o: soup(tile() + o, tile() + o + 7, 11 + o)) for o in (-1, 0, 1)})
SIZE_CASES["V=2T+1"] = lambda: soup(2 * tile() + 1, 2 * tile() + 300, 5, group=2000)  # (a few components that span tiles)
SIZE_CASES.update({f"F{f}": (lambda f=f: soup(301, f, f)) for f in (1, 63, 64, 65, 255, 256, 257)})
SIZE_CASES.update({f"F=T{o:+d}": (lambda o=o: soup(3001, tile() + o, 21 + o)) for o in (-1, 0, 1)})
SIZE_CASES["F=2T+1"] = lambda: soup(4999, 2 * tile() + 1, 6)
SIZE_CASES["F=0"] = lambda: (soup(10, 1, 0)[0], np.zeros((0, 3), np.int32))
SIZE_CASES["no referenced vertex"] = lambda: (soup(100, 1, 1)[0], np.array([[5, 5, 7], [9, 9, 9], [1, 2, 1], [3, 4, 4], [0, 0, 0]], np.int32))


@pytest.mark.parametrize("name", list(SIZE_CASES))
def test_sizes(name):
    verts, faces = SIZE_CASES[name]()
    check_mesh(verts, faces)


def test_empty_mesh():
    v, f, vi, fi = M().clean_mesh(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"), largest=True,
                                  return_index=True)
    assert v.shape == (0, 3) and f.shape == (0, 3) and vi.shape == (0,) and fi.shape == (0,)
    assert M().connected_components(torch.zeros((0, 3), dtype=torch.int32, device="cuda"), 0).shape == (0,)
    v, f = M().clean_mesh(dev(np.zeros((5, 3), np.float32)), dev(np.array([[0, 1, 2], [2, 3, 4]], np.int32)), min_faces=3)
    assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == torch.float32 and f.dtype == torch.int32


STRESS = {
    "strip ascending": lambda: strip(4097),
    "strip descending": lambda: (strip(4097)[0][::-1].copy(), (4098 - strip(4097)[1]).astype(np.int32)),
    "strip permuted": lambda: shuffled(*strip(4097), seed=3),
    "star": lambda: shuffled(np.random.RandomState(0).randn(4001, 3).astype(np.float32),
                             np.stack([np.zeros(2000, np.int64), 1 + 2 * np.arange(2000), 2 + 2 * np.arange(2000)], 1), seed=4),
    "star hub first": lambda: (np.random.RandomState(0).randn(4001, 3).astype(np.float32),
                               np.stack([np.zeros(2000, np.int64), 1 + 2 * np.arange(2000), 2 + 2 * np.arange(2000)], 1).astype(np.int32)),
    "tetrahedra": lambda: shuffled(*tetrahedra(1000), seed=5),
    "tetrahedra in order": lambda: tetrahedra(1000),
}


@pytest.mark.parametrize("name", list(STRESS))
def test_shapes_that_stress_the_union_find(name):
    verts, faces = STRESS[name]()
    lab, tab = check_mesh(verts, faces, criteria=({}, {"largest": True}))
    expect = {"strip": 1, "star": 1, "tetrahedra": 1000}[name.split()[0]]
    assert len(tab["label"]) == expect and (expect > 1 or (lab == 0).all())


def test_two_closed_surfaces_touching_in_one_vertex_are_one_component():
    verts, faces = tetrahedra(2, spacing=1.0)  # vertex 1 of the first = (1, 0, 0) = vertex 0 of the second: merge the two indices
    faces = np.where(faces == 4, 1, faces)
    verts, faces = shuffled(verts, faces, seed=8)
    lab, tab = check_mesh(verts, faces)
    assert sorted(zip(tab["faces"].tolist(), tab["verts"].tolist())) == [(0, 1), (8, 7)]  # (the orphaned copy is a component of its own)


def test_degenerate_and_duplicated_faces():
    verts = np.random.RandomState(2).randn(12, 3).astype(np.float32)
    faces = np.array([[0, 1, 2], [0, 1, 2], [2, 1, 0], [3, 3, 4], [4, 3, 3], [5, 5, 5], [6, 7, 6], [8, 9, 10], [8, 9, 10], [10, 11, 11]],
                     np.int32)
    lab, tab = check_mesh(verts, faces)
    assert lab.tolist() == [0, 0, 0, 3, 4, 5, 6, 7, 8, 8, 8, 11] and tab["faces"][[0, 6]].tolist() == [3, 2]
    verts, faces = shuffled(verts, faces, seed=1)
    check_mesh(verts, faces)


def test_out_of_range_faces_raise_with_their_count():
    verts = dev(np.zeros((6, 3), np.float32))
    faces = dev(np.array([[0, 1, 2], [3, 4, 6], [-1, 2, 3], [3, 4, 5], [2 ** 31 - 1, 0, 1], [0, 0, -5]], np.int32))
    with pytest.raises(ValueError, match=r"4 of 6 faces have an index outside \[0, 6\)"):
        M().connected_components(faces, 6)
    with pytest.raises(ValueError, match="4 of 6 faces"):
        M().clean_mesh(verts, faces, largest=True)
    # the lower layers drop such faces without using their indices
    lab = dev(np.array([0, 0, 0, 3, 3, 3], np.int32))
    t = M().component_table(verts, faces, lab)
    assert host(t["faces"]).tolist() == [1, 1]
    v, f, vi, fi = M().compact(verts, faces, torch.ones(6, dtype=torch.uint8, device="cuda"))
    assert host(fi).tolist() == [0, 3] and host(vi).tolist() == [0, 1, 2, 3, 4, 5]
    with pytest.raises(RuntimeError, match="int32"):
        M().connected_components(faces.long(), 6)


def test_selection_tie_goes_to_the_smaller_label():
    verts, faces = tetrahedra(3)
    faces = faces[[8, 9, 10, 11, 4, 5, 6, 7, 0, 1, 2]]  # 3 faces of the first, 4 of each other, the largest label first in the list
    check_mesh(verts, faces)
    v, f, vi, fi = M().clean_mesh(dev(verts), dev(faces), largest=True, return_index=True)
    assert host(vi).tolist() == [4, 5, 6, 7] and host(fi).tolist() == [4, 5, 6, 7]
    v2, f2 = M().verts_on_largest_mesh(dev(verts), dev(faces))
    assert torch.equal(v, v2) and torch.equal(f, f2)


def test_min_faces_at_exactly_a_component_count_keeps_it():
    verts, faces = tetrahedra(3)
    faces = faces[[0, 1, 2, 4, 5, 8, 9, 10, 11]]  # 3, 2 and 4 faces
    check_mesh(verts, faces, criteria=({"min_faces": 2}, {"min_faces": 3}, {"min_faces": 4}, {"min_faces": 5}))
    assert host(M().keep_mask(dev(verts), dev(faces), min_faces=3)).tolist() == [1, 1, 1, 0, 0, 1, 1, 1, 1]


def test_min_diameter_one_ulp_around_the_threshold():
    """Components that span [0, dx] on x only, inside a whole-mesh box of (1, 0.7, 0.3): the reference's own fp32 expression finds the
    neighbouring dx whose squared diagonals lie on the two sides of (frac * frac) * whole, and the kernel must split them there."""
    f32 = np.float32
    frac = 0.3
    whole = R.diag2(np.zeros(3, f32), np.array([1.0, 0.7, 0.3], f32))
    thr = f32(f32(f32(frac) * f32(frac)) * whole)
    dx = f32(np.sqrt(np.float64(thr)))
    for _ in range(8):  # walk below the threshold, then up to the first dx at or above it
        dx = np.nextafter(dx, f32(0))
    below = dx
    while R.diag2(np.zeros(3, f32), np.array([np.nextafter(below, f32(2)), 0, 0], f32)) < thr:
        below = np.nextafter(below, f32(2))
    above = np.nextafter(below, f32(2))
    d_lo, d_hi = (R.diag2(np.zeros(3, f32), np.array([d, 0, 0], f32)) for d in (below, above))
    assert d_lo < thr <= d_hi and above - below == np.spacing(below)  # the reference separates neighbours
    tri = lambda d: np.array([[0, 0, 0], [d, 0, 0], [d / 2, 0, 0]], f32)
    verts = np.concatenate([np.array([[0, 0, 0], [1, 0.7, 0.3], [1, 0, 0]], f32), tri(below), tri(above), tri(f32(0.5)), tri(f32(0.01))])
    faces = np.arange(15, dtype=np.int32).reshape(5, 3)
    ref = R.keep_mask(verts, faces, R.labels(faces, 15), min_diameter_frac=frac)
    assert ref.tolist() == [1, 0, 1, 1, 0]
    check_mesh(verts, faces, criteria=({"min_diameter_frac": frac}, {"min_diameter_frac": frac, "largest": True},
                                       {"min_diameter_frac": 1.0}, {"min_diameter_frac": 1.0000001}))
    verts, faces = shuffled(verts, faces, seed=9)
    check_mesh(verts, faces, criteria=({"min_diameter_frac": frac},))
    assert sorted(host(M().clean_mesh(dev(verts), dev(faces), min_diameter_frac=frac, return_index=True)[3]).tolist()) == [0, 2, 3]


def test_diffmc_mesh_of_two_spheres_and_a_blob():
    MC = pkg("marching_cubes")
    g = np.stack(np.meshgrid(*(np.arange(32, dtype=np.float32),) * 3, indexing="ij"), -1)
    ball = lambda c, r: np.linalg.norm(g - np.array(c, np.float32), axis=-1) - r
    field = np.minimum(np.minimum(ball((10.2, 10.4, 10.1), 7.3), ball((22.3, 21.9, 22.2), 4.2)), ball((26.3, 6.2, 6.4), 1.1))
    verts, faces = MC.marching_cubes(dev(field.astype(np.float32)), isovalue=0.0, normalize=False)
    lab, tab = check_mesh(host(verts), host(faces))
    assert len(tab["label"]) == 3 and sorted(tab["faces"].tolist())[0] < 100 and int(tab["verts"].sum()) == len(lab)
    v, f, vi, fi = M().clean_mesh(verts, faces, largest=True, return_index=True)
    f = host(f).astype(np.int64)
    assert len(f) == tab["faces"].max() and len(v) == tab["verts"][np.argmax(tab["faces"])]
    assert np.array_equal(np.unique(f), np.arange(len(v)))  # every vertex is referenced
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    _, counts = np.unique(e[:, 0] * len(v) + e[:, 1], return_counts=True)
    assert (counts == 2).all()  # closed: every edge in exactly two faces
    assert torch.equal(v, verts[vi.long()])
    # the largest sphere's radius survives in the box
    ext = host(v).max(0) - host(v).min(0)
    assert np.all(np.abs(ext - 14.6) < 0.2)


def _write_obj(path, verts, faces):
    with open(path, "w") as fh:
        for x, y, z in verts.tolist():
            fh.write(f"v {float(x)!r} {float(y)!r} {float(z)!r}\n")
        for a, b, c in faces.tolist():
            fh.write(f"f {a + 1} {b + 1} {c + 1}\n")


def test_evaluation_cleans_the_predicted_mesh(tmp_path):
    """Two OBJ / PLY pairs: the prediction is the ground truth plus a far floater.  Without `clean` the Chamfer distance is far from
    that of the floater-free files; with largest=True both metrics equal theirs bit for bit."""
    E, io = pkg("mesh_eval"), pkg("ply_io")
    cube = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    cf = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                   [1, 5, 7], [1, 7, 3]], np.int32)
    tv, tf = tetrahedra(1)
    for d in ("gt", "with", "without"):
        os.makedirs(tmp_path / d)
    for i, scale in enumerate((1.0, 0.6)):
        v = cube * np.float32(scale) - np.float32(0.3)
        _write_obj(tmp_path / "gt" / f"mesh_{i}.obj", v, cf)
        io.write_mesh_ply(str(tmp_path / "without" / f"frame_{i}.ply"), v, cf)
        io.write_mesh_ply(str(tmp_path / "with" / f"frame_{i}.ply"), np.concatenate([v, tv * np.float32(0.05) + np.float32(40.0)]),
                          np.concatenate([cf, tf + 8]))
    run = lambda pred, **kw: E.evaluation(str(tmp_path / "gt"), str(tmp_path / pred), "dgmesh", emd_sample=256, seed=3, **kw)
    clean_run, floater_run = run("without"), run("with")
    assert floater_run[0] > clean_run[0] + 100.0 and all(a > b + 100.0 for a, b in zip(floater_run[1], clean_run[1]))
    for spec in ({"largest": True}, pkg("mesh_clean").CleanSpec(min_diameter_frac=0.01), {"min_faces": 5}):
        cleaned = run("with", clean=spec)
        assert cleaned == clean_run, (spec, cleaned, clean_run)  # floats compared exactly
    assert run("with", clean=None) == floater_run
    with pytest.raises(ValueError, match="nothing of"):
        run("with", clean={"min_faces": 100})


def test_export_dynamic_mesh_and_extract_mesh_clean(tmp_path):
    """export_dynamic_mesh(clean=None) writes what the uncleaned path writes; with clean, the written mesh is the reference's cleaning
    of that file, colours gathered with the vertex index.  (DPSR's splat accumulates with float atomics: the field of the first export
    is replayed into the others.)"""
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
    (plain,) = V.export_dynamic_mesh(g, base.deform, base.deform_back, mesh, str(tmp_path / "a"), frames=1, clean=None)
    mesh.psr = lambda *a, **k: fields[0]
    (default,) = V.export_dynamic_mesh(g, base.deform, base.deform_back, mesh, str(tmp_path / "b"), frames=1)
    assert open(plain, "rb").read() == open(default, "rb").read()
    fid = torch.zeros(1, device=g.get_xyz.device)
    _, d_xyz, d_normal = V._deformations(g, base.deform, mesh.deform_normal, fid)
    verts, faces, colors = EV.mesh_and_colors(mesh, g, base.deform_back, d_xyz, d_normal, fid)
    io.write_mesh_ply(str(tmp_path / "c.ply"), verts, faces, vertex_colors=colors)
    assert open(plain, "rb").read() == open(tmp_path / "c.ply", "rb").read()
    (cleaned,) = V.export_dynamic_mesh(g, base.deform, base.deform_back, mesh, str(tmp_path / "d"), frames=1, clean={"largest": True})
    v0, f0, c0 = io.read_mesh_ply(plain, return_colors=True)
    v1, f1, c1 = io.read_mesh_ply(cleaned, return_colors=True)
    rv, rf, rvi, _ = R.clean(v0, f0, largest=True)
    same(v1, rv, "exported verts")
    same(f1, rf, "exported faces")
    same(c1, c0[rvi], "exported colours")
    ev, ef = mesh.extract_mesh(g, base.deform, mesh.deform_normal, t=0.0, clean=pkg("mesh_clean").CleanSpec(largest=True))
    same(host(ef), rf, "extract_mesh faces")
    assert ev.shape == (len(rv), 3)
    print(f"exported mesh: V {len(v0)} F {len(f0)} -> V {len(v1)} F {len(f1)}, components {len(np.unique(R.labels(f0, len(v0))))}")
