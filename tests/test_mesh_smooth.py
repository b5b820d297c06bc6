"""GPU tests of mesh smoothing (dg-mesh_amd/mesh_smooth.py, the smoothing kernel of csrc/mesh_edges.hip) against the numpy reference
tests/_edges_ref.py.  The comparison is byte for byte: every operation of a step is an IEEE fp64 add, subtract, multiply or divide in
a fixed order, without contraction, followed by one conversion to fp32, so there is nothing to measure a tolerance against.  The one
exception is stated where it is made: IEEE 754 leaves the sign and payload of a NaN that an operation produces from a NaN open, so
where the reference has a NaN the device must have a NaN, and everywhere else the bytes must be equal."""
import os
import sys

import numpy as np
import pytest
import torch

import _edges_ref as R
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu


def S():
    return pkg("mesh_smooth")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared inputs are read-only arrays)


def host(t):
    return t.cpu().numpy()


def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
    diff = int((a.view(np.uint8) != b.view(np.uint8)).sum())
    worst = float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64)))) if diff else 0.0
    assert diff == 0, f"{what}: {diff} bytes differ, largest difference {worst:.3e}"


def run(verts, faces, **kw):
    """smooth_mesh twice on the same device tensors: the two results byte for byte equal, the inputs untouched; -> numpy."""
    dv, df = dev(verts), dev(faces)
    v0, f0 = dv.clone(), df.clone()
    first = host(S().smooth_mesh(dv, df, **kw))
    second = host(S().smooth_mesh(dv, df, **kw))
    same(second, first, "run 1 against run 0")
    same(host(dv), host(v0), "input vertices after the call")
    same(host(df), host(f0), "input faces after the call")
    return first


@pytest.fixture(scope="module")
def noisy():
    verts, faces = R.noisy_icosphere(3, 0.02, 0)
    verts.setflags(write=False), faces.setflags(write=False)
    return verts, faces


@pytest.mark.parametrize("boundary", R.BOUNDARIES)
@pytest.mark.parametrize("method", ["taubin", "laplacian"])
@pytest.mark.parametrize("iterations", [0, 1, 10])
def test_noisy_icosphere_equals_the_reference(noisy, iterations, method, boundary):
    verts, faces = noisy
    got = run(verts, faces, iterations=iterations, method=method, boundary=boundary)
    same(got, R.smooth(verts, faces, iterations, 0.5, -0.53, method, boundary), f"{method} {boundary} x {iterations}")
    if iterations == 0:
        dv = dev(verts)
        assert S().smooth_mesh(dv, dev(faces), iterations=0, method=method, boundary=boundary) is dv  # the input itself


def test_noisy_icosphere_other_factors(noisy):
    verts, faces = noisy
    for lam, mu in ((1.0, -1.01), (0.33, -0.34), (0.6307, -0.6732)):
        same(run(verts, faces, iterations=3, lam=lam, mu=mu), R.smooth(verts, faces, 3, lam, mu), f"lam {lam} mu {mu}")


@pytest.mark.parametrize("method", ["taubin", "laplacian"])
@pytest.mark.parametrize("iterations", [1, 10])
def test_grid_patch_rim(iterations, method):
    """fixed leaves the rim rows bit-unchanged; curve moves them, and only inside the rim's plane z = 0; free pulls the rim out of its
    plane towards the lifted interior and, with the Laplacian, shrinks its extent."""
    n, m = 9, 13
    verts, faces = R.grid_patch(n, m, seed=4)
    rim = R.grid_rim(n, m)
    out = {b: run(verts, faces, iterations=iterations, method=method, boundary=b) for b in R.BOUNDARIES}
    for b in R.BOUNDARIES:
        same(out[b], R.smooth(verts, faces, iterations, 0.5, -0.53, method, b), f"{method} {b} x {iterations}")
    same(out["fixed"][rim], verts[rim], "fixed: the rim")
    assert (out["fixed"][~rim] != verts[~rim]).any()
    assert (out["curve"][rim, 2] == 0).all() and (out["curve"][rim, :2] != verts[rim, :2]).any()
    assert (out["free"][rim, 2] != 0).any()
    if method == "laplacian":
        extent = lambda v: float(np.ptp(v[rim, 0]) * np.ptp(v[rim, 1]))
        assert extent(out["free"]) < extent(verts)


def nan_aware_same(got, ref, what):
    """Bytes equal wherever the reference is not NaN; NaN wherever it is (module docstring)."""
    nan = np.isnan(ref)
    assert (np.isnan(got) == nan).all(), f"{what}: NaNs at other places"
    same(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), ref), what)


@pytest.mark.parametrize("boundary", R.BOUNDARIES)
@pytest.mark.parametrize("method,iterations", [("taubin", 1), ("laplacian", 1), ("taubin", 10)])
def test_salted_mesh(method, iterations, boundary):
    """Unused vertices, vertices of only-invalid faces and a used NaN vertex are bit-unchanged.  The NaN vertex's neighbours are not
    protected: their sums take the NaN in, so they are NaN after the first step and copied from then on, and the NaN spreads by one
    ring per step -- after one Laplacian step exactly the ring of the NaN vertex is NaN, after a Taubin iteration (two steps) two
    rings are."""
    verts, faces, sets = R.salted()
    got = run(verts, faces, iterations=iterations, method=method, boundary=boundary)
    ref = R.smooth(verts, faces, iterations, 0.5, -0.53, method, boundary)
    nan_aware_same(got, ref, f"{method} {boundary} x {iterations}")
    same(got[sets["unused"]], verts[sets["unused"]], "unused vertices and vertices of only-invalid faces")
    same(got[sets["nan"]], verts[sets["nan"]], "the NaN vertex")
    t = R.edge_table(faces, len(verts))
    ring = lambda vs: set(int(k) for v in vs for k in t["adj"][t["adj_offset"][v]:t["adj_offset"][v + 1]])
    one = ring([sets["nan"]])
    two = one | ring(one)
    if iterations == 1:
        expect = (one if method == "laplacian" else two) | {sets["nan"]}
        assert set(np.nonzero(np.isnan(got).any(1))[0].tolist()) - set(sets["unused"].tolist()) == expect
        assert 0 < len(one) < len(two) < 42  # the mesh is larger than two rings: the statement is not empty


def test_wheel_and_soup_equal_the_reference():
    """A list longer than a workgroup, and lists over non-manifold edges."""
    for verts, faces in (R.wheel(600), R.random_soup()):
        for boundary in R.BOUNDARIES:
            same(run(verts, faces, iterations=2, boundary=boundary), R.smooth(verts, faces, 2, boundary=boundary), boundary)


def test_empty_meshes_and_apply():
    Sm = S()
    none = torch.zeros((0, 3), device="cuda")
    assert Sm.smooth_mesh(none, torch.zeros((0, 3), dtype=torch.int32, device="cuda")).shape == (0, 3)
    verts, faces = R.tetrahedron()
    lone = dev(verts)
    same(host(Sm.smooth_mesh(lone, torch.zeros((0, 3), dtype=torch.int32, device="cuda"))), verts, "no faces: nothing moves")
    colour = torch.rand(4, 3, device="cuda")
    fd = dev(faces)
    v, f, c = Sm.apply({"iterations": 2, "method": "laplacian"}, lone, fd, colour)
    assert f is fd and c is colour  # smoothing moves vertices only
    same(host(v), R.smooth(verts, faces, 2, method="laplacian"), "apply")
    assert Sm.apply(None, lone, f, colour) == (lone, f, colour)
    with pytest.raises(RuntimeError, match="float32"):
        Sm.smooth_mesh(lone.double(), dev(faces))


def test_cli_round_trips_a_ply(tmp_path, capsys):
    io = pkg("ply_io")
    verts, faces = R.noisy_icosphere(2, 0.03, 1)
    colour = np.random.RandomState(1).rand(len(verts), 3).astype(np.float32)
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    io.write_mesh_ply(src, verts, faces, vertex_colors=colour)
    v0, f0, c0 = io.read_mesh_ply(src, return_colors=True)
    assert S().main([src, dst, "--iterations", "4", "--boundary", "free"]) == 0
    assert "iterations 4" in capsys.readouterr().out
    v1, f1, c1 = io.read_mesh_ply(dst, return_colors=True)
    same(f1, f0, "faces")
    same(c1, c0, "colours")
    same(v1, R.smooth(v0, f0, 4, boundary="free"), "vertices")
    io.write_mesh_ply(src, verts, faces)  # a file without colours stays without
    assert S().main([src, dst, "--method", "laplacian"]) == 0
    assert io.read_mesh_ply(dst, return_colors=True)[2] is None
    assert pkg("mesh_topology").main([src, dst]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len([ln for ln in lines if ln.startswith("{")]) == 2 and '"watertight": true' in lines[-1]


def test_export_dynamic_mesh_and_extract_mesh_smooth(tmp_path):
    """export_dynamic_mesh(smooth=None) writes what it wrote before; with smooth the written mesh has the faces and colours of the
    unsmoothed export and the reference's smoothing of its vertices; extract_mesh smooths after `clean` and before `simplify`.
    (DPSR's splat accumulates with float atomics: the field of the first export is replayed into the others.)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_trainer_dp_gpu import make_mesh_trainer
    import _meshclean_ref as RC
    T, V, io = pkg("trainer"), pkg("visualize"), pkg("ply_io")
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
    (plain,) = V.export_dynamic_mesh(g, base.deform, base.deform_back, mesh, str(tmp_path / "a"), frames=1)
    mesh.psr = lambda *a, **k: fields[0]
    (none,) = V.export_dynamic_mesh(g, base.deform, base.deform_back, mesh, str(tmp_path / "b"), frames=1, smooth=None)
    assert open(plain, "rb").read() == open(none, "rb").read()
    spec = S().SmoothSpec(iterations=3, boundary="free")
    (smoothed,) = V.export_dynamic_mesh(g, base.deform, base.deform_back, mesh, str(tmp_path / "c"), frames=1, smooth=spec)
    v0, f0, c0 = io.read_mesh_ply(plain, return_colors=True)
    v1, f1, c1 = io.read_mesh_ply(smoothed, return_colors=True)
    same(f1, f0, "exported faces")
    same(c1, c0, "exported colours")
    assert (v1 != v0).any()
    same(v1, R.smooth(v0, f0, 3, boundary="free"), "exported vertices")
    # clean, then smooth, then simplify
    pv, pf = (host(t) for t in mesh.extract_mesh(g, base.deform, mesh.deform_normal, t=0.0))
    ev, ef = mesh.extract_mesh(g, base.deform, mesh.deform_normal, t=0.0, clean={"largest": True}, smooth={"iterations": 2})
    cv, cf, _, _ = RC.clean(pv, pf, largest=True)
    same(host(ef), cf, "extract_mesh faces")
    same(host(ev), R.smooth(cv, cf, 2), "extract_mesh vertices: smoothed after the cleaning")
    sv, sf = mesh.extract_mesh(g, base.deform, mesh.deform_normal, t=0.0, simplify={"grid": 16}, smooth={"iterations": 2})
    want = pkg("mesh_simplify").simplify_mesh(dev(R.smooth(pv, pf, 2)), dev(pf), grid=16)
    same(host(sf), host(want[1]), "extract_mesh faces: simplified after the smoothing")
    same(host(sv), host(want[0]), "extract_mesh vertices: simplified after the smoothing")
    print(f"exported mesh: V {len(v0)} F {len(f0)}, largest move {float(np.abs(v1 - v0).max()):.3e}")
