"""Differentiable marching cubes (dg-mesh_amd/marching_cubes.py, csrc/marching_cubes.hip, case table csrc/mc_tables.hpp from
tools/gen_mc_tables.py).  diso is not vendored, so there is no third-party output to compare with: the CPU tests check that the
table is what its generator writes and that the restatement of the conventions (tests/_mc_ref.py) produces closed, consistently
oriented meshes; the GPU tests check the kernels against that restatement exactly, the meshes geometrically, the adjoint against
the analytic one and central differences, and the mesh phase of the trainer on DiffMC's mesh.  At scale: bit-exact on grids
around the block scan's one-segment-per-thread limit (NB = 1024, 1025, 1055, 1099) and on the 288^3 DPSR grid, whose backward
is checked there too."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _mc_ref as R
from conftest import ROOT, pkg


def _padded(core, outside=1.0):
    """core surrounded by one layer of outside values: the surface does not reach the grid boundary."""
    g = np.full(tuple(s + 2 for s in core.shape), outside, np.float32)
    g[1:-1, 1:-1, 1:-1] = core
    return g


def sphere(n, r, c=None):
    c = (n - 1) / 2 if c is None else c
    i = np.arange(n, dtype=np.float64)
    x, y, z = np.meshgrid(i, i, i, indexing="ij")
    return (np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - r).astype(np.float32)


def torus(n, R0, r0):
    c = (n - 1) / 2
    i = np.arange(n, dtype=np.float64) - c
    x, y, z = np.meshgrid(i, i, i, indexing="ij")
    return (np.sqrt((np.sqrt(x ** 2 + y ** 2) - R0) ** 2 + z ** 2) - r0).astype(np.float32)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
def test_generator_reproduces_the_committed_table():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_mc_tables.py"), "--check"], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "largest triangle count per case: 5" in out.stdout


def test_table_shape_and_counts():
    corner_a, count, tris, max_tris = R.load_table()
    assert max_tris == 5 and count[0] == 0 and count[255] == 0 and all(count[1 << c] == 1 for c in range(8))
    for case in range(256):
        row = tris[case]
        assert (row[:3 * count[case]] >= 0).all() and (row[:3 * count[case]] < 12).all() and (row[3 * count[case]:] == -1).all()
    assert sorted(corner_a.tolist()) == [0, 0, 0, 1, 1, 2, 2, 3, 4, 4, 5, 6]


@pytest.mark.parametrize("seed", range(6))
def test_restatement_mesh_is_closed_and_oriented_on_random_signs(seed):
    rng = np.random.RandomState(seed)
    shape = [(8, 9, 10), (5, 7, 6), (12, 4, 9)][seed % 3]
    core = np.where(rng.rand(*shape) < 0.5, -1.0, 1.0).astype(np.float32) * rng.uniform(0.2, 1.0, shape).astype(np.float32)
    v, f, _ = R.marching_cubes(_padded(core))
    assert len(f) > 0 and R.is_closed_and_oriented(f)
    assert np.isfinite(v).all()


def test_restatement_mesh_is_closed_when_every_face_is_ambiguous():
    """Checkerboard signs on 8x9x10: each cube face of the interior has two diagonal inside corners."""
    i, j, k = np.meshgrid(np.arange(8), np.arange(9), np.arange(10), indexing="ij")
    rng = np.random.RandomState(3)
    core = (np.where((i + j + k) % 2 == 0, -1.0, 1.0) * rng.uniform(0.3, 1.0, i.shape)).astype(np.float32)
    v, f, _ = R.marching_cubes(_padded(core))
    assert R.is_closed_and_oriented(f)
    assert len(f) > 0


def test_restatement_sphere_normals_point_outward():
    g = sphere(24, 7.3)
    v, f, _ = R.marching_cubes(g, normalize=False)
    area, n = R.area_and_normals(v, f)
    cen = v[f].mean(1) - 11.5
    assert (np.einsum("ij,ij->i", n, cen) > 0).all()
    assert R.is_closed_and_oriented(f) and R.euler_characteristic(v, f) == 2


def test_mesh_ply_round_trip(tmp_path):
    P = pkg("ply_io")
    rng = np.random.RandomState(0)
    v = rng.randn(50, 3).astype(np.float32)
    f = rng.randint(0, 50, (70, 3)).astype(np.int32)
    path = str(tmp_path / "m.ply")
    P.write_mesh_ply(path, v, f)
    head = open(path, "rb").read(400)
    assert b"property list uchar int vertex_indices" in head and b"binary_little_endian" in head
    v2, f2 = P.read_mesh_ply(path)
    assert np.array_equal(v, v2) and np.array_equal(f, f2) and f2.dtype == np.int32
    with pytest.raises(ValueError, match="list properties"):  # the checkpoint reader keeps refusing list properties
        P.read_ply(path)
    P.write_mesh_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v3, f3 = P.read_mesh_ply(path)
    assert v3.shape == (0, 3) and f3.shape == (0, 3)


def test_diffmc_refuses_cpu_and_other_dtypes():
    M = pkg("marching_cubes")
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.DiffMC()(torch.zeros(4, 4, 4))
    with pytest.raises(RuntimeError, match="float32"):
        M.DiffMC(dtype=torch.float64)


def test_c_abi_refuses_bad_arguments_without_gpu():
    L = pkg("_lib")
    lib = L.lib()
    assert lib.dgm_mc_scratch_bytes(1, 4, 4) == 0 and lib.dgm_mc_scratch_bytes(2000, 2000, 2000) == 0
    assert lib.dgm_mc_scratch_bytes(288, 288, 288) > 0
    assert lib.dgm_mc_count(1, 4, 4, None, 0.0, None, None, None) != 0 and b">= 2" in lib.dgm_last_error()
    assert lib.dgm_mc_count(2000, 2000, 2000, None, 0.0, None, None, None) != 0 and b"int32" in lib.dgm_last_error()
    assert lib.dgm_mc_count(4, 4, 4, None, 0.0, None, None, None) != 0 and b"NULL" in lib.dgm_last_error()
    assert lib.dgm_mc_emit(4, 4, 4, None, None, 0.0, 1, None, 0, 0, None, None, None) != 0
    assert lib.dgm_mc_backward(4, 4, 4, None, None, 0.0, 1, None, 0, None, None, None, None) != 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _gpu(grid, iso=0.0, deform=None, normalize=True):
    M = pkg("marching_cubes")
    g = torch.tensor(grid, device="cuda")
    d = torch.tensor(deform, device="cuda") if deform is not None else None
    v, f = M.DiffMC()(g, deform=d, isovalue=iso, normalize=normalize)
    assert v.dtype == torch.float32 and f.dtype == torch.int32
    return v.cpu().numpy(), f.cpu().numpy()


def _exact(grid, iso=0.0, deform=None, normalize=True):
    v, f = _gpu(grid, iso, deform, normalize)
    rv, rf, _ = R.marching_cubes(grid, iso, deform, normalize)
    assert v.shape == rv.shape and f.shape == rf.shape
    assert np.array_equal(f, rf)
    ulp = np.abs(v.view(np.int32).astype(np.int64) - rv.view(np.int32).astype(np.int64))
    assert (ulp <= 1).all(), float(np.abs(v - rv).max())
    return v, f


def _noise(shape, seed):
    rng = np.random.RandomState(seed)
    return rng.randn(*shape).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("with_deform", [False, True])
def test_gpu_matches_restatement_exactly(normalize, with_deform):
    rng = np.random.RandomState(11)
    cases = [(sphere(64, 20.3), 0.0), (torus(48, 14.0, 5.2), 0.0), (_noise((33, 40, 47), 1), 0.1)]
    eq = np.round(_noise((17, 18, 19), 2) * 2) / 2  # many values exactly at the iso level
    cases.append((eq.astype(np.float32), 0.5))
    for grid, iso in cases:
        deform = (0.3 * rng.randn(*grid.shape, 3)).astype(np.float32) if with_deform else None
        v, f = _exact(grid, iso, deform, normalize)
        assert len(f) > 0


@pytest.mark.gpu
def test_gpu_matches_restatement_on_the_opacity_field():
    S = pkg("synthetic")
    MU = pkg("mesh_utils")
    g = S.make_gaussians(3000, seed=0, kind="aniso", extent=0.7)
    a = S.activate(g)
    t = lambda x: torch.tensor(x, device="cuda")
    occ = MU.get_opacity_field_from_gaussians(t(a["means3D"]), t(a["rotations"]), t(a["scales"]), t(a["opacities"]),
                                              resolution=64, num_blocks=16)
    grid = (-occ).cpu().numpy()
    v, f = _exact(grid, iso=-0.01)
    assert len(f) > 0


@pytest.mark.gpu
def test_gpu_empty_surface():
    M = pkg("marching_cubes")
    g = torch.ones(9, 10, 11, device="cuda", requires_grad=True)
    d = torch.zeros(9, 10, 11, 3, device="cuda", requires_grad=True)
    v, f = M.DiffMC()(g, deform=d)
    assert v.shape == (0, 3) and f.shape == (0, 3) and f.dtype == torch.int32
    (v.sum() + 0.0).backward()
    assert g.grad is not None and float(g.grad.abs().max()) == 0.0 and float(d.grad.abs().max()) == 0.0


@pytest.mark.gpu
def test_gpu_geometry_sphere_and_torus():
    r = 40.5
    v, f = _gpu(sphere(128, r), normalize=False)
    assert R.is_closed_and_oriented(f) and R.euler_characteristic(v, f) == 2
    area, n = R.area_and_normals(v, f)
    assert abs(area - 4 * math.pi * r * r) < 0.01 * 4 * math.pi * r * r
    cen = v[f].mean(1) - 63.5
    assert (np.einsum("ij,ij->i", n, cen) > 0).all()
    v, f = _gpu(torus(96, 28.0, 10.0), normalize=False)
    assert R.is_closed_and_oriented(f) and R.euler_characteristic(v, f) == 0


def _grads(grid, deform, iso, normalize, w):
    M = pkg("marching_cubes")
    g = torch.tensor(grid, device="cuda", requires_grad=True)
    d = torch.tensor(deform, device="cuda", requires_grad=True) if deform is not None else None
    v, f = M.DiffMC()(g, deform=d, isovalue=iso, normalize=normalize)
    (v * torch.tensor(w, device="cuda")).sum().backward()
    return g.grad.cpu().numpy(), (d.grad.cpu().numpy() if d is not None else None)


@pytest.mark.gpu
@pytest.mark.parametrize("with_deform", [False, True])
def test_gpu_backward_matches_analytic_adjoint_and_is_bit_reproducible(with_deform):
    rng = np.random.RandomState(5)
    grid = _noise((21, 26, 30), 7)
    deform = (0.2 * rng.randn(*grid.shape, 3)).astype(np.float32) if with_deform else None
    rv, rf, rec = R.marching_cubes(grid, 0.05, deform, True)
    w = rng.randn(*rv.shape).astype(np.float32)
    dg, dd = _grads(grid, deform, 0.05, True, w)
    ref_g, ref_d = R.backward(rec, w, with_deform)
    assert np.abs(dg - ref_g).max() <= 1e-6 * np.abs(ref_g).max()
    if with_deform:
        assert np.abs(dd - ref_d).max() <= 1e-6 * np.abs(ref_d).max()
    dg2, dd2 = _grads(grid, deform, 0.05, True, w)
    assert np.array_equal(dg, dg2) and (dd is None or np.array_equal(dd, dd2))


@pytest.mark.gpu
def test_gpu_backward_matches_central_differences():
    rng = np.random.RandomState(9)
    grid = sphere(12, 3.7) + (0.05 * rng.randn(12, 12, 12)).astype(np.float32)
    grid[np.abs(grid) < 0.05] = 0.05  # no value near the iso level: a small step flips no sign
    deform = (0.1 * rng.randn(12, 12, 12, 3)).astype(np.float32)
    rv, _, _ = R.marching_cubes(grid, 0.0, deform, True)
    w = rng.randn(*rv.shape)
    dg, dd = _grads(grid, deform, 0.0, True, w.astype(np.float32))
    L = lambda gr, de: float((R.marching_cubes(gr, 0.0, de, True, dtype=np.float64)[0] * w).sum())
    g64, d64 = grid.astype(np.float64), deform.astype(np.float64)
    h = 1e-6
    pts = [tuple(p) for p in np.argwhere(np.abs(dg) > 0)[::7][:40]]
    assert len(pts) >= 20
    for p in pts:
        a, b = g64.copy(), g64.copy()
        a[p] += h
        b[p] -= h
        fd = (L(a, d64) - L(b, d64)) / (2 * h)
        assert abs(fd - dg[p]) <= 1e-3 * max(1.0, abs(fd)), (p, fd, dg[p])
        c = rng.randint(3)
        a, b = d64.copy(), d64.copy()
        a[p + (c,)] += h
        b[p + (c,)] -= h
        fd = (L(g64, a) - L(g64, b)) / (2 * h)
        assert abs(fd - dd[p + (c,)]) <= 1e-3 * max(1.0, abs(fd)), (p, c, fd, dd[p + (c,)])


def _diffmc_trainer():
    """The mesh trainer of test_trainer_dp_gpu (res 48) with its mesh phase on DiffMC's mesh."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_trainer_dp_gpu import make_mesh_trainer
    T = pkg("trainer")
    base = make_mesh_trainer(0, 1)
    mesh = T.MeshPhase(*base.mesh.networks(), dpsr=base.mesh.dpsr, n_verts=4000, scale=1.0, device=base.g.get_xyz.device,
                       stand_in_weight=1e-3, mesh_source="diffmc", laplacian_loss_weight=1.0)
    return T.Trainer(base.g, base.deform, base.deform_back, base.cameras, background=base.bg, rank=0, world=1, seed=0, mesh=mesh)


@pytest.mark.gpu
def test_mesh_phase_diffmc_steps_and_moves_everything():
    DP = pkg("dpsr")
    tr = _diffmc_trainer()
    before = [p.detach().clone() for p in tr.params]
    it = tr.opt.dpsr_iter + tr.opt.normal_deform_delay + 1000
    for s in range(3):
        losses, _ = tr.loss_terms(tr.cameras[s], it + s)
        assert all(bool(torch.isfinite(v)) for v in losses.values()), losses
        assert "laplacian_loss" in losses
        verts, faces = tr.mesh.last_mesh
        assert verts.shape[0] > 100 and faces.shape[0] > 100
        expect = DP._laplace_regularizer_torch(verts.cpu(), faces.cpu()) * 1000 * (1 - (it + s) / tr.opt.iterations)
        assert abs(float(losses["laplacian_loss"]) - float(expect)) <= 1e-5 * abs(float(expect))
        tr.step(it + s)
    torch.cuda.synchronize()
    moved = [not torch.equal(x.detach(), y) for x, y in zip(tr.params, before)]
    off = 6
    for m in [tr.deform, tr.deform_back] + tr.mesh.networks():
        n = len(list(m.net.parameters()))
        assert any(moved[off:off + n]), m.model_name
        off += n
    assert moved[0] and moved[off] and moved[off + 1], "positions / normals / density threshold did not move"
    assert all(bool(torch.isfinite(p).all()) for p in tr.params)
    verts, faces = tr.mesh.extract_mesh(tr.g, tr.deform, tr.mesh.deform_normal, 0.3)
    assert verts.shape[0] > 100 and faces.dtype == torch.int32 and int(faces.max()) < verts.shape[0]


@pytest.mark.gpu
def test_density_threshold_gradient_flows_through_diffmc():
    """Only the Laplacian term of the DiffMC mesh: its gradient reaches the density threshold and the normals through DPSR."""
    DP = pkg("dpsr")
    tr = _diffmc_trainer()
    ms = tr.mesh
    g = tr.g
    for p in (g.density_thres_param, g._normal, g._xyz):
        p.grad = None
    psr = ms.psr(g, None, None)
    verts, faces = ms.surface(g, psr)
    DP.laplace_regularizer_const(verts, faces).backward()
    for p in (g.density_thres_param, g._normal, g._xyz):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0


# ---- at scale: the block scan past one segment per thread, the 288^3 DPSR grid of the reference configs --------------------------
def _bit_exact(grid, iso=0.0, deform=None, normalize=True):
    """vertices bit-equal and faces equal to the restatement -> (verts, faces, restatement record)."""
    v, f = _gpu(grid, iso, deform, normalize)
    rv, rf, rec = R.marching_cubes(grid, iso, deform, normalize)
    assert f.shape == rf.shape and np.array_equal(f, rf)
    assert v.shape == rv.shape and np.array_equal(v.view(np.int32), rv.view(np.int32)), float(np.abs(v - rv).max())
    print(f"grid {grid.shape}: {len(rv)} vertices, {len(rf)} faces bit-equal")
    return v, f, rec


def _scan_blocks(shape):
    """NB of dgm_mc_count: one block total per 1024 points, scanned by mc_scan_kernel's 1024 threads, ceil(NB / 1024) each."""
    return -(-int(np.prod(shape)) // 1024)


def checkerboard(shape, seed):
    """Alternating signs: every cell is the two-tetrahedra case, 4 triangles, every edge crossed -- the densest mesh."""
    i, j, k = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")
    mag = np.random.RandomState(seed).uniform(0.3, 1.0, shape)
    return (np.where((i + j + k) % 2 == 0, -1.0, 1.0) * mag).astype(np.float32)


def dpsr_phi_288(sig=3.0):
    """The indicator grid of the reference configs' DPSR (grid_res 288, dpsr_sig 3.0) on a noisy oriented sphere, on the device."""
    import _dpsr_ref
    D = pkg("dpsr")
    Vn, Nn = _dpsr_ref.noisy_sphere(100000, 288)
    V, N = torch.tensor(Vn, device="cuda"), torch.tensor(Nn, device="cuda")
    return D.DPSR(res=(288, 288, 288), sig=sig)(V.unsqueeze(0), N.unsqueeze(0))[0]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,nb", [((64, 128, 128), 1024), ((2, 2, 262145), 1025), ((262145, 2, 2), 1025),
                                      ((2, 600, 900), 1055)])
def test_gpu_bit_exact_around_one_scan_segment_per_thread(shape, nb):
    """NB = 1024 gives every scan thread one block; NB = 1025 and 1055 give seg = 2 with a ragged last thread, so a rounded-down
    segment would leave the last blocks' offsets unwritten."""
    assert _scan_blocks(shape) == nb
    _, f, _ = _bit_exact(_noise(shape, nb), 0.0)
    assert len(f) > 0


@pytest.mark.gpu
def test_gpu_bit_exact_on_a_checkerboard_past_one_segment():
    shape = (104, 104, 104)
    assert _scan_blocks(shape) == 1099
    v, f, _ = _bit_exact(checkerboard(shape, 3), 0.0)
    assert len(f) == 4 * 103 ** 3


@pytest.mark.gpu
@pytest.mark.parametrize("with_deform", [False, True])
def test_gpu_on_the_dpsr_grid_at_288(with_deform):
    """The GPU's DPSR phi at 288^3 fed to both sides: forward bit-exact, backward within 1e-6 of max of the analytic adjoint
    (per grid point <= 6 incident edges of 3 terms, each a few roundings: ~30 u = 1.8e-6 of the largest term; the terms of one
    point rarely cancel to below half of the max) and bit-identical run to run."""
    grid = dpsr_phi_288().cpu().numpy()
    assert _scan_blocks(grid.shape) > 1024
    rng = np.random.RandomState(288)
    deform = (0.3 * rng.randn(*grid.shape, 3)).astype(np.float32) if with_deform else None
    v, f, rec = _bit_exact(grid, 0.0, deform, True)
    assert len(f) > 100000
    w = rng.randn(*v.shape).astype(np.float32)
    dg, dd = _grads(grid, deform, 0.0, True, w)
    ref_g, ref_d = R.backward(rec, w, with_deform)
    err = np.abs(dg - ref_g).max() / np.abs(ref_g).max()
    print(f"DiffMC backward 288^3 dgrid: err {err:.3e} of max, bound 1e-6")
    assert err <= 1e-6
    if with_deform:
        err = np.abs(dd - ref_d).max() / np.abs(ref_d).max()
        print(f"DiffMC backward 288^3 ddeform: err {err:.3e} of max, bound 1e-6")
        assert err <= 1e-6
    dg2, dd2 = _grads(grid, deform, 0.0, True, w)
    assert np.array_equal(dg, dg2) and (dd is None or np.array_equal(dd, dd2))
