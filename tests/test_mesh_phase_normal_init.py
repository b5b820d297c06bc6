"""Entering the mesh phase inside the trainer (MeshPhase(normal_init=True), trainer.py): a Trainer started before dpsr_iter with
zero normals and no centre / scale / threshold crosses it; normal_init=False changes nothing; the sync-free forward does not redo
the iteration; two data-parallel ranks stay replica-identical across it."""
import copy
import os
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, pkg


def test_normal_init_needs_dpsr_and_the_diffmc_mesh():
    T = pkg("trainer")
    with pytest.raises(ValueError):
        T.MeshPhase(None, None, None, dpsr=object(), mesh_source="probes", normal_init=True, device="cpu")
    with pytest.raises(ValueError):
        T.MeshPhase(None, None, None, dpsr=None, mesh_source="diffmc", normal_init=True, device="cpu")
    assert T.MeshPhase(None, None, None, dpsr=object(), mesh_source="diffmc", normal_init=True, device="cpu").normal_init
    assert not T.MeshPhase(None, None, None, mesh_source="diffmc", device="cpu").normal_init


def entering_trainer(rank=0, world=1, res=48, **mesh_kw):
    """test_mesh_phase_anchor.anchored_trainer's scene and networks, reused by import: its Gaussians (normals put back to zero), its
    deformation, normal and appearance networks and its cameras, under a fresh MeshPhase that is given NO center / scale /
    density_thres, and a fresh Trainer on top."""
    from test_mesh_phase_anchor import anchored_trainer
    T, DP = pkg("trainer"), pkg("dpsr")
    tr = anchored_trainer(rank, world, anchor=False, res=res)
    old = tr.mesh
    with torch.no_grad():
        tr.g._normal.zero_()
        tr.g.density_thres_param.zero_()
    dev = tr.g.get_xyz.device
    mesh = T.MeshPhase(old.deform_normal, old.deform_back_normal, old.appearance, dpsr=DP.DPSR(res=(res,) * 3, sig=2.0), n_verts=4000,
                       device=dev, stand_in_weight=1e-3, mesh_source="diffmc", **mesh_kw)
    assert mesh.init == {"density_thres": None, "center": None, "scale": None}
    return T.Trainer(tr.g, tr.deform, tr.deform_back, tr.cameras, opt=pkg("scene").OptimizationParams(), background=tr.bg, rank=rank,
                     world=world, seed=0, mesh=mesh)


@pytest.mark.gpu
def test_a_trainer_crosses_dpsr_iter():
    N = pkg("normal_init")
    tr = entering_trainer(normal_init=True)
    it0 = tr.opt.dpsr_iter
    assert tr.normal_init_due(it0) and not tr.normal_init_due(it0 - 1) and not tr.normal_init_due(it0 + 1)
    for it in (it0 - 2, it0 - 1):
        losses, _ = tr.loss_terms(tr.cameras[0], it)
        assert not ({"mask_loss", "mesh_img_loss", "laplacian_loss"} & set(losses))
        tr.step(it)
        assert float(tr.g._normal.detach().abs().max()) == 0.0 and tr.mesh.last_normal_init is None
    # update_scale_center by hand on a copy of the model, with the networks as they are right before the step
    ref = copy.copy(tr.g)
    N.update_scale_center(ref, tr.deform, gaussian_ratio=1.1)
    gen_before = tr.normal_init_generator.get_state().clone()
    param = tr.g._normal
    loss, _ = tr.step(it0)
    torch.cuda.synchronize()
    assert torch.equal(tr.g.gaussian_center, ref.gaussian_center) and torch.equal(tr.g.gaussian_scale, ref.gaussian_scale)
    assert tr.g._normal is param and torch.isfinite(loss)
    info = tr.mesh.last_normal_init
    assert info is not None and info["F"] > 0
    assert not torch.equal(tr.normal_init_generator.get_state(), gen_before)
    # the chain wrote unit normals and the threshold; this step's own Adam update then moved them by at most their learning rates
    # (normal: rotation_lr * 100 = 0.1, threshold: 0.01; the first Adam step is at most lr per element)
    n0 = pkg("anchor").face_geometry(info["verts"], info["faces"])[1][info["face_index"].long()][info["nearest"]]
    assert float((n0.norm(dim=1) - 1).abs().max()) <= 1e-5
    assert float((tr.g._normal.detach() - n0).abs().max()) <= 0.1 * 1.001
    assert abs(float(tr.g.density_thres_param) - tr.opt.init_density_threshold) <= 0.01 * 1.001
    for it in (it0 + 1, it0 + 2):
        losses, _ = tr.loss_terms(tr.cameras[1], it)
        for k in ("mask_loss", "mesh_img_loss", "laplacian_loss"):
            assert k in losses and bool(torch.isfinite(losses[k])), k
        assert tr.mesh.last_mesh[1].shape[0] > 0
        l2, _ = tr.step(it)
        assert torch.isfinite(l2)
    assert tr.mesh.last_normal_init is info, "normal_initialization ran again after dpsr_iter"


@pytest.mark.gpu
def test_normal_init_sets_unit_normals_and_the_threshold_in_loss_terms():
    """loss_terms alone (no optimizer step): right after it, the normals are unit vectors and the threshold is exactly
    opt.init_density_threshold; the mesh terms of that very iteration are built from them."""
    tr = entering_trainer(normal_init=True)
    it0 = tr.opt.dpsr_iter
    losses, _ = tr.loss_terms(tr.cameras[0], it0)
    n = tr.g._normal.detach()
    ln = n.norm(dim=1)
    assert float(((ln - 1).abs() * (ln > 0)).max()) <= 1e-5 and float((ln > 0).float().mean()) > 0.99
    assert float(tr.g.density_thres_param) == pytest.approx(tr.opt.init_density_threshold, rel=1e-6)
    for k in ("mask_loss", "mesh_img_loss", "laplacian_loss"):
        assert k in losses and bool(torch.isfinite(losses[k])), k
    assert tr.mesh.last_mesh[1].shape[0] > 0


MESH_TERMS = ("mask_loss", "mesh_img_loss", "laplacian_loss")


@pytest.mark.gpu
def test_normal_init_false_is_the_parent_behaviour():
    """Off (the default), the iterations around dpsr_iter give the losses of a MeshPhase built without the argument: the same
    terms in the same order; the render / cycle terms bit for bit; the three mesh terms, which go through the DPSR splat's atomic
    accumulation and differ in the last bits between any two evaluations (tests/test_mesh_phase_anchor.py compares them the same
    way), to 1e-5 relative.  normal_initialization never runs."""
    out = []
    for kw in ({}, {"normal_init": False}):
        tr = entering_trainer(**kw)
        with torch.no_grad():
            tr.g._normal.copy_(torch.nn.functional.normalize(tr.g.get_xyz.detach(), dim=1))
        vals = []
        for it in (tr.opt.dpsr_iter - 1, tr.opt.dpsr_iter, tr.opt.dpsr_iter + 1):
            assert not tr.normal_init_due(it)
            losses, _ = tr.loss_terms(tr.cameras[0], it)
            vals.append({k: v.detach().clone() for k, v in losses.items()})
        assert tr.mesh.last_normal_init is None
        out.append(vals)
    seen = set()
    for a, b in zip(*out):
        assert list(a) == list(b)
        for k in a:
            seen.add(k)
            if k in MESH_TERMS:
                print(k, float(a[k]), float(b[k]))
                assert abs(float(a[k]) - float(b[k])) <= 1e-5 * abs(float(b[k])) + 1e-12, k
            else:
                assert torch.equal(a[k], b[k]), k
    assert set(MESH_TERMS) <= seen, "the mesh terms were never compared"


@pytest.mark.gpu
def test_sync_free_forward_does_not_redo_the_entering_iteration(monkeypatch):
    RZ = pkg("rasterizer")
    monkeypatch.setattr(RZ, "SYNC_FREE", True)
    tr = entering_trainer(normal_init=True)
    it0 = tr.opt.dpsr_iter
    N = pkg("normal_init")
    calls = []
    fn = N.normal_initialization
    monkeypatch.setattr(N, "normal_initialization", lambda *a, **k: calls.append(1) or fn(*a, **k))
    settles = []
    settle = RZ.settle
    monkeypatch.setattr(RZ, "settle", lambda *a, **k: settles.append(1) or settle(*a, **k))
    P = tr.g._xyz.shape[0]
    expect = torch.Generator(device=tr.g._xyz.device)
    expect.set_state(tr.normal_init_generator.get_state())
    torch.rand((P, 3), generator=expect, device=tr.g._xyz.device)
    tr.step(it0)
    torch.cuda.synchronize()
    assert len(calls) == 1 and not settles, "the entering iteration was deferred / redone"
    assert torch.equal(tr.normal_init_generator.get_state(), expect.get_state()), "the generator advanced more than once"
    tr.step(it0 + 1)
    assert len(calls) == 1 and settles, "later iterations defer their settle again"


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    tr = entering_trainer(rank, world, normal_init=True)
    it0 = tr.opt.dpsr_iter
    tr.step(it0 - 1)
    torch.cuda.synchronize()
    before = tr.replicas_identical()
    tr.step(it0)
    tr.step(it0 + 1)
    torch.cuda.synchronize()
    after = tr.replicas_identical()
    torch.save({"before": before, "after": after, "center": tr.g.gaussian_center.cpu(), "scale": tr.g.gaussian_scale.cpu(),
                "normal_sum": float(tr.g._normal.detach().abs().sum())}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_dp2_entering_keeps_replicas_identical():
    world = 2
    with tempfile.TemporaryDirectory() as d:
        port = 33700 + (os.getpid() % 2000)
        mp.start_processes(_worker, args=(world, port, d), nprocs=world, join=True, start_method="spawn")
        r = [torch.load(os.path.join(d, f"rank{k}.pt")) for k in range(world)]
    print(r)
    assert all(x["before"] and x["after"] for x in r)
    assert torch.equal(r[0]["center"], r[1]["center"]) and torch.equal(r[0]["scale"], r[1]["scale"])
    assert r[0]["normal_sum"] == r[1]["normal_sum"] > 0
