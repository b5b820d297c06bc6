"""Gaussian-mesh anchoring inside the trainer (MeshPhase(anchor=True), trainer.py): an anchoring iteration adds 0.1 * anchor_loss,
changes P exactly as plan_anchor predicted, leaves the Gaussian Parameters un-stepped while every network and the density threshold
move, and is followed by a normal step on the new set; a non-anchoring iteration is unchanged by anchor=True; two data-parallel
ranks stay replica-identical through an anchoring event."""
import os
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, pkg


def test_anchor_needs_the_diffmc_mesh():
    T = pkg("trainer")
    with pytest.raises(ValueError):
        T.MeshPhase(None, None, None, mesh_source="probes", anchor=True, device="cpu")
    assert T.MeshPhase(None, None, None, mesh_source="diffmc", anchor=True, device="cpu").anchor
    S = pkg("scene")
    o = S.OptimizationParams()
    assert (o.use_anchor, o.anchor_iter, o.anchor_interval, o.anchor_search_radius, o.anchor_topn, o.anchor_n_1_bs,
            o.anchor_0_1_bs) == (1.0, 8000, 100, 0.0005, 2, 512, 1024)


def anchored_trainer(rank=0, world=1, anchor=True, res=48):
    """make_mesh_trainer's scene and networks with MeshPhase(mesh_source="diffmc", anchor=...) built through its constructor."""
    from test_trainer_dp_gpu import make_trainer
    D, T, DP = pkg("deform"), pkg("trainer"), pkg("dpsr")
    tr = make_trainer(rank, world)
    dev = tr.g.get_xyz.device
    torch.manual_seed(7)
    dn = D.DeformModelNormalSep(is_blender=True, model_name="deform_normal", device=dev, trunk_impl="hip")
    dbn = D.DeformModelNormalSep(is_blender=True, model_name="deform_back_normal", device=dev, trunk_impl="hip")
    app = D.AppearanceModel(is_blender=True, device=dev, trunk_impl="hip")
    with torch.no_grad():
        for m in (dn, dbn):
            torch.nn.init.normal_(m.net.gaussian_normal.weight, std=0.02)
        tr.g._normal.copy_(torch.nn.functional.normalize(tr.g.get_xyz.detach(), dim=1))
    mesh = T.MeshPhase(dn, dbn, app, dpsr=DP.DPSR(res=(res,) * 3, sig=2.0), n_verts=4000, scale=1.0, device=dev,
                       stand_in_weight=1e-3, mesh_source="diffmc", anchor=anchor)
    opt = pkg("scene").OptimizationParams()
    opt.anchor_search_radius = 0.002  # (the test scene is coarse: a wider bound so that every class is populated)
    opt.anchor_0_1_bs = 200
    opt.anchor_n_1_bs = 100
    return T.Trainer(tr.g, tr.deform, tr.deform_back, tr.cameras, opt=opt, background=tr.bg, rank=rank, world=world, seed=0, mesh=mesh)


@pytest.mark.gpu
def test_anchoring_iteration_in_the_trainer():
    tr = anchored_trainer()
    it = tr.opt.anchor_iter + tr.opt.anchor_interval  # 8100: anchoring
    assert tr.anchor_due(it) and not tr.anchor_due(it + 1)
    P0 = tr.g._xyz.shape[0]
    g_before = [p.detach().clone() for p in tr.g.parameters()]
    nets = [tr.deform, tr.deform_back] + tr.mesh.networks()
    n_before = [[p.detach().clone() for p in m.net.parameters()] for m in nets]
    thr = tr.g.density_thres_param.detach().clone()
    seen = {}
    A = pkg("anchor")
    plan_fn = A.plan_anchor

    def spy(*a, **k):
        plan = plan_fn(*a, **k)
        seen["plan"] = plan
        seen["keep"] = int(plan["keep"].sum())
        return plan
    A.plan_anchor = spy
    try:
        losses, _ = tr.loss_terms(tr.cameras[0], it)
    finally:
        A.plan_anchor = plan_fn
    assert "anchor_loss" in losses
    assert torch.equal(losses["anchor_loss"], seen["plan"]["loss"] * 0.1)
    tr._anchor_plan = None
    A.plan_anchor = spy
    try:
        loss, _ = tr.step(it)
    finally:
        A.plan_anchor = plan_fn
    torch.cuda.synchronize()
    info = tr.last_anchor_info
    print(info, seen["plan"]["counts"])
    assert info["old_P"] == P0 and info["new_P"] == seen["keep"] + seen["plan"]["n_new"] == tr.g._xyz.shape[0]
    assert tr.g._xyz.shape[0] != P0 and torch.isfinite(loss)
    # surviving Gaussians are un-stepped: their rows equal the rows they were gathered from
    keep = seen["plan"]["keep"]
    K = int(keep.sum())
    for a, b in zip(tr.g.parameters(), g_before):
        assert torch.equal(a.detach()[:K], b[keep]), "a Gaussian parameter was stepped on the anchoring iteration"
    for m, before in zip(nets, n_before):
        assert any(not torch.equal(p.detach(), q) for p, q in zip(m.net.parameters(), before)), m.model_name
    assert not torch.equal(tr.g.density_thres_param.detach(), thr)
    assert tr.g.xyz_gradient_accum.shape[0] == tr.g._xyz.shape[0] and float(tr.g.denom.sum()) == 0.0
    # a normal step on the new set
    P1 = tr.g._xyz.shape[0]
    x1 = tr.g._xyz.detach().clone()
    loss2, _ = tr.step(it + 1)
    torch.cuda.synchronize()
    assert torch.isfinite(loss2) and tr.g._xyz.shape[0] == P1 and not torch.equal(tr.g._xyz.detach(), x1)


@pytest.mark.gpu
def test_non_anchoring_iteration_is_unchanged_by_anchor_true():
    """Off the anchoring iterations anchor=True changes nothing: plan_anchor is never called, there is no anchor loss, no plan is
    kept and no surgery runs; the loss terms are the same terms as anchor=False's on the same trainer, with the same values up to
    the DPSR splat's atomic accumulation order."""
    tr = anchored_trainer(anchor=True)
    A = pkg("anchor")
    plan_fn, calls = A.plan_anchor, []
    A.plan_anchor = lambda *a, **k: calls.append(1) or plan_fn(*a, **k)
    try:
        for it in (tr.opt.anchor_iter + tr.opt.anchor_interval + 1, tr.opt.anchor_iter, tr.opt.anchor_iter - tr.opt.anchor_interval):
            assert not tr.anchor_due(it)
            la, _ = tr.loss_terms(tr.cameras[1], it)
            assert "anchor_loss" not in la and tr._anchor_plan is None
            tr.mesh.anchor = False
            lb, _ = tr.loss_terms(tr.cameras[1], it)
            tr.mesh.anchor = True
            assert list(la) == list(lb)
            for k in la:  # (the DPSR chain's atomics can differ in the last bits between two evaluations)
                assert abs(float(la[k]) - float(lb[k])) <= 1e-5 * abs(float(lb[k])) + 1e-12, k
            P0 = tr.g._xyz.shape[0]
            tr.step(it)
            assert tr.last_anchor_info is None and tr.g._xyz.shape[0] == P0
    finally:
        A.plan_anchor = plan_fn
    torch.cuda.synchronize()
    assert not calls, "plan_anchor ran on a non-anchoring iteration"


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    tr = anchored_trainer(rank, world)
    it = tr.opt.anchor_iter + tr.opt.anchor_interval
    tr.step(it)
    tr.step(it + 1)
    torch.cuda.synchronize()
    same = tr.replicas_identical()
    torch.save({"same": same, "P": tr.g._xyz.shape[0], "info": tr.last_anchor_info}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_dp2_anchoring_keeps_replicas_identical():
    world = 2
    with tempfile.TemporaryDirectory() as d:
        port = 31700 + (os.getpid() % 2000)
        mp.start_processes(_worker, args=(world, port, d), nprocs=world, join=True, start_method="spawn")
        r = [torch.load(os.path.join(d, f"rank{k}.pt")) for k in range(world)]
    print(r)
    assert r[0]["same"] and r[1]["same"] and r[0]["P"] == r[1]["P"]
    assert r[0]["info"] == r[1]["info"] and r[0]["info"]["new_P"] != r[0]["info"]["old_P"]
