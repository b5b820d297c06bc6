"""MeshPhase(mesh_source="diffmc", mesh_losses="render"): the reference's mask / mesh-image losses (R/train.py:264-275) on the
DiffMC mesh rendered by this project's rasterizer, and the default "stand_in" path unchanged."""
import os
import sys

import pytest
import torch

from conftest import ROOT, pkg


def _trainer(mesh_losses, with_masks=True):
    """The mesh trainer of test_trainer_dp_gpu (res 48) with its mesh phase on DiffMC's mesh; every camera carries a mask: the
    teacher (the same Gaussians) rendered with colour 1 on black."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_trainer_dp_gpu import make_mesh_trainer
    T, S = pkg("trainer"), pkg("scene")
    base = make_mesh_trainer(0, 1)
    g = base.g
    if with_masks:
        with torch.no_grad():
            ones = torch.ones((g.get_xyz.shape[0], 3), device=g.get_xyz.device)
            black = torch.zeros(3, device=g.get_xyz.device)
            for cam in base.cameras:
                img = S.render(cam, g, S.PipelineParams(), black, 0.0, 0.0, 0.0, override_color=ones)["render"]
                cam.gt_alpha_mask = img[0].clamp(0.0, 1.0)[..., None].detach().clone()
    mesh = T.MeshPhase(*base.mesh.networks(), dpsr=base.mesh.dpsr, n_verts=4000, scale=1.0, device=g.get_xyz.device,
                       stand_in_weight=1e-3, mesh_source="diffmc", laplacian_loss_weight=1.0, mesh_losses=mesh_losses)
    return T.Trainer(g, base.deform, base.deform_back, base.cameras, background=base.bg, rank=0, world=1, seed=0, mesh=mesh)


def test_camera_mask_keyword_defaults_to_none():
    syn, S = pkg("synthetic"), pkg("scene")
    cam = S.TorchCamera(syn.make_camera(8, 6), "cpu")
    assert cam.gt_alpha_mask is None
    cam = S.TorchCamera(syn.make_camera(8, 6), "cpu", gt_alpha_mask=torch.ones((6, 8, 1)))
    assert cam.gt_alpha_mask.shape == (6, 8, 1) and cam.gt_alpha_mask.dtype == torch.float32


@pytest.mark.gpu
def test_render_losses_train_three_steps():
    tr = _trainer("render")
    it = tr.opt.dpsr_iter + tr.opt.normal_deform_delay + 1000
    before = [p.detach().clone() for p in tr.params]
    for s in range(3):
        losses, _ = tr.loss_terms(tr.cameras[s], it + s)
        assert {"mask_loss", "mesh_img_loss", "laplacian_loss"} <= set(losses)
        assert all(bool(torch.isfinite(v)) for v in losses.values()), losses
        print(f"step {s}: " + ", ".join(f"{k} {float(v):.4f}" for k, v in losses.items()))
        assert float(losses["mask_loss"]) > 0 and float(losses["mesh_img_loss"]) > 0
        tr.step(it + s)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for p in tr.params)
    assert any(not torch.equal(x.detach(), y) for x, y in zip(tr.params, before))


@pytest.mark.gpu
def test_render_mode_needs_masked_cameras():
    tr = _trainer("render", with_masks=False)
    it = tr.opt.dpsr_iter + tr.opt.normal_deform_delay + 1000
    with pytest.raises(RuntimeError, match="gt_alpha_mask"):
        tr.loss_terms(tr.cameras[0], it)


@pytest.mark.gpu
def test_mask_loss_alone_reaches_threshold_normals_and_positions():
    tr = _trainer("render")
    g, ms = tr.g, tr.mesh
    MR = pkg("mesh_raster")
    for p in (g.density_thres_param, g._normal, g._xyz):
        p.grad = None
    cam = tr.cameras[1]
    verts, faces = ms.surface(g, ms.psr(g, None, None))
    mask = MR.render_mask(None, verts, faces, cam)
    assert mask.shape == (cam.image_height, cam.image_width, 1)
    ((mask - cam.gt_alpha_mask).abs().mean() * 100).backward()
    for p in (g.density_thres_param, g._normal, g._xyz):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0


@pytest.mark.gpu
def test_stand_in_default_is_unchanged():
    """The default mesh_losses is "stand_in" and computes the stand-in terms exactly as before."""
    S = pkg("scene")
    tr = _trainer("stand_in")
    assert pkg("trainer").MeshPhase.__init__.__defaults__[-1] == "stand_in"
    ms, g, opt = tr.mesh, tr.g, tr.opt
    it = opt.dpsr_iter + opt.normal_deform_delay + 1000
    cam = tr.cameras[0]
    losses = {}
    psr = ms.psr(g, None, None)
    tr.diffmc_terms(cam, it, losses, psr)
    verts, faces = ms.surface(g, psr)
    t_v = cam.fid.reshape(1, 1).expand(verts.shape[0], -1)
    vtx_color = ms.appearance.step(verts + tr.deform_back.step(verts.detach(), t_v)[0], t_v)
    u = (verts - g.gaussian_center) / g.gaussian_scale
    radius = u.norm(dim=1)
    mask = S.l1_loss(radius, torch.full_like(radius, 0.5)) * 100 * opt.mask_loss_weight * ms.stand_in_weight
    img = S.l1_loss(vtx_color, 0.5 + 0.5 * torch.sin(3.0 * u.detach())) * opt.mesh_img_loss_weight * (1e3 * ms.stand_in_weight)
    assert torch.equal(losses["mask_loss"], mask) and torch.equal(losses["mesh_img_loss"], img)
