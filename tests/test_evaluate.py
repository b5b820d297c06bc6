"""evaluate.testing end to end: a small mesh-phase scene (2 000 Gaussians, DPSR at 48^3, three 176x176 cameras with masks)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg

N_VIEWS, SIDE = 3, 176


@pytest.fixture(scope="module")
def scene():
    """The mesh trainer of test_trainer_dp_gpu with its mesh phase on DiffMC's mesh, every camera carrying gt_alpha_mask."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_trainer_dp_gpu import make_mesh_trainer
    T, S = pkg("trainer"), pkg("scene")
    base = make_mesh_trainer(0, 1, res=48, P=2000, W=SIDE, H=SIDE, n_frames=N_VIEWS)
    g = base.g
    with torch.no_grad():
        ones = torch.ones((g.get_xyz.shape[0], 3), device=g.get_xyz.device)
        black = torch.zeros(3, device=g.get_xyz.device)
        for cam in base.cameras:
            img = S.render(cam, g, S.PipelineParams(), black, 0.0, 0.0, 0.0, override_color=ones)["render"]
            cam.gt_alpha_mask = img[0].clamp(0.0, 1.0)[..., None].detach().clone()
    mesh = T.MeshPhase(*base.mesh.networks(), dpsr=base.mesh.dpsr, n_verts=4000, scale=1.0, device=g.get_xyz.device,
                       mesh_source="diffmc", mesh_losses="render")
    mesh.bind(g)
    return dict(g=g, deform=base.deform, deform_back=base.deform_back, cameras=base.cameras, bg=base.bg, mesh=mesh,
                pipe=S.PipelineParams())


def _record_psr(mesh):
    """DPSR's splat accumulates with float atomics, so two evaluations of phi differ in their last bits.  To compare testing() bit
    for bit with an independent evaluation of everything downstream, every phi that testing() computes is kept, in call order."""
    fields, orig = [], mesh.psr

    def psr(*a, **k):
        fields.append(orig(*a, **k))
        return fields[-1]

    mesh.psr = psr
    return fields, orig


@pytest.mark.gpu
def test_rows_equal_independent_renders_and_files_parse(scene, tmp_path):
    E, S, MRast, io = pkg("evaluate"), pkg("scene"), pkg("mesh_raster"), pkg("ply_io")
    g, mesh, cams = scene["g"], scene["mesh"], scene["cameras"]
    fields, orig = _record_psr(mesh)
    try:
        res = E.testing(g, scene["deform"], scene["deform_back"], cams, pipe=scene["pipe"], background=scene["bg"], mesh=mesh,
                        out_dir=str(tmp_path), save_meshes=True)
    finally:
        mesh.psr = orig
    views = res["views"]
    assert views.shape == (N_VIEWS, 2, 4) and views.dtype == np.float64 and np.isfinite(views).all() and len(fields) == N_VIEWS
    assert res["columns"] == ("mse", "psnr", "ssim", "ms_ssim")
    with torch.no_grad():
        for idx, cam in enumerate(cams):
            xyz = g.get_xyz.detach()
            t = cam.fid.reshape(1, 1).expand(xyz.shape[0], -1)
            d_xyz, d_rot, d_scl = scene["deform"].step(xyz, t)[:3]
            gs = S.render(cam, g, scene["pipe"], scene["bg"], d_xyz, d_rot, d_scl, False)["render"].clamp(0.0, 1.0)
            verts, faces = mesh.surface(g, fields[idx])
            t_v = cam.fid.reshape(1, 1).expand(verts.shape[0], -1)
            color = mesh.appearance.step(verts + scene["deform_back"].step(verts, t_v)[0], t_v)
            mi = MRast.render_mesh(None, verts, faces, color, cam, whitebackground=True)
            for row, img in enumerate((gs, mi)):
                m = E.image_metrics(img, cam.original_image)
                got = np.array([float(m[k][0]) for k in res["columns"]])
                print(f"view {idx} {'gaussian' if row == 0 else 'mesh'}: " + " ".join(f"{k} {v:.6f}" for k, v in zip(res["columns"], got)))
                assert np.array_equal(got, views[idx, row]), (idx, row, got, views[idx, row])
            v, f, c = io.read_mesh_ply(str(tmp_path / "test_results" / "dynamic_mesh" / f"frame_{idx}.ply"), return_colors=True)
            assert len(v) > 0 and len(f) > 0
            assert np.array_equal(v, verts.cpu().numpy()) and np.array_equal(f, faces.cpu().numpy())
            assert np.array_equal(c[:, :3], np.clip(color.cpu().numpy() * 255, 0, 255).astype(np.uint8)) and (c[:, 3] == 255).all()
    for row, name in enumerate(("gaussian", "mesh")):
        for i, k in enumerate(res["columns"]):
            assert res[name][k] == float(views[:, row, i].mean())
    assert res["time_per_view"] > 0 and abs(res["fps"] * res["time_per_view"] - 1.0) < 1e-12
    lines = open(tmp_path / "test_results" / "test_result.txt").read().split("\n")
    assert len(lines) == 3 and lines[2] == ""
    tok = [ln.split() for ln in lines[:2]]
    assert tok[0][:2] == ["Gaussian", "image"] and tok[0][2::2] == ["PSNR", "SSIM", "MSSSIM"]
    assert tok[1][:2] == ["Mesh", "image"] and tok[1][2::2] == ["PSNR", "SSIM", "MSSSIM", "total_time", "fps"]
    for ln, name in zip(tok, ("gaussian", "mesh")):
        for label, k in (("PSNR", "psnr"), ("SSIM", "ssim"), ("MSSSIM", "ms_ssim")):
            assert ln[ln.index(label) + 1] == f"{res[name][k]:.4f}"
    assert tok[1][tok[1].index("fps") + 1] == f"{res['fps']:.4f}"
    assert "LPIPS" not in "".join(lines)


@pytest.mark.gpu
def test_without_mesh_only_the_gaussian_columns_are_filled(scene, tmp_path):
    E = pkg("evaluate")
    res = E.testing(scene["g"], scene["deform"], scene["deform_back"], scene["cameras"], pipe=scene["pipe"], background=scene["bg"],
                    out_dir=str(tmp_path))
    assert res["mesh"] is None and np.isfinite(res["views"][:, 0]).all() and np.isnan(res["views"][:, 1]).all()
    assert not os.path.exists(tmp_path / "test_results" / "dynamic_mesh")
    text = open(tmp_path / "test_results" / "test_result.txt").read()
    assert text.startswith("Gaussian image PSNR ") and "Mesh image" not in text and "fps" in text
    with pytest.raises(ValueError):
        E.testing(scene["g"], scene["deform"], scene["deform_back"], scene["cameras"], pipe=scene["pipe"], background=scene["bg"],
                  out_dir=str(tmp_path), save_meshes=True)
