"""normal_init.normal_initialization end to end on the GPU: from the golden's Gaussians against the reference's own result
(tests/golden/normal_init_small.npz), on a sphere shell (orientation, unit length, Parameter identity, Adam state), with `out_dir`,
and on a field without a surface."""
import os
import types

import numpy as np
import pytest
import torch

from _anchor_ref import PolyField
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "normal_init_small.npz")


def model(xyz, rotation, scaling, opacity):
    S = pkg("scene")
    P = len(xyz)
    g = S.GaussianModel(sh_degree=3, device=torch.device(DEV))
    g.load_raw(xyz, np.zeros((P, 1, 3), np.float32), np.zeros((P, 15, 3), np.float32), scaling, rotation, opacity)
    return g


def shell(P=4000, radius=0.04, centre=(0.125, 0.125, 0.125), sigma=0.015, seed=0):
    """Gaussians on a sphere shell whose surface lies inside ONE block of the opacity field's 16^3 block grid (about [0.008, 0.243]^3
    of the +-2 box at 256^3): the block rule truncates a Gaussian at its block's margin, and a surface cut by that truncation is
    a staircase, not a sphere.  Here every Gaussian reaches every voxel of the block; the field at the centre (2.7 sigma from the
    shell) is ~80, far above the isovalue, so there is no inner sheet; it falls to 0.01 about 4.5 sigma outside the shell, at radius
    ~0.107 < 0.117, the distance from the centre to the block's faces."""
    rng = np.random.RandomState(seed)
    d = rng.randn(P, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    xyz = (d * radius + np.array(centre)).astype(np.float32)
    rot = np.tile(np.array([[1.0, 0, 0, 0]], np.float32), (P, 1))
    return model(xyz, rot, np.full((P, 3), np.log(sigma), np.float32), np.full((P, 1), 1.0, np.float32)), np.array(centre, np.float32)


OPT = types.SimpleNamespace(init_density_threshold=0.05)
ZERO = PolyField(np.zeros((4, 3), np.float32), np.zeros(4, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32))


def test_end_to_end_against_the_reference_golden():
    """Centre, scale and threshold to 1e-6 relative.  The normals go through this project's fp32 opacity field, which differs from
    the reference's in the last bits, so a nearest-sample tie can flip: the allowed share of Gaussians whose normal is more than 1
    degree off is 2 * flip_share_ref + 5 / P, flip_share_ref being the reference chain's own sensitivity to a field perturbation of
    the opacity-field test's tolerance (measured and stored by make_normal_init_golden.py)."""
    N = pkg("normal_init")
    gold = np.load(GOLD)
    g = model(gold["xyz"], gold["rotation"], gold["scaling"], gold["opacity"])
    deform = PolyField(*[gold[f"deform/{i}"] for i in range(4)])
    P = g._xyz.shape[0]
    d_xyz, d_rot, d_scl, _ = deform.step(g.get_xyz.detach(), float(gold["t0"]))
    # (the golden's draws are torch.rand of a CPU generator: they go in through `draws`)
    info = N.normal_initialization(g, deform, d_xyz, d_rot, d_scl, opt=OPT, gaussian_ratio=float(gold["gaussian_ratio"]),
                                   draws=torch.tensor(gold["u"], device=DEV), occ_resolution=int(gold["res"]))
    c = g.gaussian_center.cpu().numpy().astype(np.float64)
    assert np.abs(c - gold["center"]).max() <= 1e-6 * np.abs(gold["center"]).max()
    assert abs(float(g.gaussian_scale[0]) - float(gold["scale"][0])) <= 1e-6 * float(gold["scale"][0])
    assert abs(float(g.density_thres_param.detach()) - float(gold["threshold"][0])) <= 1e-6 * float(gold["threshold"][0])
    print("V, F:", info["V"], info["F"], "golden:", int(gold["V"]), int(gold["F"]))
    n = g._normal.detach().cpu().numpy().astype(np.float64)
    cos = (n * gold["normals"].astype(np.float64)).sum(1)
    share = float((cos < np.cos(np.deg2rad(1.0))).mean())
    allowed = 2 * float(gold["flip_share_ref"]) + 5 / P
    print(f"share of normals more than 1 degree off the reference's: {share:.6f} (allowed {allowed:.6f}, "
          f"flip_share_ref {float(gold['flip_share_ref']):.6f})")
    assert share <= allowed


def test_shell_normals_point_one_way_and_the_parameter_stays():
    N = pkg("normal_init")
    g, centre = shell()
    g.training_setup(pkg("scene").OptimizationParams())
    for p in g.parameters():  # non-trivial Adam moments
        p.grad = torch.randn_like(p)
    g.optimizer.step()
    param = g._normal
    st = g.optimizer.state[param]
    m, v = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    gen = torch.Generator(device=DEV).manual_seed(3)
    x0 = g._xyz.detach().clone()
    info = N.normal_initialization(g, ZERO, 0.0, 0.0, 0.0, opt=OPT, gaussian_ratio=1.1, generator=gen)
    assert g._normal is param and g.optimizer.state[param] is st
    assert torch.equal(st["exp_avg"], m) and torch.equal(st["exp_avg_sq"], v) and torch.equal(g._xyz.detach(), x0)
    assert info["F"] > 0 and info["faces"].shape == (info["F"], 3) and info["verts"].shape == (info["V"], 3)
    n = g._normal.detach()
    ln = n.norm(dim=1)
    nz = ln > 0
    assert float(nz.float().mean()) > 0.99
    assert float((ln[nz] - 1).abs().max()) <= 1e-5
    radial = g._xyz.detach() - torch.tensor(centre, device=DEV)
    dots = (n * radial).sum(1)[nz]
    print("dot(normal, radial): min", float(dots.min()), "max", float(dots.max()))
    assert bool((dots > 0).all()) or bool((dots < 0).all())
    assert float(g.density_thres_param) == pytest.approx(0.05, rel=1e-6)
    # the box of a static scene: centre of the shell, scale = largest edge * 1.1 / 2
    x = g._xyz.detach()
    assert torch.allclose(g.gaussian_center, (x.amax(0) + x.amin(0)) / 2, atol=1e-6)
    assert torch.allclose(g.gaussian_scale, (x.amax(0) - x.amin(0)).amax().reshape(1) * 1.1 / 2, rtol=1e-6)


def test_out_dir_files_equal_the_device_tensors(tmp_path):
    N, io = pkg("normal_init"), pkg("ply_io")
    g, _ = shell(P=1500)
    d = torch.full((1500, 3), 0.01, device=DEV)
    info = N.normal_initialization(g, ZERO, d, 0.0, 0.0, opt=OPT, generator=torch.Generator(device=DEV).manual_seed(1),
                                   out_dir=str(tmp_path), occ_resolution=128)
    v, f = io.read_mesh_ply(str(tmp_path / "mesh_init.ply"))
    assert np.array_equal(v, info["verts"].cpu().numpy()) and np.array_equal(f, info["faces"].cpu().numpy())
    p, n = io.read_pointcloud_ply(str(tmp_path / "pointcloud_init.ply"))
    assert np.array_equal(p, (g._xyz.detach() + d).cpu().numpy()) and np.array_equal(n, g._normal.detach().cpu().numpy())


def test_a_field_without_surface_raises():
    N = pkg("normal_init")
    g, _ = shell(P=500)
    with torch.no_grad():
        g._opacity.fill_(-7.0)  # sigmoid = 9e-4: below the field's 0.005 pre-filter and the 0.01 isovalue
    normal = g._normal.detach().clone()
    with pytest.raises(RuntimeError, match=r"isovalue -0\.01.*maximum"):
        N.normal_initialization(g, ZERO, 0.0, 0.0, 0.0, opt=OPT, generator=torch.Generator(device=DEV).manual_seed(1), occ_resolution=64)
    assert torch.equal(g._normal.detach(), normal)


def test_a_surface_without_area_is_reported_one_call_later():
    """Nothing waits for the device inside the chain, so faces that are all degenerate give zero normals there and then; the total
    area travels to the host on its own and the AreaCheck the chain returns (the trainer calls it at the start of the next step)
    raises."""
    N = pkg("normal_init")
    verts = torch.tensor([[0.0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]], device=DEV)
    xyz = torch.rand((64, 3), device=DEV)
    flat = torch.tensor([[0, 1, 2], [1, 1, 2], [2, 0, 1]], dtype=torch.int32, device=DEV)
    normals, _, fidx, idx, total = N.normals_from_surface(xyz, verts, flat, 64, generator=torch.Generator(device=DEV).manual_seed(0))
    assert float(normals.abs().max()) == 0.0 and bool((fidx == -1).all()) and bool((idx == -1).all())
    with pytest.raises(RuntimeError, match="total area of the 3 faces"):
        N.AreaCheck(total, 3)()
    good = torch.tensor([[0, 1, 3]], dtype=torch.int32, device=DEV)
    normals, _, _, _, total = N.normals_from_surface(xyz, verts, good, 64, generator=torch.Generator(device=DEV).manual_seed(0))
    N.AreaCheck(total, 1)()
    assert torch.equal(normals, torch.tensor([[0.0, 0, 1]], device=DEV).expand(64, 3))
    # the chain hands one out, and the trainer's next step() would call it
    g, _ = shell(P=1500)
    info = N.normal_initialization(g, ZERO, 0.0, 0.0, 0.0, opt=OPT, generator=torch.Generator(device=DEV).manual_seed(1), occ_resolution=128)
    info["area_check"]()
