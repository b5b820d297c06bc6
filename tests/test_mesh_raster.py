"""The mesh rasterizer (dg-mesh_amd/mesh_raster.py, csrc/mesh_raster.hip): the float64 restatement (_meshrast_ref.py) checked
against geometry on the CPU, and the HIP kernels checked against the restatement on the GPU -- ids, barycentrics, interpolate,
antialias, every adjoint, run-to-run identity, edge cases, a 288^3 DiffMC mesh at 800 x 800, and alignment with the Gaussian
rasterizer's pixel grid."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import _meshrast_ref as R
from conftest import ROOT, pkg

D = torch.float64


def screen_pos(pts, H, W, z=0.5, w=1.0):
    """Clip positions (V, 4) whose screen position is pts (V, 2) (pixels), at depth z/w = z and the given w."""
    pts = torch.as_tensor(pts, dtype=D)
    z = torch.as_tensor(z, dtype=D).expand(pts.shape[0])
    w = torch.as_tensor(w, dtype=D).expand(pts.shape[0])
    x = (pts[:, 0] / (0.5 * W) - 1.0) * w
    y = (pts[:, 1] / (0.5 * H) - 1.0) * w
    return torch.stack([x, y, z * w, w], 1)


def grid_pillow(n, x0, y0, step):
    """A closed mesh: two triangulated (n+1)^2 sheets with vertices at (x0 + i step, y0 + j step), the back sheet at larger depth and
    opposite winding, sharing the boundary vertices."""
    verts, idx = [], {}
    for s in (0, 1):
        for j in range(n + 1):
            for i in range(n + 1):
                border = i in (0, n) or j in (0, n)
                if s == 1 and border:
                    idx[(1, i, j)] = idx[(0, i, j)]
                    continue
                idx[(s, i, j)] = len(verts)
                verts.append((x0 + i * step, y0 + j * step, 0.3 if s == 0 else 0.6))
    faces = []
    for s in (0, 1):
        for j in range(n):
            for i in range(n):
                a, b, c, d = idx[(s, i, j)], idx[(s, i + 1, j)], idx[(s, i + 1, j + 1)], idx[(s, i, j + 1)]
                f1, f2 = (a, b, c), (a, c, d)
                if s == 1:
                    f1, f2 = (a, c, b), (a, d, c)
                faces += [f1, f2]
    v = np.array(verts)
    return v[:, :2], v[:, 2], np.array(faces, np.int64)


def uv_sphere(nu, nv, r=1.0):
    verts = [(0.0, 0.0, r)]
    for i in range(1, nv):
        th = math.pi * i / nv
        for j in range(nu):
            ph = 2 * math.pi * j / nu
            verts.append((r * math.sin(th) * math.cos(ph), r * math.sin(th) * math.sin(ph), r * math.cos(th)))
    verts.append((0.0, 0.0, -r))
    faces = []
    for j in range(nu):
        faces.append((0, 1 + j, 1 + (j + 1) % nu))
    for i in range(nv - 2):
        for j in range(nu):
            a, b = 1 + i * nu + j, 1 + i * nu + (j + 1) % nu
            c, d = a + nu, b + nu
            faces += [(a, c, b), (b, c, d)]
    last = len(verts) - 1
    base = 1 + (nv - 2) * nu
    for j in range(nu):
        faces.append((base + j, last, base + (j + 1) % nu))
    return np.array(verts, np.float64), np.array(faces, np.int64)


def _tilt(a=0.7, b=0.3):
    ca, sa, cb, sb = math.cos(a), math.sin(a), math.cos(b), math.sin(b)
    return np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])


# ---- CPU: the restatement itself --------------------------------------------------------------------------------------------------
def _coverage_sum(pts, H, W):
    pos = screen_pos(pts, H, W).requires_grad_(True)
    tri = torch.tensor([[0, 1, 2]])
    ids, zw, _ = R.rasterize_ids(pos, tri, H, W)
    ones = torch.ones((3, 1), dtype=D)
    u, v, _ = R.barycentrics(pos, tri, ids, H, W)
    m = R.antialias(R.interpolate(ones, u, v, ids, tri), ids, zw, pos, tri, H, W)
    return pos, m.sum()


def _area(p):
    return 0.5 * abs((p[1][0] - p[0][0]) * (p[2][1] - p[0][1]) - (p[1][1] - p[0][1]) * (p[2][0] - p[0][0]))


TRI = [(12.3, 9.7), (81.9, 23.4), (37.15, 70.6)]


def test_antialiased_coverage_of_a_large_triangle_equals_its_area():
    """The rule is exact along every row / column an edge crosses away from the edge's end points; each of the 3 vertices spoils at
    most the two rows and two columns around it by less than a pixel each: |error| < 3 x 4 px^2."""
    H, W = 80, 96
    _, s = _coverage_sum(TRI, H, W)
    area = _area(TRI)
    err = abs(float(s.detach()) - area)
    print(f"coverage sum {float(s.detach()):.4f} vs area {area:.4f}: error {err:.4f} px^2 (bound 12)")
    assert err < 12.0
    assert err < 0.01 * area


def test_coverage_derivative_matches_the_area_derivative():
    H, W = 80, 96
    pos, s = _coverage_sum(TRI, H, W)
    s.backward()
    p = np.array(TRI)
    sign = np.sign((p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[1, 1] - p[0, 1]) * (p[2, 0] - p[0, 0]))
    g = np.zeros((3, 2))
    for k in range(3):  # dA/dp_k = 0.5 sign * perp(p_{k+2} - p_{k+1})
        a, b = p[(k + 1) % 3], p[(k + 2) % 3]
        g[k] = 0.5 * sign * np.array([a[1] - b[1], b[0] - a[0]])
    gx = pos.grad[:, 0].numpy() / (0.5 * W)  # d/d(screen x) = d/d(clip x) / (W / 2) at w = 1
    gy = pos.grad[:, 1].numpy() / (0.5 * H)
    mine = np.stack([gx, gy], 1)
    err = np.abs(mine - g).max() / np.abs(g).max()
    print(f"coverage gradient vs area gradient: {err:.3e} of max")
    assert err < 0.05


def test_axis_aligned_edges_are_exact():
    """A rectangle (two triangles) with edges at fractional positions: every pixel on a side holds its exact area fraction, away
    from the corners -- next to a corner the front centre may belong to the face that does not own the side (the diagonal
    passes between them), and the pair is left alone -- and the total is exact up to the pixels around the four corners."""
    H, W = 40, 48
    x0, x1, y0, y1 = 10.3, 30.8, 5.6, 20.2
    pts = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    pos = screen_pos(pts, H, W)
    tri = torch.tensor([[0, 1, 2], [0, 2, 3]])
    ids, zw, _ = R.rasterize_ids(pos, tri, H, W)
    u, v, _ = R.barycentrics(pos, tri, ids, H, W)
    m = R.antialias(R.interpolate(torch.ones((4, 1), dtype=D), u, v, ids, tri), ids, zw, pos, tri, H, W)[..., 0]
    xs, ys = np.arange(W), np.arange(H)
    cx = np.clip(np.minimum(xs + 1, x1) - np.maximum(xs, x0), 0, 1)
    cy = np.clip(np.minimum(ys + 1, y1) - np.maximum(ys, y0), 0, 1)
    exact = cy[:, None] * cx[None, :]
    corner = np.zeros((H, W), bool)
    for cxp in (int(x0), int(x1)):
        for cyp in (int(y0), int(y1)):
            corner[cyp - 2:cyp + 3, cxp - 2:cxp + 3] = True
    err = np.abs(m.numpy() - exact)
    print(f"axis-aligned: max error off corners {err[~corner].max():.2e}, total {abs(m.sum().item() - exact.sum()):.3e}")
    assert err[~corner].max() < 1e-12
    assert abs(m.sum().item() - exact.sum()) < 4.0


def test_a_centre_on_a_shared_edge_is_covered_by_exactly_one_face():
    """Two faces share an edge through pixel centres (x = 10.5, exactly representable); both cover those centres (inclusive
    edges, exactly negated edge values) and the depth tie-break keeps the lower id."""
    H, W = 24, 24
    pts = [(10.5, 2.0), (10.5, 21.0), (3.2, 11.0), (19.7, 12.0)]
    pos = screen_pos(pts, H, W)
    tri = torch.tensor([[0, 1, 2], [1, 0, 3]])
    sx, sy, _ = R.screen(pos, H, W)
    px, py = torch.tensor([10.5], dtype=D), torch.tensor([7.5], dtype=D)
    E0 = R._edges_canon(sx, sy, tri[:1], px, py)
    E1 = R._edges_canon(sx, sy, tri[1:], px, py)
    assert float(E0[2][0, 0]) == 0.0 and float(E1[2][0, 0]) == -0.0  # the shared edge (vertices 0, 1): exactly negated (zero here)
    ids, _, _ = R.rasterize_ids(pos, tri, H, W)
    col = ids[2:21, 10]
    assert bool((col == 1).all()), col
    # one pixel column to either side belongs to one face each, and the two faces meet without a gap
    assert bool((ids[5:18, 9] == 1).all()) and bool((ids[5:18, 11] == 2).all())


@pytest.mark.parametrize("kind", ["pillow", "sphere"])
def test_no_background_inside_a_closed_mesh(kind):
    H, W = 48, 64
    if kind == "pillow":  # vertices on pixel centres: every edge passes through centres
        xy, z, faces = grid_pillow(6, 8.5, 6.5, 6.0)
        pos = screen_pos(xy, H, W, z=torch.tensor(z))
        inside = np.zeros((H, W), bool)
        inside[6:43, 8:45] = True
    else:
        v, faces = uv_sphere(24, 12, r=1.0)
        v = v @ _tilt()
        xy = v[:, :2] * 18.0 + np.array([32.1, 23.9])
        pos = screen_pos(xy, H, W, z=torch.tensor(0.5 + 0.1 * v[:, 2]))
        yy, xx = np.mgrid[0:H, 0:W]
        inside = (xx + 0.5 - 32.1) ** 2 + (yy + 0.5 - 23.9) ** 2 < (18.0 * math.cos(math.pi / 12) * 0.98) ** 2
    ids, _, _ = R.rasterize_ids(pos, torch.tensor(faces), H, W)
    holes = int(((ids.numpy() == 0) & inside).sum())
    print(f"{kind}: {int(inside.sum())} centres inside the silhouette, {holes} background")
    assert holes == 0


def test_restatement_adjoints_match_central_differences():
    """autograd of the restatement (the reference the GPU adjoints are held to) against central differences in float64, with the
    discrete part (ids, z/w) fixed."""
    H, W = 24, 32
    gen = torch.Generator().manual_seed(3)
    v, faces = uv_sphere(8, 5, r=1.0)
    v = v @ _tilt()  # (seen down its axis, the rings of a UV sphere project onto each other: exact ties)
    xy = v[:, :2] * 9.0 + np.array([15.7, 11.3])
    pos0 = screen_pos(xy, H, W, z=torch.tensor(0.5 + 0.1 * v[:, 2]), w=torch.tensor(1.0 + 0.2 * v[:, 0]))
    tri = torch.tensor(faces)
    attr = torch.rand((pos0.shape[0], 3), generator=gen, dtype=D)
    ids, zw, _ = R.rasterize_ids(pos0, tri, H, W)
    wgt = torch.randn((H, W, 3), generator=gen, dtype=D)

    def L(pos, at):
        u, vv, _ = R.barycentrics(pos, tri, ids, H, W)
        return (R.antialias(R.interpolate(at, u, vv, ids, tri), ids, zw, pos, tri, H, W) * wgt).sum()

    pos = pos0.clone().requires_grad_(True)
    at = attr.clone().requires_grad_(True)
    L(pos, at).backward()
    h = 1e-6
    rng = np.random.RandomState(0)

    def fd_pos(i, c, hh):
        a, b = pos0.clone(), pos0.clone()
        a[i, c] += hh
        b[i, c] -= hh
        return float(L(a, attr) - L(b, attr)) / (2 * hh)

    checked = 0
    for _ in range(40):
        i, c = int(rng.randint(pos0.shape[0])), int(rng.choice([0, 1, 3]))
        fd, fd2 = fd_pos(i, c, h), fd_pos(i, c, h / 2)
        if abs(fd - fd2) > 1e-4 * max(1.0, abs(fd)):  # a discrete event (a silhouette / crossing flip) inside the step: skip
            continue
        assert abs(fd - float(pos.grad[i, c])) <= 1e-5 * max(1.0, abs(fd)), (i, c, fd, float(pos.grad[i, c]))
        checked += 1
    print(f"{checked} position coordinates checked against central differences")
    assert checked >= 20
    for _ in range(6):
        i, c = int(rng.randint(attr.shape[0])), int(rng.randint(3))
        a, b = attr.clone(), attr.clone()
        a[i, c] += h
        b[i, c] -= h
        fd = float(L(pos0, a) - L(pos0, b)) / (2 * h)
        assert abs(fd - float(at.grad[i, c])) <= 1e-6 * max(1.0, abs(fd))


def test_api_refuses_cpu_tensors_and_wrong_dtypes_without_gpu():
    MR = pkg("mesh_raster")
    pos = torch.zeros((1, 3, 4))
    tri = torch.zeros((1, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        MR.rasterize(None, pos, tri, (8, 8))
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        MR.antialias(torch.zeros((1, 8, 8, 1)), torch.zeros((1, 8, 8, 4)), pos, tri)


def test_mesh_losses_option_is_validated_without_gpu():
    T = pkg("trainer")
    with pytest.raises(ValueError, match="mesh_source='diffmc'"):
        T.MeshPhase(None, None, None, n_verts=8, device="cpu", mesh_losses="render")
    with pytest.raises(ValueError, match="mesh_losses"):
        T.MeshPhase(None, None, None, n_verts=8, device="cpu", mesh_source="diffmc", mesh_losses="nvdiffrast")
    assert T.MeshPhase(None, None, None, n_verts=8, device="cpu").mesh_losses == "stand_in"


# ---- GPU: kernels against the restatement -------------------------------------------------------------------------------------
def _mr():
    return pkg("mesh_raster")


def random_scene(F, H, W, seed, soup=True):
    """A sphere (closed; w varies) plus `F` random small triangles in front of and behind it, as clip positions."""
    rng = np.random.RandomState(seed)
    v, faces = uv_sphere(16, 9, r=1.0)
    v = v @ _tilt(0.5 + 0.1 * seed, 0.2)
    c = np.array([W * (0.4 + 0.2 * rng.rand()), H * (0.4 + 0.2 * rng.rand())])
    r = 0.3 * min(H, W)
    xy = [v[:, :2] * r + c]
    z = [0.5 + 0.2 * v[:, 2]]
    w = [1.0 + 0.3 * v[:, 0]]
    tris = [faces]
    n0 = len(v)
    if soup and F > 0:
        cen = rng.rand(F, 1, 2) * np.array([W, H])
        pts = cen + rng.randn(F, 3, 2) * rng.uniform(0.5, 6.0, (F, 1, 1))
        xy.append(pts.reshape(-1, 2))
        z.append(np.repeat(rng.uniform(0.2, 0.8, F), 3) + 0.01 * rng.randn(3 * F))
        w.append(rng.uniform(0.5, 2.0, 3 * F))
        tris.append(n0 + np.arange(3 * F).reshape(F, 3))
    pos = screen_pos(np.concatenate(xy), H, W, z=torch.tensor(np.concatenate(z)), w=torch.tensor(np.concatenate(w)))
    return pos.float(), torch.tensor(np.concatenate(tris)).int()


def _gpu_chain(pos, tri, attr, H, W):
    MR = _mr()
    p = pos.cuda().unsqueeze(0).contiguous()
    t = tri.cuda().contiguous()
    a = attr.cuda().contiguous()
    rast, _ = MR.rasterize(None, p, t, (H, W))
    col, _ = MR.interpolate(a, rast, t)
    out = MR.antialias(col, rast, p, t)
    return rast, col, out


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,F,seed", [(48, 64, 600, 0), (131, 97, 1800, 1), (800, 800, 1500, 2)])
def test_gpu_matches_restatement(H, W, F, seed):
    pos, tri = random_scene(F, H, W, seed)
    attr = torch.rand((pos.shape[0], 3), generator=torch.Generator().manual_seed(seed))
    rast, col, out = _gpu_chain(pos, tri, attr, H, W)
    rast_c, col_c, out_c = rast[0].cpu(), col[0].cpu(), out[0].cpu()
    # the 800 x 800 case: a crop around the sphere's edge
    x0, y0, w, h = (0, 0, W, H) if H * W < 40000 else (int(W * 0.1), int(H * 0.3), 160, 120)
    ids, zw, fragile = R.rasterize_ids(pos.double(), tri, H, W, x0, y0, w, h)
    gid = rast_c[y0:y0 + h, x0:x0 + w, 3].long()
    mism = (gid != ids)
    n_bad, n_frag = int((mism & ~fragile).sum()), int(fragile.sum())
    print(f"{H}x{W} F={tri.shape[0]}: {int(mism.sum())} id mismatches, all within {n_frag} fragile centres; {n_bad} elsewhere")
    assert n_bad == 0
    assert int(mism.sum()) <= max(4, h * w // 1000)
    ok = ~mism & (ids > 0) & ~fragile
    u, v, z = R.barycentrics(pos.double(), tri, ids, H, W, x0, y0)
    g = rast_c[y0:y0 + h, x0:x0 + w].double()
    eu, ev = (g[..., 0] - u)[ok].abs().max(), (g[..., 1] - v)[ok].abs().max()
    ez = ((g[..., 2] - z)[ok].abs() / (1 + z[ok].abs())).max()
    print(f"  u, v, z/w errors {float(eu):.2e} {float(ev):.2e} {float(ez):.2e}")
    assert eu < 5e-4 and ev < 5e-4 and ez < 1e-5
    assert bool((rast_c[..., 3] == 0).eq((rast_c[..., :3] == 0).all(-1)).logical_or(rast_c[..., 3] > 0).all())
    # interpolate from the GPU's own rast: fp32 rounding only
    gi = rast_c[..., 3].long()
    ref_col = R.interpolate(attr.double(), rast_c[..., 0].double(), rast_c[..., 1].double(), gi, tri)
    assert float((col_c.double() - ref_col).abs().max()) < 1e-5
    # antialias from the GPU's ids / z/w: the same discrete decisions except within rounding of a crossing or a silhouette test
    ref_out = R.antialias(col_c.double(), gi, rast_c[..., 2].double(), pos.double(), tri, H, W)
    d = (out_c.double() - ref_out).abs().max(-1).values
    n_aa = int((d > 1e-4).sum())
    print(f"  antialias: max error {float(d.max()):.2e}, {n_aa} pixels above 1e-4")
    assert n_aa <= max(2, H * W // 20000)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,seed", [(48, 64, 3), (97, 131, 4)])
def test_gpu_adjoints_match_fp64_autograd(H, W, seed):
    MR = _mr()
    pos, tri = random_scene(300, H, W, seed)
    gen = torch.Generator().manual_seed(seed)
    attr = torch.rand((pos.shape[0], 3), generator=gen)
    wgt = torch.randn((H, W, 3), generator=gen)
    p = pos.cuda().unsqueeze(0).requires_grad_(True)
    a = attr.cuda().requires_grad_(True)
    t = tri.cuda()
    rast, _ = MR.rasterize(None, p, t, (H, W))
    col, _ = MR.interpolate(a, rast, t)
    out = MR.antialias(col, rast, p, t)
    (out[0] * wgt.cuda()).sum().backward()
    gid, gz = rast[0, ..., 3].long().cpu(), rast[0, ..., 2].detach().double().cpu()
    # restatement on the GPU's discrete part
    pr = pos.double().requires_grad_(True)
    ar = attr.double().requires_grad_(True)
    u, v, _ = R.barycentrics(pr, tri, gid, H, W)
    ref = R.antialias(R.interpolate(ar, u, v, gid, tri), gid, gz, pr, tri, H, W)
    (ref * wgt.double()).sum().backward()
    ea = float((a.grad.cpu().double() - ar.grad).abs().max() / ar.grad.abs().max())
    gp, rp = p.grad[0].cpu().double(), pr.grad
    ep = float((gp - rp).abs().max() / rp.abs().max())
    print(f"{H}x{W}: dattr {ea:.2e}, dpos {ep:.2e} of max")
    assert ea < 1e-5
    assert ep < 1e-3
    assert float(gp[:, 2].abs().max()) == 0.0
    # each stage's adjoint alone: rasterize (u, v), antialias (colour)
    p2 = pos.cuda().unsqueeze(0).requires_grad_(True)
    rast2, _ = MR.rasterize(None, p2, t, (H, W))
    wr = torch.randn((H, W, 2), generator=gen)
    (rast2[0, ..., :2] * wr.cuda()).sum().backward()
    pr2 = pos.double().requires_grad_(True)
    u2, v2, _ = R.barycentrics(pr2, tri, gid, H, W)
    (u2 * wr[..., 0].double() + v2 * wr[..., 1].double()).sum().backward()
    er = float((p2.grad[0].cpu().double() - pr2.grad).abs().max() / pr2.grad.abs().max())
    print(f"  rasterize dpos {er:.2e} of max")
    assert er < 1e-3
    c = torch.rand((1, H, W, 2), generator=gen).cuda().requires_grad_(True)
    o = MR.antialias(c, rast.detach(), p.detach(), t)
    wc = torch.randn((H, W, 2), generator=gen)
    (o[0] * wc.cuda()).sum().backward()
    cr = c.detach()[0].cpu().double().requires_grad_(True)
    (R.antialias(cr, gid, gz, pos.double(), tri, H, W) * wc.double()).sum().backward()
    ec = float((c.grad[0].cpu().double() - cr.grad).abs().max())
    assert ec < 1e-4, ec  # (t from fp32 screen positions)


@pytest.mark.gpu
def test_gpu_forward_is_bit_reproducible():
    H, W = 131, 97
    pos, tri = random_scene(1500, H, W, 7)
    attr = torch.rand((pos.shape[0], 4), generator=torch.Generator().manual_seed(7))
    a = _gpu_chain(pos, tri, attr, H, W)
    b = _gpu_chain(pos, tri, attr, H, W)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---- GPU: edge cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_empty_and_single_vertex_meshes():
    MR = _mr()
    H, W = 16, 24
    color = torch.rand((1, H, W, 2), device="cuda")
    for V, F in ((3, 0), (1, 4)):
        p = torch.rand((1, V, 4), device="cuda") + 0.5
        t = torch.zeros((F, 3), dtype=torch.int32, device="cuda")
        rast, _ = MR.rasterize(None, p, t, (H, W))
        assert int(torch.count_nonzero(rast)) == 0
        col, _ = MR.interpolate(torch.rand((V, 3), device="cuda"), rast, t)
        assert int(torch.count_nonzero(col)) == 0
        assert torch.equal(MR.antialias(color, rast, p, t), color)


@pytest.mark.gpu
def test_gpu_repeated_degenerate_and_behind_camera_faces():
    H, W = 40, 40
    pts = [(5.2, 5.1), (33.7, 8.3), (12.4, 34.6), (20.0, 20.0), (30.0, 30.0), (25.0, 25.0)]
    pos = screen_pos(pts, H, W)
    # vertex 6: behind the camera (w < 0)
    pos = torch.cat([pos, torch.tensor([[0.1, 0.1, -0.2, -0.5]], dtype=D)]).float()
    tri = torch.tensor([[3, 4, 5],   # collinear: zero area
                        [0, 1, 2], [0, 1, 2],   # repeated: the lower id wins every centre
                        [2, 1, 0],   # the same face, opposite winding, later id
                        [0, 1, 6]], dtype=torch.int32)  # a vertex at w <= 0: dropped
    rast, _, _ = _gpu_chain(pos, tri, torch.ones((7, 1)), H, W)
    gid = rast[0, ..., 3].long().cpu()
    ids, _, fragile = R.rasterize_ids(pos.double(), tri, H, W)
    assert torch.equal(gid[~fragile], ids[~fragile])
    assert set(gid.unique().tolist()) == {0, 2}


@pytest.mark.gpu
def test_gpu_full_screen_quad_leaves_no_background():
    """Two triangles larger than the screen (the workgroup path: their boxes hold every centre)."""
    H, W = 300, 421
    pos = torch.tensor([[-1.5, -1.5, 0.5, 1.0], [1.5, -1.5, 0.5, 1.0], [1.5, 1.5, 0.5, 1.0], [-1.5, 1.5, 0.5, 1.0]])
    tri = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    rast, _, out = _gpu_chain(pos, tri, torch.ones((4, 1)), H, W)
    gid = rast[0, ..., 3].long().cpu()
    assert int((gid == 0).sum()) == 0
    ids, _, fragile = R.rasterize_ids(pos.double(), tri, H, W)
    assert torch.equal(gid[~fragile], ids[~fragile])
    # no silhouette inside the screen (the diagonal is shared, its third vertices on opposite sides): the mask stays 1
    assert float((out[0, ..., 0].cpu() - 1.0).abs().max()) < 1e-6


@pytest.mark.gpu
def test_gpu_100k_faces_on_one_pixel():
    H, W = 32, 32
    F = 100000
    rng = np.random.RandomState(5)
    base = np.array([(10.2, 10.1), (11.3, 10.4), (10.6, 11.2)])
    pts = (base[None] + 0.05 * rng.randn(F, 3, 2)).reshape(-1, 2)
    z = np.repeat(rng.randint(0, 50, F) / 100.0 + 0.2, 3)  # 50 depth levels, ~2000 faces each
    pos = screen_pos(pts, H, W, z=torch.tensor(z)).float()
    tri = torch.arange(3 * F, dtype=torch.int32).reshape(F, 3)
    r1, _, o1 = _gpu_chain(pos, tri, torch.ones((3 * F, 1)), H, W)
    r2, _, o2 = _gpu_chain(pos, tri, torch.ones((3 * F, 1)), H, W)
    assert torch.equal(r1, r2) and torch.equal(o1, o2)
    gid = int(r1[0, 10, 10, 3])
    zf = pos[:, 2].reshape(F, 3)[:, 0].double().numpy()
    sx, sy, _ = R.screen(pos.double(), H, W)
    E = R._edges_canon(sx, sy, tri.long(), torch.tensor([10.5], dtype=D), torch.tensor([10.5], dtype=D))
    ok, o = R.face_ok(pos.double(), tri, H, W)
    cov = ok & ((o[:, None] * torch.stack([e[:, 0:1] for e in E], 0)[..., 0].T) >= 0).all(1)
    cand = np.nonzero(cov.numpy())[0]
    near = zf[cand].min()
    print(f"100k faces on one pixel: {len(cand)} cover the centre, winner {gid - 1} at z {zf[gid - 1]:.4f} (nearest level {near:.4f})")
    # the winner is on the nearest level (within a level, the fp32-interpolated z/w of the faces differ in the last bits)
    assert len(cand) > 50000 and gid - 1 in set(cand.tolist()) and zf[gid - 1] == near
    assert abs(float(r1[0, 10, 10, 2]) - near) < 1e-6


@pytest.mark.gpu
def test_gpu_input_checks():
    MR = _mr()
    p = torch.rand((1, 3, 4), device="cuda")
    t = torch.zeros((1, 3), dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="2\\^24"):
        MR.rasterize(None, p, torch.zeros((1 << 24, 3), dtype=torch.int32, device="cuda"), (8, 8))
    with pytest.raises(RuntimeError, match="float32"):
        MR.rasterize(None, p.double(), t, (8, 8))
    with pytest.raises(RuntimeError, match="int32"):
        MR.rasterize(None, p, t.long(), (8, 8))
    with pytest.raises(RuntimeError, match="contiguous"):
        MR.rasterize(None, torch.rand((1, 4, 3), device="cuda").transpose(1, 2), t, (8, 8))
    with pytest.raises(RuntimeError, match="batch size 1"):
        MR.rasterize(None, torch.rand((2, 3, 4), device="cuda"), t, (8, 8))
    rast, _ = MR.rasterize(None, p, t, (8, 8))
    with pytest.raises(RuntimeError, match="contiguous"):
        MR.interpolate(torch.rand((3, 4), device="cuda")[:, ::2], rast, t)
    with pytest.raises(RuntimeError, match="float32"):
        MR.antialias(torch.rand((1, 8, 8, 1), device="cuda").half(), rast, p, t)


# ---- GPU: at scale ------------------------------------------------------------------------------------------------------------------
def _torch_raster_fp64(pos, tri, H, W):
    """An independent float64 raster on the device: every triangle's covered centres (plain edge functions, inclusive), then a
    scatter-reduce amin of depth per pixel and of the id among the pixel's nearest -> ids (H, W) (0: background)."""
    p = pos.double()
    w = p[:, 3]
    sx, sy, zw = (p[:, 0] / w + 1) * (0.5 * W), (p[:, 1] / w + 1) * (0.5 * H), p[:, 2] / w
    t = tri.long()
    X, Y, Z = sx[t], sy[t], zw[t]
    a2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    keep = (w[t] > 0).all(1) & (a2 != 0)
    x0 = torch.ceil(X.min(1).values - 0.5).clamp(0, W).long()
    x1 = torch.floor(X.max(1).values - 0.5).clamp(-1, W - 1).long()
    y0 = torch.ceil(Y.min(1).values - 0.5).clamp(0, H).long()
    y1 = torch.floor(Y.max(1).values - 0.5).clamp(-1, H - 1).long()
    bw, bh = (x1 - x0 + 1).clamp_min(0), (y1 - y0 + 1).clamp_min(0)
    n = torch.where(keep, bw * bh, torch.zeros_like(bw))
    f = torch.repeat_interleave(torch.arange(t.shape[0], device=t.device), n)
    start = torch.cumsum(n, 0) - n
    j = torch.arange(f.numel(), device=t.device) - start[f]
    px = x0[f] + j % bw[f]
    py = y0[f] + j // bw[f]
    cx, cy = px.double() + 0.5, py.double() + 0.5
    o = torch.sign(a2)[f]
    E = []
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        E.append((X[f, b] - X[f, a]) * (cy - Y[f, a]) - (Y[f, b] - Y[f, a]) * (cx - X[f, a]))
    cov = (o * E[0] >= 0) & (o * E[1] >= 0) & (o * E[2] >= 0)
    z = (E[0] * Z[f, 0] + E[1] * Z[f, 1] + E[2] * Z[f, 2]) / (E[0] + E[1] + E[2])
    pix = (py * W + px)[cov]
    z, f = z[cov], f[cov]
    zmin = torch.full((H * W,), float("inf"), dtype=D, device=t.device).scatter_reduce(0, pix, z, "amin")
    at = z == zmin[pix]
    big = torch.iinfo(torch.long).max
    imin = torch.full((H * W,), big, dtype=torch.long, device=t.device).scatter_reduce(0, pix[at], f[at], "amin")
    return torch.where(imin == big, 0, imin + 1).reshape(H, W)


@pytest.mark.gpu
def test_gpu_ids_on_the_288_diffmc_mesh_at_800():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_marching_cubes import dpsr_phi_288
    from scipy import ndimage
    syn, S, M = pkg("synthetic"), pkg("scene"), pkg("marching_cubes")
    MR = _mr()
    verts, faces = M.DiffMC()(dpsr_phi_288())
    verts = (verts * 2.0 - 1.0) * 1.1
    cam = S.TorchCamera(syn.make_camera(800, 800, radius=3.5), "cuda")
    with torch.no_grad():
        pos = MR.clip_positions(cam, verts)
        rast, _ = MR.rasterize(None, pos, faces, (800, 800))
    gid = rast[0, ..., 3].long()
    ref = _torch_raster_fp64(pos[0], faces, 800, 800)
    mism = int((gid != ref).sum())
    cov = int((ref > 0).sum())
    print(f"288^3 DiffMC mesh: F={faces.shape[0]}, {cov} covered pixels, {mism} id mismatches vs fp64 (bound {cov // 500})")
    assert faces.shape[0] > 100000 and cov > 10000
    assert mism <= cov // 500
    mask = (gid > 0).cpu().numpy()
    holes = int((ndimage.binary_fill_holes(mask) & ~mask).sum())
    print(f"  silhouette interior holes: {holes}")
    assert holes == 0


# ---- GPU: alignment with the Gaussian rasterizer ----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_clip_positions_land_on_the_gaussian_pixels(syn):
    import conftest
    import gpu_util
    S = pkg("scene")
    MR = _mr()
    W, H = 160, 120
    a = conftest.raster_args(syn, 64, W, H, seed=3)
    f = gpu_util.hip_forward(a)
    m2 = torch.tensor(f["means2D"], dtype=D)
    cam = S.TorchCamera(syn.make_camera(W, H), "cuda")
    assert np.array_equal(cam.full_proj_transform.cpu().numpy(), a["projmatrix"])
    pts = torch.tensor(a["means3D"], device="cuda")
    pos = MR.clip_positions(cam, pts)[0].double().cpu()
    sx, sy, _ = R.screen(pos, H, W)
    vis = f["radii"] > 0
    d = torch.stack([sx - 0.5, sy - 0.5], 1)[torch.tensor(vis)] - m2[torch.tensor(vis)]
    print(f"mesh screen - 0.5 vs ndc2Pix: max {float(d.abs().max()):.2e} px over {int(vis.sum())} points")
    assert float(d.abs().max()) < 1e-3
    # a small triangle around a projected point covers the pixel whose centre is nearest to it
    i = int(np.nonzero(vis)[0][0])
    cx, cy = float(m2[i, 0]), float(m2[i, 1])
    tri_pts = screen_pos([(cx + 0.5 - 0.8, cy + 0.5 - 0.6), (cx + 0.5 + 0.8, cy + 0.5 - 0.6), (cx + 0.5, cy + 0.5 + 0.9)], H, W)
    rast, _ = MR.rasterize(None, tri_pts.float().cuda().unsqueeze(0), torch.tensor([[0, 1, 2]], dtype=torch.int32, device="cuda"),
                           (H, W))
    assert int(rast[0, int(round(cy)), int(round(cx)), 3]) == 1


# ---- GPU: end to end: fitting a silhouette ------------------------------------------------------------------------------------------
class _Cam:
    def __init__(self, cam):
        self.full_proj_transform = torch.tensor(cam.full_proj_transform, device="cuda")
        self.image_width, self.image_height = cam.image_width, cam.image_height


@pytest.mark.gpu
def test_gpu_mask_loss_fits_an_offset_sphere(syn):
    """Masks of a sphere from 4 views; the same sphere offset by a few pixels is moved back by Adam on the mask loss alone (the only
    geometry gradient is the antialias one): loss and IoU must improve clearly."""
    MR = _mr()
    v, faces = uv_sphere(32, 16, r=0.6)
    base = torch.tensor(v, dtype=torch.float32, device="cuda")
    tri = torch.tensor(faces, dtype=torch.int32, device="cuda")
    cams = [_Cam(syn.make_camera(96, 96, azimuth=0.4 + 1.5 * k, elevation=0.2 + 0.15 * k)) for k in range(4)]
    with torch.no_grad():
        gts = [MR.render_mask(None, base, tri, c) for c in cams]
    off = torch.tensor([0.09, -0.07, 0.08], device="cuda", requires_grad=True)
    opt = torch.optim.Adam([off], lr=0.01)

    def evaluate():
        loss, inter, union = 0.0, 0, 0
        for c, g in zip(cams, gts):
            m = MR.render_mask(None, base + off, tri, c)
            loss = loss + (m - g).abs().mean()
            a, b = m.detach() > 0.5, g > 0.5
            inter, union = inter + int((a & b).sum()), union + int((a | b).sum())
        return loss, inter / union

    with torch.no_grad():
        l0, iou0 = evaluate()
    for _ in range(40):
        opt.zero_grad()
        loss, _ = evaluate()
        loss.backward()
        assert bool(torch.isfinite(off.grad).all()) and float(off.grad.abs().max()) > 0
        opt.step()
    with torch.no_grad():
        l1, iou1 = evaluate()
    print(f"mask fit: loss {float(l0):.4f} -> {float(l1):.4f}, IoU {iou0:.4f} -> {iou1:.4f}, offset {off.detach().cpu().tolist()}")
    assert float(l1) < 0.5 * float(l0)
    assert iou1 > iou0 + 0.03
