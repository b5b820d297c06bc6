"""Torch restatement of the reference's Gaussian-mesh anchoring (R/scene/gaussian_model_dpsr_dynamic_anchor.py:383-460 prune /
cat surgery, :599-677 average_and_prune / densify_from_face, :745-829 anchor_mesh; R/ = dgmesh/), written the reference's way --
torch.unique / isin / cumsum masks / masked_select -- on the CPU.  The matching decisions use the fp32 distance
(dx*dx + dy*dy) + dz*dz of fp32 centroids ((v0 + v1) + v2) / 3, the definition the device kernels implement; everything after
the decisions runs in `dtype` (float64 for the checks).  The random draws are inputs: (perm_n1, perm_0_1, angle)."""
import math

import torch
import torch.nn.functional as F

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "normal")


def face_geometry32(verts, faces):
    v = verts.float()
    f = faces.long()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cent = ((a + b) + c) / 3.0
    e1, e2 = b - a, c - a
    n = torch.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    ln = torch.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    nrm = torch.where(ln[:, None] > 0, n / torch.where(ln > 0, ln, torch.ones_like(ln))[:, None], torch.zeros_like(n))
    return cent, nrm


def nearest32(q, t, max_d2=math.inf, chunk=2048):
    """Brute force with the kernels' fp32 formula and tie rule: (idx int64, d2 fp32)."""
    q, t = q.float(), t.float()
    idx = torch.full((q.shape[0],), -1, dtype=torch.long, device=q.device)
    d2 = torch.full((q.shape[0],), math.inf, dtype=torch.float32, device=q.device)
    for s in range(0, q.shape[0], chunk):
        qq = q[s:s + chunk]
        if t.shape[0] == 0:
            continue
        dx = t[None, :, 0] - qq[:, None, 0]
        dy = t[None, :, 1] - qq[:, None, 1]
        dz = t[None, :, 2] - qq[:, None, 2]
        d = (dx * dx + dy * dy) + dz * dz
        d = torch.where(torch.isnan(d), torch.full_like(d, math.inf), d)
        m, j = d.min(1)  # (min returns the first index of the minimum)
        ok = m < max_d2
        idx[s:s + chunk] = torch.where(ok, j, torch.full_like(j, -1))
        d2[s:s + chunk] = torch.where(ok, m, torch.full_like(m, math.inf))
    return idx, d2


def axis_angle_to_quaternion(aa):
    ang = torch.norm(aa, p=2, dim=-1, keepdim=True)
    half = ang * 0.5
    small = ang.abs() < 1e-6
    s = torch.where(small, 0.5 - ang * ang / 48, torch.sin(half) / torch.where(small, torch.ones_like(ang), ang))
    return torch.cat([torch.cos(half), aa * s], -1)


def dist3(p):
    """distCUDA2: mean squared distance to the 3 nearest other points (fp64 here)."""
    if p.shape[0] == 0:
        return p.new_zeros(0)
    d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    d.fill_diagonal_(math.inf)
    k = min(3, p.shape[0] - 1)
    if k == 0:
        return torch.full((p.shape[0],), 3.4028234663852886e38, dtype=p.dtype)
    v = d.topk(k, dim=1, largest=False).values
    if k < 3:  # (the kernel keeps FLT_MAX in the empty slots)
        v = torch.cat([v, torch.full((p.shape[0], 3 - k), 3.4028234663852886e38, dtype=p.dtype)], 1)
    return v.mean(1)


def anchor_ref(state, verts, faces, deform, deform_back, t, max_d2, topn, bs, increase_bs, draws, dtype=torch.float64):
    """state: {name: (P, ...) tensor, name + '/m', name + '/v': Adam moments or absent}.  deform / deform_back: callables
    (xyz (N, 3) in `dtype`, t) -> (d_xyz, d_rotation, d_scaling, d_normal).  Returns (new_state, info)."""
    P = state["xyz"].shape[0]
    S = {k: v.to(dtype) for k, v in state.items()}
    xyz32 = state["xyz"].float()
    cent32, nrm32 = face_geometry32(verts, faces)
    d_xyz = deform(S["xyz"], t)[0]
    x = S["xyz"] + d_xyz
    # (matching in fp32: the deformation evaluated in fp32 and added in fp32 like the device's, the fp32 distance formula)
    face_idx, d2 = nearest32(xyz32 + deform(xyz32, t)[0].float(), cent32, max_d2)
    valid = face_idx >= 0
    Fn = cent32.shape[0]
    fi = face_idx[valid]
    uniq, counts = torch.unique(fi, return_counts=True)
    f11, fn1 = uniq[counts == 1], uniq[counts > 1]
    allf = torch.arange(Fn)
    f01 = allf[~(torch.isin(allf, f11) | torch.isin(allf, fn1))]
    vidx = torch.nonzero(valid).squeeze(1)
    m11 = torch.isin(fi, f11)
    g11 = vidx[m11]
    dd = x[g11] - cent32.to(dtype)[fi[m11]]
    loss11 = (dd * dd).sum(1).mean() if g11.numel() else torch.zeros((), dtype=dtype)
    sel = fn1[draws["perm_n1"].long()] if fn1.numel() else fn1
    # n-1: match mask over the VALID Gaussians, first topn in index order
    match = sel.view(-1, 1) == fi.view(1, -1)
    top = match & (torch.cumsum(match.long(), 1) <= topn)
    new_rows = []
    if sel.numel():
        k = top.sum(1)
        members = [vidx[torch.nonzero(top[r]).squeeze(1)] for r in range(sel.numel())]
        rows = torch.cat(members)
        dx, dr, ds, dn = deform(S["xyz"][rows], t)
        seg = torch.repeat_interleave(torch.arange(sel.numel()), k)
        mean = lambda v: torch.zeros((sel.numel(),) + tuple(v.shape[1:]), dtype=dtype).index_add_(0, seg, v) / \
            k.to(dtype).reshape((-1,) + (1,) * (v.dim() - 1))
        m_xyz = mean(S["xyz"][rows] + dx)
        m_s, m_r, m_n = mean(S["scaling"][rows] + ds), mean(S["rotation"][rows] + dr), mean(S["normal"][rows] + dn)
        bx, br, bs_, bn = deform_back(m_xyz, t)
        new_rows.append({"xyz": m_xyz + bx, "scaling": m_s + bs_, "rotation": m_r + br, "normal": F.normalize(m_n + bn, dim=-1),
                         "f_dc": mean(S["f_dc"][rows]), "f_rest": mean(S["f_rest"][rows]), "opacity": mean(S["opacity"][rows])})
        loss_n1 = torch.norm(cent32.to(dtype)[sel] - m_xyz, dim=-1).mean()
    else:
        loss_n1 = torch.zeros((), dtype=dtype)
    # (the reference recomputes the 0-1 mask from the SELECTED n-1 faces (:812): unselected n-1 faces are 0-1 candidates too)
    f01s = allf[~(torch.isin(allf, f11) | torch.isin(allf, sel))]
    sel0 = f01s[draws["perm_0_1"].long()] if f01s.numel() else f01s
    if sel0.numel():
        c0, n0 = cent32.to(dtype)[sel0], nrm32.to(dtype)[sel0]
        Z = c0.shape[0]
        rot = axis_angle_to_quaternion(F.normalize(n0, dim=-1) * (draws["angle"].to(dtype).reshape(Z, 1) * 2 * math.pi))
        scl = torch.log(torch.sqrt(torch.clamp_min(dist3(cent32[sel0].to(dtype)), 1e-7)))[:, None].repeat(1, 3)
        bx, br, bs_, bn = deform_back(c0, t)
        K = state["f_rest"].shape[1]
        new_rows.append({"xyz": c0 + bx, "scaling": scl + bs_, "rotation": rot + br, "normal": F.normalize(n0 + bn, dim=-1),
                         "f_dc": torch.ones((Z, 1, 3), dtype=dtype), "f_rest": torch.zeros((Z, K, 3), dtype=dtype),
                         "opacity": torch.log(torch.full((Z, 1), 0.1, dtype=dtype) / (1 - 0.1))})
    in_sel = torch.zeros(P, dtype=torch.bool)
    if sel.numel():
        in_sel[vidx[match.any(0)]] = True
    keep = valid & ~in_sel
    out = {}
    for n in NAMES:
        out[n] = torch.cat([S[n][keep]] + [r[n] for r in new_rows], 0)
        for mk in ("/m", "/v"):
            if n + mk in S:
                out[n + mk] = torch.cat([S[n + mk][keep]] + [torch.zeros_like(r[n]) for r in new_rows], 0)
    info = {"keep": keep, "loss_1_1": loss11, "loss_n_1": loss_n1, "n11": f11.numel(), "nn1": fn1.numel(), "n01": f01.numel(),
            "sel_n1": sel, "sel_0_1": sel0, "face_of": face_idx}
    return out, info


class PolyField:
    """A deformation field with the reference's four `.step(xyz, time_input)` outputs (d_xyz, d_rotation, d_scaling, d_normal),
    built from adds and multiplies only, so that MLP rounding stays out of the goldens and fp32 results agree bit for bit on any
    device.  consts: (W (4, 3), c_rot (4,), c_scale (3,), c_normal (3,)); W[3] is the time row."""

    def __init__(self, W, c_rot, c_scale, c_normal):
        self.W, self.c = W, (c_rot, c_scale, c_normal)

    def consts(self):
        return (self.W,) + self.c

    def step(self, xyz, t):
        t = torch.as_tensor(t, dtype=xyz.dtype, device=xyz.device).reshape(-1)[:1].reshape(1, 1)
        W = torch.as_tensor(self.W).to(device=xyz.device, dtype=xyz.dtype)
        c = [torch.as_tensor(v).to(device=xyz.device, dtype=xyz.dtype) for v in self.c]
        d_xyz = ((xyz[:, 0:1] * W[0] + xyz[:, 1:2] * W[1]) + xyz[:, 2:3] * W[2]) + t * W[3]
        s = xyz[:, 0:1] + xyz[:, 1:2] * xyz[:, 2:3]
        return d_xyz, s * c[0], s * c[1], (xyz * xyz) * c[2]

    __call__ = step
