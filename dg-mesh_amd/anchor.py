"""Gaussian-mesh anchoring (GaussianModelDPSRDynamicAnchor.anchor_mesh, R/scene/gaussian_model_dpsr_dynamic_anchor.py:553-829,
called from R/train.py:286-304; R/ = the reference's dgmesh/) on top of libdgmesh_hip.

Every Gaussian, deformed to time t, is matched to its nearest face centroid of the current mesh.  Gaussians farther than the search
bound are pruned; faces chosen by exactly one Gaussian (1-1) give the distance loss; of the faces chosen by several (n-1) a random
batch is collapsed into one Gaussian each (the mean of their first `topn` members in deformed space, mapped back with deform_back);
a random batch of the faces nobody chose (0-1) receives a new Gaussian at its centroid.

The reference does the face geometry with trimesh on the host, the matching with pytorch3d.knn_points (a P x F brute force) and the
bookkeeping with torch.unique / isin / cumsum.  Here (csrc/anchor.hip):
  face_geometry -> dgm_anchor_face_geometry, nearest -> dgm_anchor_nn (exact, bit-reproducible, grid-accelerated for a finite
  bound), classification -> dgm_anchor_classify;
the surgery reuses the densify gather (dgm_densify_decide with a keep mask + dgm_densify_apply, densify.py).  plan_anchor reads
back four integers once (the class sizes); apply_anchor reads back the survivor count once.

The bound quirk is kept: knn_points returns SQUARED distances and the reference compares them with the LINEAR radius
gaussian_scale * search_radius, so a Gaussian is valid iff d2 < gaussian_scale * search_radius (fp32).
Deviations:
  * an empty 1-1 or n-1 set contributes 0 to the loss (the reference's mean of an empty tensor is NaN);
  * topn > 2 averages min(count, topn) members (the reference's .view(-1, topn, ...) fails on faces with fewer members; with the
    shipped topn = 2 every n-1 face has at least two, and both rules agree);
  * a deformation network with three outputs (DeformModel) contributes a zero normal delta.
Kept as the reference does it: the 0-1 mask is rebuilt from the n-1 faces of the random batch (R/...:812), so the n-1 faces left
out of the batch are 0-1 candidates too (randperm over n_0_1 + n_n_1 - batch).
No CPU fallback: every function raises on CPU tensors.
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F_

from . import _lib
from . import densify as _D

GROUPS = _D.GROUPS
ATTR = _D.ATTR


def _need_cuda(name, *ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError(f"anchor.{name} needs CUDA/HIP tensors (dg-mesh_amd has no CPU path)")


def face_geometry(verts, faces):
    """trimesh's triangles_center and face_normals on the device: centroids (F, 3), unit normals (F, 3) (zero for a degenerate
    face).  A face with an index outside [0, V) gets a NaN centroid and a zero normal."""
    _need_cuda("face_geometry", verts, faces)
    v = verts.detach().contiguous().float()
    f = faces.detach().contiguous().to(torch.int32)
    V, F = v.shape[0], f.shape[0]
    cent = torch.empty((F, 3), dtype=torch.float32, device=v.device)
    nrm = torch.empty((F, 3), dtype=torch.float32, device=v.device)
    with _lib.device_guard(v.device):
        _lib.check(_lib.lib().dgm_anchor_face_geometry(V, F, _lib.vp(v), _lib.vp(f), _lib.vp(cent), _lib.vp(nrm), _lib.stream_ptr()))
    return cent, nrm


def _nearest_raw(queries, targets, max_d2):
    _need_cuda("nearest", queries, targets)
    q = queries.detach().contiguous().float()
    t = targets.detach().contiguous().float()
    Nq, Nt = q.shape[0], t.shape[0]
    L = _lib.lib()
    idx = torch.empty(Nq, dtype=torch.int32, device=q.device)
    d2 = torch.empty(Nq, dtype=torch.float32, device=q.device)
    scratch = None
    if not math.isinf(max_d2):
        scratch = torch.empty(int(L.dgm_anchor_nn_scratch_bytes(Nq, Nt)), dtype=torch.uint8, device=q.device)
    with _lib.device_guard(q.device):
        _lib.check(L.dgm_anchor_nn(Nq, Nt, _lib.vp(q), _lib.vp(t), float(max_d2), _lib.vp(scratch), _lib.vp(idx), _lib.vp(d2), _lib.stream_ptr()))
    return idx, d2


def nearest(queries, targets, max_d2=float("inf")):
    """Exact nearest target of every query: (idx (Nq,) int64, d2 (Nq,) fp32), d2 = (dx*dx + dy*dy) + dz*dz in fp32, ties to the
    smaller target index; idx = -1 and d2 = +inf where no target has d2 < max_d2.  max_d2 = inf is knn_points(K=1)."""
    idx, d2 = _nearest_raw(queries, targets, max_d2)
    return idx.long(), d2


def classify(face_of, F):
    """Per-face bookkeeping of the matching (face_of (P,) int32, -1 = invalid): counts, offsets, lists, members, rank (see
    include/dgmesh_hip.h, dgm_anchor_classify) and the host tuple (n_1_1, n_n_1, n_0_1, n_valid) -- the one read-back."""
    _need_cuda("classify", face_of)
    fo = face_of.contiguous().to(torch.int32)
    P = fo.shape[0]
    dev = fo.device
    L = _lib.lib()
    out = {k: torch.empty(F, dtype=torch.int32, device=dev) for k in ("counts", "offsets", "lists")}
    out.update({k: torch.empty(P, dtype=torch.int32, device=dev) for k in ("members", "rank")})
    totals = torch.empty(4, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(L.dgm_anchor_classify_scratch_bytes(P, F)), dtype=torch.uint8, device=dev)
    with _lib.device_guard(dev):
        _lib.check(L.dgm_anchor_classify(P, F, _lib.vp(fo), _lib.vp(scratch), _lib.vp(out["counts"]), _lib.vp(out["offsets"]), _lib.vp(out["lists"]),
                                         _lib.vp(out["members"]), _lib.vp(out["rank"]), _lib.vp(totals), _lib.stream_ptr()))
    out["totals"] = tuple(int(v) for v in totals.tolist())
    return out


def _time(t, N, dev):
    return torch.as_tensor(t, dtype=torch.float32, device=dev).reshape(1, 1).expand(N, -1)


def _step4(model, xyz, t):
    """model.step(xyz, t) as the reference's four outputs (d_xyz, d_rotation, d_scaling, d_normal); no rows, no call."""
    N = xyz.shape[0]
    if N == 0:
        z = xyz.new_zeros
        return z((0, 3)), z((0, 4)), z((0, 3)), z((0, 3))
    out = model.step(xyz, _time(t, N, xyz.device))
    d_normal = out[3] if len(out) > 3 else torch.zeros_like(out[0])
    return out[0], out[1], out[2], d_normal


def axis_angle_to_quaternion(axis_angle):
    """pytorch3d.transforms.axis_angle_to_quaternion (real part first)."""
    angles = torch.norm(axis_angle, p=2, dim=-1, keepdim=True)
    half = angles * 0.5
    small = angles.abs() < 1e-6
    safe = torch.where(small, torch.ones_like(angles), angles)
    s = torch.where(small, 0.5 - (angles * angles) / 48, torch.sin(half) / safe)
    return torch.cat([torch.cos(half), axis_angle * s], dim=-1)


def _inverse_sigmoid(x):
    return torch.log(x / (1 - x))


def plan_anchor(g, verts, faces, deform, deform_back, t, search_radius=0.0005, topn=2, bs=256, increase_bs=1024, generator=None,
                draws=None):
    """Everything of anchor_mesh that only reads state: the matching, the classification, anchor_loss_1_1 (with its gradient to
    `deform` through d_xyz), the constant anchor_loss_n_1, the keep mask and the appended rows of every parameter group.
    `generator`: the device generator of the two permutations and the angles (drawn in the reference's order: randperm n-1,
    randperm 0-1, randn); `draws`: {"perm_n1", "perm_0_1", "angle"} injected instead (a test feeds the reference's own).
    Returns a dict for apply_anchor; plan["loss"] = anchor_loss_1_1 + anchor_loss_n_1."""
    xyz = g._xyz
    _need_cuda("plan_anchor", xyz, verts, faces)
    dev = xyz.device
    P = xyz.shape[0]
    scale = float(torch.as_tensor(g.gaussian_scale).reshape(-1)[0])
    max_d2 = float(np.float32(np.float32(scale) * np.float32(search_radius)))  # (fp32 tensor * python float, as in the reference)
    # 1. deform (with grad: anchor_loss_1_1 reaches the deformation network), 2. face geometry, 3. nearest face
    d_xyz = _step4(deform, xyz.detach(), t)[0]
    x = g.get_xyz + d_xyz
    cent, nrm = face_geometry(verts, faces)
    F = cent.shape[0]
    face_of, _ = _nearest_raw(x.detach(), cent, max_d2)
    # 4. classify
    c = classify(face_of, F)
    n11, nn1, n01, nvalid = c["totals"]
    counts, offsets, lists, members = c["counts"].long(), c["offsets"].long(), c["lists"].long(), c["members"].long()
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    # 5. 1-1 loss: the one Gaussian of each 1-1 face, in index order (the reference's boolean mask)
    if n11 > 0:
        f11 = lists[:n11]
        g11, order = torch.sort(members[offsets[f11]])
        dd = x[g11] - cent[f11[order]]
        loss11 = ((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]).mean()
    else:
        loss11 = zero
    # 6. n-1 faces: randperm -> first topn members each -> averaged in deformed space -> deform_back
    if draws is not None:
        perm1 = torch.as_tensor(draws["perm_n1"], device=dev).long()
    else:
        perm1 = torch.randperm(nn1, device=dev, generator=generator)[:bs]
    sel = lists[n11:n11 + nn1][perm1]
    X = int(sel.shape[0])
    sel_face = torch.zeros(F + 1, dtype=torch.bool, device=dev)
    rows = {}
    with torch.no_grad():
        if X > 0:
            ar = torch.arange(topn, device=dev)
            pos = offsets[sel][:, None] + ar[None, :]
            if topn <= 2:  # every n-1 face has >= 2 members: topn each, as the reference's view(-1, topn, ...)
                k = torch.full((X,), topn, dtype=torch.long, device=dev)
                mrows = members[pos.reshape(-1)]
            else:
                k = torch.clamp(counts[sel], max=topn)
                mrows = members[pos[ar[None, :] < k[:, None]]]
            uniform = topn <= 2
            seg = None if uniform else torch.repeat_interleave(torch.arange(X, device=dev), k)

            def mean(v):
                if uniform:
                    return v.reshape((X, topn) + tuple(v.shape[1:])).mean(1)
                s = torch.zeros((X,) + tuple(v.shape[1:]), dtype=v.dtype, device=dev).index_add_(0, seg, v)
                return s / k.reshape((X,) + (1,) * (v.dim() - 1)).to(v.dtype)

            dx, dr, ds, dn = _step4(deform, xyz.detach()[mrows], t)
            m_xyz = mean(xyz.detach()[mrows] + dx)
            m_scaling = mean(g._scaling.detach()[mrows] + ds)
            m_rotation = mean(g._rotation.detach()[mrows] + dr)
            m_normal = mean(g._normal.detach()[mrows] + dn)
            bx, br, bsc, bn = _step4(deform_back, m_xyz, t)
            rows["n_1"] = {"xyz": m_xyz + bx, "scaling": m_scaling + bsc, "rotation": m_rotation + br,
                           "normal": F_.normalize(m_normal + bn, p=2, dim=-1),
                           "f_dc": mean(g._features_dc.detach()[mrows]), "f_rest": mean(g._features_rest.detach()[mrows]),
                           "opacity": mean(g._opacity.detach()[mrows])}
            loss_n1 = torch.norm(cent[sel] - m_xyz, dim=-1).mean()
            sel_face[sel] = True
        else:
            loss_n1 = zero
        # 7. 0-1 faces: new Gaussians at a random batch of centroids.  The reference rebuilds the 0-1 mask from the SELECTED n-1
        #    faces (R/...:812), so the n-1 faces outside the batch are candidates too, in ascending face order with the 0-1 ones.
        n0c = n01 + nn1 - X
        if X == nn1:
            cand = lists[n11 + nn1:]
        else:  # (a compaction without a host read-back: slot n0c takes the faces that are not candidates)
            m = (counts == 0) | ((counts > 1) & ~sel_face[:F])
            at = torch.where(m, torch.cumsum(m, 0) - 1, torch.full_like(counts, n0c))
            cand = torch.empty(n0c + 1, dtype=torch.long, device=dev).scatter_(0, at, torch.arange(F, device=dev))[:n0c]
        if draws is not None:
            perm0 = torch.as_tensor(draws["perm_0_1"], device=dev).long()
        else:
            perm0 = torch.randperm(n0c, device=dev, generator=generator)[:increase_bs]
        f0 = cand[perm0]
        Z = int(f0.shape[0])
        if Z > 0:
            from .knn import distCUDA2
            c0, nm0 = cent[f0], nrm[f0]
            if draws is not None:
                angle = torch.as_tensor(draws["angle"], dtype=torch.float32, device=dev).reshape(Z, 1)
            else:
                angle = torch.randn((Z, 1), device=dev, generator=generator)
            rot = axis_angle_to_quaternion(F_.normalize(nm0, p=2, dim=-1) * (angle * 2 * np.pi))
            dist2 = torch.clamp_min(distCUDA2(c0), 0.0000001)
            scl = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
            bx, br, bsc, bn = _step4(deform_back, c0, t)
            K = g._features_rest.shape[1]
            rows["0_1"] = {"xyz": c0 + bx, "scaling": scl + bsc, "rotation": rot + br, "normal": F_.normalize(nm0 + bn, p=2, dim=-1),
                           "f_dc": torch.ones((Z, 1, 3), dtype=torch.float32, device=dev),
                           "f_rest": torch.zeros((Z, K, 3), dtype=torch.float32, device=dev),
                           "opacity": _inverse_sigmoid(0.1 * torch.ones((Z, 1), dtype=torch.float32, device=dev))}
        # keep: valid and not a member of a selected n-1 face
        fo = face_of.long()
        keep = (fo >= 0) & ~sel_face[torch.where(fo >= 0, fo, torch.full_like(fo, F))]
    new_rows = {k: torch.cat([r[k] for r in rows.values()], 0) if rows else None for k in GROUPS}
    return {"keep": keep, "rows": new_rows, "n_new": X + Z, "loss": loss11 + loss_n1, "loss_1_1": loss11, "loss_n_1": loss_n1,
            "face_of": face_of, "n_faces": F, "old_P": P, "counts": (n11, nn1, n01, nvalid), "perm_n1": perm1, "perm_0_1": perm0,
            "selected_n1": sel, "selected_0_1": f0}


@torch.no_grad()
def apply_anchor(g, plan):
    """The surgery of a plan: prune every Gaussian outside plan["keep"] (parameters and both Adam moments through the densify
    gather), append the plan's rows with zero moments, re-seat the Parameters in the optimizer and zero the densification
    statistics at the new size (densification_postfix).  Returns the numbers the reference prints."""
    P = g._xyz.shape[0]
    if P > 0:
        scratch, K, _, _ = _D._decide(g, P, keep_mask=plan["keep"])
        _D._apply(g, P, scratch, K, 0, 0, None)
    if plan["n_new"] > 0:
        _append(g, plan["rows"])
    Pn = g._xyz.shape[0]
    dev = g._xyz.device
    g.xyz_gradient_accum = torch.zeros((Pn, 1), device=dev)
    g.denom = torch.zeros((Pn, 1), device=dev)
    g.max_radii2D = torch.zeros((Pn,), device=dev)
    n11, nn1, n01, nvalid = plan["counts"]
    F = plan["n_faces"]
    return {"old_P": plan["old_P"], "new_P": Pn, "faces": F, "hit_rate_1_1": n11 / F if F else 0.0,
            "invalid_ratio": (plan["old_P"] - nvalid) / plan["old_P"] if plan["old_P"] else 0.0}


def _append(g, rows):
    """cat_tensors_to_optimizer (R/...:421-443): new rows behind the old ones, zero Adam moments for them."""
    opt = g.optimizer
    by_name = {grp["name"]: grp for grp in opt.param_groups} if opt is not None else {}
    for name in GROUPS:
        old = getattr(g, ATTR[name])
        ext = rows[name].to(old.dtype).reshape((-1,) + tuple(old.shape[1:]))
        p_new = nn.Parameter(torch.cat((old.detach(), ext), 0).contiguous().requires_grad_(True))
        if name in by_name:
            grp = by_name[name]
            st = opt.state.pop(grp["params"][0], None)
            grp["params"][0] = p_new
            if st is not None:
                if "exp_avg" in st:
                    st["exp_avg"] = torch.cat((st["exp_avg"], torch.zeros_like(ext)), 0).contiguous()
                    st["exp_avg_sq"] = torch.cat((st["exp_avg_sq"], torch.zeros_like(ext)), 0).contiguous()
                opt.state[p_new] = st
        setattr(g, ATTR[name], p_new)


def anchor_mesh(g, verts, faces, deform, deform_back, t, search_radius=0.0005, topn=2, bs=256, increase_bs=1024, generator=None):
    """anchor_mesh (R/...:745-829): plan, apply, return anchor_loss = anchor_loss_1_1 + anchor_loss_n_1."""
    plan = plan_anchor(g, verts, faces, deform, deform_back, t, search_radius, topn, bs, increase_bs, generator=generator)
    apply_anchor(g, plan)
    return plan["loss"]
