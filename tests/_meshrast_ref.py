"""Plain float64 torch restatement of the mesh rasterizer (dg-mesh_amd/mesh_raster.py, csrc/mesh_raster.hip): brute-force
coverage and depth over every pixel x triangle, perspective-correct barycentrics, interpolate and the antialias rule, with
autograd standing in for every adjoint.  Runs on the CPU (or any device); no HIP.  The differentiable passes take a `dtype`
(default float64; float32 gives a single-precision run of the same arithmetic); rasterize_ids is always float64.

pos (V, 4) clip space, tri (F, 3); screen s = ((x/w + 1) W/2, (y/w + 1) H/2), pixel centres at (px + .5, py + .5)."""
import torch

D = torch.float64


def screen(pos, H, W, dtype=D):
    pos = pos.to(dtype)
    w = pos[:, 3]
    return (pos[:, 0] / w + 1.0) * (0.5 * W), (pos[:, 1] / w + 1.0) * (0.5 * H), pos[:, 2] / w


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _edges_canon(sx, sy, tri, px, py):
    """E_k (F, P) for every face and pixel centre: edge k = (vertices (k+1)%3, (k+2)%3), endpoints in ascending id order, signed as
    in the face's cyclic order.  Faces sharing an edge see exactly negated values."""
    out = []
    for k in range(3):
        a, b = tri[:, (k + 1) % 3], tri[:, (k + 2) % 3]
        swap = a > b
        lo, hi = torch.where(swap, b, a), torch.where(swap, a, b)
        e = _edge(sx[lo][:, None], sy[lo][:, None], sx[hi][:, None], sy[hi][:, None], px[None], py[None])
        out.append(torch.where(swap[:, None], -e, e))
    return out


def face_ok(pos, tri, H, W):
    """The faces the rasterizer keeps: indices in range, every w > 0, finite screen positions, non-zero screen area; and the
    orientation sign of each."""
    V = pos.shape[0]
    tri = tri.long()
    inr = ((tri >= 0) & (tri < V)).all(1)
    t = tri.clamp(0, max(V - 1, 0))
    sx, sy, zw = screen(pos, H, W)
    if V == 0:
        return torch.zeros(tri.shape[0], dtype=torch.bool), torch.ones(tri.shape[0], dtype=D)
    wpos = (pos[:, 3].to(D) > 0)[t].all(1)
    fin = (torch.isfinite(sx) & torch.isfinite(sy) & torch.isfinite(zw))[t].all(1)
    a2 = _edge(sx[t[:, 0]], sy[t[:, 0]], sx[t[:, 1]], sy[t[:, 1]], sx[t[:, 2]], sy[t[:, 2]])
    ok = inr & wpos & fin & (a2 != 0) & torch.isfinite(a2)
    return ok, torch.where(a2 > 0, 1.0, -1.0).to(D)


def rasterize_ids(pos, tri, H, W, x0=0, y0=0, w=None, h=None, tol=1e-4, chunk=1 << 22):
    """Brute force over the pixels of the crop [x0, x0 + w) x [y0, y0 + h) and every face: id (h, w) int64 (face + 1, 0 on
    background), z/w (h, w) of the winner, and `fragile` (h, w) bool: a centre within `tol` pixels of a face's boundary or whose
    two nearest covering depths differ by less than tol x (1 + |z/w|) -- where fp32 and fp64 may disagree."""
    w = W - x0 if w is None else w
    h = H - y0 if h is None else h
    pos, tri = pos.detach().to(D).cpu(), tri.long().cpu()
    ok, o = face_ok(pos, tri, H, W)
    fidx = torch.nonzero(ok).flatten()
    sx, sy, zw = screen(pos, H, W)
    yy, xx = torch.meshgrid(torch.arange(y0, y0 + h, dtype=D), torch.arange(x0, x0 + w, dtype=D), indexing="ij")
    px, py = (xx + 0.5).flatten(), (yy + 0.5).flatten()
    P = px.numel()
    best = torch.full((P,), float("inf"), dtype=D)
    second = torch.full((P,), float("inf"), dtype=D)
    bid = torch.zeros(P, dtype=torch.long)
    fragile = torch.zeros(P, dtype=torch.bool)
    step = max(1, chunk // max(P, 1))
    for c0 in range(0, fidx.numel(), step):
        f = fidx[c0:c0 + step]
        t = tri[f]
        E = _edges_canon(sx, sy, t, px, py)
        oo = o[f][:, None]
        dist = []
        for k in range(3):
            a, b = t[:, (k + 1) % 3], t[:, (k + 2) % 3]
            L = torch.sqrt((sx[b] - sx[a]) ** 2 + (sy[b] - sy[a]) ** 2).clamp_min(1e-300)[:, None]
            dist.append(oo * E[k] / L)
        dmin = torch.minimum(torch.minimum(dist[0], dist[1]), dist[2])
        Ds = E[0] + E[1] + E[2]
        cov = (dmin >= 0) & (Ds != 0)
        fragile |= (dmin.abs() < tol).any(0)
        z = (E[0] * zw[t[:, 0]][:, None] + E[1] * zw[t[:, 1]][:, None] + E[2] * zw[t[:, 2]][:, None]) / torch.where(Ds != 0, Ds, 1.0)
        z = torch.where(cov, z, torch.full_like(z, float("inf")))
        # fold this chunk in: (depth, id) lexicographic minimum, ties to the lower id (faces ascend within and across chunks)
        for r in range(z.shape[0]):
            zr = z[r]
            better = zr < best
            second = torch.where(better, best, torch.minimum(second, zr))
            bid = torch.where(better, f[r] + 1, bid)
            best = torch.where(better, zr, best)
    near_tie = torch.isfinite(second) & ((second - best).abs() < tol * (1 + best.abs()))
    fragile |= near_tie
    return bid.reshape(h, w), torch.where(bid > 0, best, torch.zeros_like(best)).reshape(h, w), fragile.reshape(h, w)


def barycentrics(pos, tri, ids, H, W, x0=0, y0=0, dtype=D):
    """Differentiable in pos: (u, v) (h, w) perspective-correct barycentrics of vertices 0 and 1 of the face `ids` names
    (0: background -> 0), and z/w.  dtype: the precision of the arithmetic (float64, or float32 for a single-precision run)."""
    h, w = ids.shape
    D = dtype
    pos = pos.to(D)
    tri = tri.long()
    sel = ids.flatten() > 0
    f = (ids.flatten()[sel] - 1)
    dev = pos.device
    yy, xx = torch.meshgrid(torch.arange(y0, y0 + h, dtype=D, device=dev), torch.arange(x0, x0 + w, dtype=D, device=dev),
                            indexing="ij")
    px, py = (xx + 0.5).flatten()[sel], (yy + 0.5).flatten()[sel]
    sx, sy, zw = screen(pos, H, W, D)
    t = tri[f]
    E = []
    for k in range(3):
        a, b = t[:, (k + 1) % 3], t[:, (k + 2) % 3]
        E.append(_edge(sx[a], sy[a], sx[b], sy[b], px, py))
    e = [E[k] / pos[t[:, k], 3] for k in range(3)]
    S = e[0] + e[1] + e[2]
    Ds = E[0] + E[1] + E[2]
    z = (E[0] * zw[t[:, 0]] + E[1] * zw[t[:, 1]] + E[2] * zw[t[:, 2]]) / Ds
    out = torch.zeros((h * w, 3), dtype=D, device=dev)
    out = out.index_put((torch.nonzero(sel).flatten(),), torch.stack([e[0] / S, e[1] / S, z], 1))
    return out[:, 0].reshape(h, w), out[:, 1].reshape(h, w), out[:, 2].reshape(h, w)


def interpolate(attr, u, v, ids, tri, dtype=D):
    """out (h, w, C) = u a0 + v a1 + (1 - u - v) a2 on covered pixels, 0 on background (differentiable in attr, u, v)."""
    attr = attr.to(dtype)
    tri = tri.long()
    f = (ids - 1).clamp_min(0)
    t = tri[f]
    a0, a1, a2 = attr[t[..., 0]], attr[t[..., 1]], attr[t[..., 2]]
    out = u[..., None] * a0 + v[..., None] * a1 + (1 - u - v)[..., None] * a2
    return torch.where((ids > 0)[..., None], out, torch.zeros_like(out))


def silhouette_flags(pos, tri, H, W, dtype=D):
    """(F, 3) bool: edge k of face f is a silhouette (one face; more than two; two whose third vertices lie on the same screen side
    or on the edge's line)."""
    tri = tri.long()
    F = tri.shape[0]
    if F == 0:
        return torch.zeros((0, 3), dtype=torch.bool, device=tri.device)
    sx, sy, _ = screen(pos.detach(), H, W, dtype)
    a = torch.stack([tri[:, (k + 1) % 3] for k in range(3)], 1)
    b = torch.stack([tri[:, (k + 2) % 3] for k in range(3)], 1)
    c = tri
    key = torch.minimum(a, b) * (1 << 32) + torch.maximum(a, b)
    uniq, inv, cnt = torch.unique(key.flatten(), return_inverse=True, return_counts=True)
    sumc = torch.zeros(uniq.numel(), dtype=torch.long, device=tri.device).index_add_(0, inv, c.flatten())
    other = (sumc[inv] - c.flatten()).reshape(F, 3).clamp(0, max(pos.shape[0] - 1, 0))
    n = cnt[inv].reshape(F, 3)
    Ec = _edge(sx[a], sy[a], sx[b], sy[b], sx[c], sy[c])
    Eo = _edge(sx[a], sy[a], sx[b], sy[b], sx[other], sy[other])
    opposite = ((Ec > 0) & (Eo < 0)) | ((Ec < 0) & (Eo > 0))
    return (n != 2) | ~opposite


def antialias(color, ids, zw, pos, tri, H, W, dtype=D):
    """The antialias rule on the whole image (ids, zw (H, W); color (H, W, C)), differentiable in color and pos: returns out
    (H, W, C)."""
    D = dtype
    color = color.to(D)
    pos = pos.to(D)
    tri = tri.long()
    sil = silhouette_flags(pos, tri, H, W, D)
    sx, sy, _ = screen(pos, H, W, D)
    dev = pos.device
    yy, xx = torch.meshgrid(torch.arange(H, dtype=D, device=dev), torch.arange(W, dtype=D, device=dev), indexing="ij")
    cx, cy = (xx + 0.5).flatten(), (yy + 0.5).flatten()
    idf, zf = ids.flatten(), zw.flatten().to(D)
    out = color.reshape(H * W, -1).clone()
    cflat = color.reshape(H * W, -1)
    lin = torch.arange(H * W, device=dev).reshape(H, W)
    for vertical in (False, True):
        p = (lin[:-1, :] if vertical else lin[:, :-1]).flatten()
        q = p + (W if vertical else 1)
        ip, iq = idf[p], idf[q]
        qf = (ip == 0) | ((iq != 0) & ((zf[q] < zf[p]) | ((zf[q] == zf[p]) & (iq < ip))))
        diff = ip != iq
        pf, po = torch.where(qf, q, p), torch.where(qf, p, q)
        T = (torch.where(qf, iq, ip) - 1).clamp_min(0)
        hit = torch.zeros_like(diff)
        tval = torch.zeros(p.numel(), dtype=D, device=dev)
        for k in range(3):
            a, b = tri[T, (k + 1) % 3], tri[T, (k + 2) % 3]
            dx, dy = (sx[b] - sx[a]).detach(), (sy[b] - sy[a]).detach()
            steep = dy.abs() >= dx.abs()
            dirok = ~steep if vertical else steep
            ff = _edge(sx[a], sy[a], sx[b], sy[b], cx[pf], cy[pf])
            fo = _edge(sx[a], sy[a], sx[b], sy[b], cx[po], cy[po])
            cross = ((ff > 0) & (fo < 0)) | ((ff < 0) & (fo > 0))
            take = diff & ~hit & dirok & cross & sil[T, k]
            t = ff / torch.where(take, ff - fo, torch.ones_like(ff))
            tval = torch.where(take, t, tval)
            hit = hit | take
        far = hit & (tval.detach() > 0.5)
        near = hit & (tval.detach() < 0.5)
        tgt = torch.where(far, po, pf)
        src = torch.where(far, pf, po)
        alpha = torch.where(far, tval - 0.5, 0.5 - tval)
        m = far | near
        add = alpha[m][:, None] * (cflat[src[m]] - cflat[tgt[m]])
        out = out.index_add(0, tgt[m], add)
    return out.reshape(color.shape)


def render_chain(pos, tri, attr, H, W, ids=None, zw=None, dtype=D):
    """rasterize -> interpolate -> antialias end to end (ids / zw: the discrete part, default from rasterize_ids)."""
    if ids is None:
        ids, zw, _ = rasterize_ids(pos, tri, H, W)
    u, v, z = barycentrics(pos, tri, ids, H, W, dtype=dtype)
    col = interpolate(attr, u, v, ids, tri, dtype)
    return antialias(col, ids, zw if zw is not None else z.detach(), pos, tri, H, W, dtype), ids
