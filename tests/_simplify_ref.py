"""Plain numpy statement of dg-mesh_amd/mesh_simplify.py (csrc/mesh_simplify.hip): quadric vertex clustering on a uniform grid.
The cell arithmetic is float32 in the kernel's order, the placement float64 from the float32 inputs with the sums taken per cluster
in ascending face order (np.add.at applies its operands one after another, in index order).  The final compaction is
_meshclean_ref.compact.  This project's own reference: nothing here comes from pymeshlab, trimesh or Open3D."""
import numpy as np

import _meshclean_ref as MC

F32, F64 = np.float32, np.float64
MAX_DIM = 1 << 20
GRID_RANGE = (2, 1024)
MAX_COUNT_PASSES = 10


def _mesh(verts, faces):
    return np.ascontiguousarray(verts, F32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)


def valid_faces(verts, faces):
    """Indices in [0, V) and pairwise different, all nine coordinates finite."""
    verts, faces = _mesh(verts, faces)
    ok = MC.valid_faces(faces, len(verts))
    fin = np.isfinite(verts).all(1) if len(verts) else np.zeros(0, bool)
    idx = np.where(ok[:, None], faces, 0).astype(np.int64)
    return ok & (fin[idx].all(1) if len(verts) else False)


def box(verts, faces):
    """(o, hi) float32 over the vertices of the valid faces, ordered by their bits; None without a valid face."""
    verts, faces = _mesh(verts, faces)
    ok = valid_faces(verts, faces)
    if not ok.any():
        return None
    key = MC.float_key(verts[np.unique(faces[ok])])
    return MC.key_float(key.min(0)), MC.key_float(key.max(0))


def grid_cell(o, hi, grid):
    with np.errstate(all="ignore"):
        h = F32(np.max((hi - o).astype(F32)) / F32(grid))
    return h if h > 0 and np.isfinite(h) else F32(1.0)


def grid_dims(o, hi, h):
    with np.errstate(all="ignore"):
        q = np.ceil((hi - o).astype(F32) / F32(h))
    if not (q <= MAX_DIM).all():
        raise ValueError("more than 2^20 cells along an axis")
    return np.maximum(q, 1).astype(np.int64)


def cell_index(verts, o, h, n):
    """(V, 3) int64 = min(n - 1, floor((x - o) / h)) in float32."""
    with np.errstate(all="ignore"):
        q = np.floor((verts - o[None]).astype(F32) / F32(h))
    q = np.where(np.isfinite(q), q, 0)
    return np.minimum(np.maximum(q, 0).astype(np.int64), n[None] - 1)


def cluster(verts, faces, h):
    """-> dict: ok (F,) valid faces, rep (V,) int32 the representative of every used vertex (-1: unused), idx (V, 3) the cells,
    o, n; rep_faces (F, 3) int32 (-1 rows for invalid faces), keep (F,) uint8 = valid, not null, not duplicate."""
    verts, faces = _mesh(verts, faces)
    V, F = len(verts), len(faces)
    ok = valid_faces(verts, faces)
    out = {"ok": ok, "rep": np.full(V, -1, np.int32), "rep_faces": np.full((F, 3), -1, np.int32), "keep": np.zeros(F, np.uint8),
           "o": None, "n": None, "idx": np.zeros((V, 3), np.int64), "h": F32(h)}
    if not ok.any():
        return out
    o, hi = box(verts, faces)
    n = grid_dims(o, hi, h)
    used = np.zeros(V, bool)
    used[faces[ok].reshape(-1)] = True
    idx = cell_index(verts, o, F32(h), n)
    key = (idx[:, 2] * n[1] + idx[:, 1]) * n[0] + idx[:, 0]
    uv = np.flatnonzero(used)
    _, first, inv = np.unique(key[uv], return_index=True, return_inverse=True)  # (first occurrence = the smallest index: uv ascends)
    rep = np.full(V, -1, np.int32)
    rep[uv] = uv[first][inv]
    rf = np.full((F, 3), -1, np.int32)
    rf[ok] = rep[faces[ok]]
    keep = ok & (rf[:, 0] != rf[:, 1]) & (rf[:, 1] != rf[:, 2]) & (rf[:, 0] != rf[:, 2])
    cand = np.flatnonzero(keep)
    if len(cand):
        _, firsts = np.unique(np.sort(rf[cand], 1), axis=0, return_index=True)  # (the first of equal rows: the smallest face index)
        keep[:] = False
        keep[cand[firsts]] = True
    out.update(rep=rep, rep_faces=rf, keep=keep.astype(np.uint8), o=o, n=n, idx=idx)
    return out


def instances(c):
    """(cluster, face) pairs in ascending face order: every valid face once per distinct cluster of its corners."""
    f = np.flatnonzero(c["ok"])
    rf = c["rep_faces"][f]
    parts = [(rf[:, 0], f), (rf[:, 1][rf[:, 1] != rf[:, 0]], f[rf[:, 1] != rf[:, 0]])]
    third = (rf[:, 2] != rf[:, 0]) & (rf[:, 2] != rf[:, 1])
    parts.append((rf[:, 2][third], f[third]))
    r, ff = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    order = np.argsort(ff, kind="stable")
    return r[order].astype(np.int64), ff[order].astype(np.int64)


def place(verts, faces, c, regularization=1e-3):
    """(V, 3) float32: the new position in every representative's row, the old position elsewhere."""
    verts, faces = _mesh(verts, faces)
    V = len(verts)
    placed = verts.copy()
    if c["o"] is None:
        return placed
    r, f = instances(c)
    h = F64(c["h"])
    centre = c["o"].astype(F64)[None] + (c["idx"].astype(F64) + 0.5) * h  # (V, 3): a representative's row is its cell's centre
    cc = centre[r]
    p = verts.astype(F64)[faces[f].astype(np.int64)]  # (I, 3 corners, 3)
    p0, p1, p2 = p[:, 0], p[:, 1], p[:, 2]
    e1, e2 = p1 - p0, p2 - p0
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    q = p0 - cc
    d = -((n[:, 0] * q[:, 0] + n[:, 1] * q[:, 1]) + n[:, 2] * q[:, 2])
    g = ((p0 + p1) + p2) / 3.0 - cc
    A, b, G, cnt = np.zeros((V, 3, 3)), np.zeros((V, 3)), np.zeros((V, 3)), np.zeros(V, np.int64)
    np.add.at(A, r, n[:, :, None] * n[:, None, :])
    np.add.at(b, r, n * d[:, None])
    np.add.at(G, r, g)
    np.add.at(cnt, r, 1)
    reps = np.flatnonzero(cnt > 0)
    xh = G[reps] / cnt[reps][:, None].astype(F64)
    mu = F64(regularization) * ((A[reps, 0, 0] + A[reps, 1, 1]) + A[reps, 2, 2])
    x = xh.copy()
    s = mu > 0
    if s.any():
        M = A[reps][s] + mu[s][:, None, None] * np.eye(3)[None]
        x[s] = np.linalg.solve(M, (mu[s][:, None] * xh[s] - b[reps][s])[:, :, None])[:, :, 0]
    x = np.clip(x, -h, h)
    placed[reps] = (centre[reps] + x).astype(F32)
    return placed


def count(verts, faces, h):
    c = cluster(verts, faces, h)
    fi = np.flatnonzero(c["keep"])
    return len(np.unique(c["rep_faces"][fi])), len(fi)


def bisect(count_at, target):
    lo, hi = GRID_RANGE
    best, tried = None, []
    while lo <= hi and len(tried) < MAX_COUNT_PASSES:
        mid = (lo + hi) // 2
        tried.append(mid)
        if count_at(mid) <= target:
            best, lo = mid, mid + 1
        else:
            hi = mid - 1
    return best, tried


def simplify(verts, faces, cell=None, grid=None, target_faces=None, regularization=1e-3):
    """-> dict: verts (V', 3) float32, faces (F', 3) int32, vert_index, face_index, vert_map (V,) int32, cell, grid, grids_tried,
    lists (the length of every cluster's face list)."""
    verts, faces = _mesh(verts, faces)
    assert sum(a is not None for a in (cell, grid, target_faces)) == 1
    V = len(verts)
    bx = box(verts, faces)
    tried = []
    if bx is None:
        return {"verts": np.zeros((0, 3), F32), "faces": np.zeros((0, 3), np.int32), "vert_index": np.zeros(0, np.int32),
                "face_index": np.zeros(0, np.int32), "vert_map": np.full(V, -1, np.int32), "cell": None, "grid": grid, "grids_tried": tried,
                "lists": np.zeros(0, np.int64)}
    if target_faces is not None:
        grid, tried = bisect(lambda g: count(verts, faces, grid_cell(*bx, g))[1], target_faces)
        if grid is None:
            raise ValueError("target_faces is not reached even at the coarsest grid")
    h = F32(cell) if cell is not None else grid_cell(*bx, grid)
    c = cluster(verts, faces, h)
    placed = place(verts, faces, c, regularization)
    v, f, vi, fi = MC.compact(placed, c["rep_faces"], c["keep"])
    new = np.full(V, -1, np.int32)
    new[vi] = np.arange(len(vi), dtype=np.int32)
    vert_map = np.where(c["rep"] >= 0, new[np.maximum(c["rep"], 0)], -1).astype(np.int32)
    lists = np.bincount(instances(c)[0], minlength=V)
    return {"verts": v, "faces": f, "vert_index": vi, "face_index": fi, "vert_map": vert_map, "cell": float(h), "grid": grid,
            "grids_tried": tried, "lists": lists[lists > 0]}


# ---- hand-made meshes --------------------------------------------------------------------------------------------------------------
def subdivided_cube(k):
    """The surface of [0, 1]^3 with every side cut into k x k squares of two triangles: 6 k^2 + 2 vertices, 12 k^2 faces."""
    t = np.arange(k + 1) / k
    pts, index = [], {}

    def vid(p):
        key = tuple(int(round(x * k)) for x in p)
        if key not in index:
            index[key] = len(pts)
            pts.append(p)
        return index[key]

    faces = []
    for axis in range(3):
        for side in (0.0, 1.0):
            u, w = [a for a in range(3) if a != axis]
            for i in range(k):
                for j in range(k):
                    quad = []
                    for du, dw in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0.0, 0.0, 0.0]
                        p[axis], p[u], p[w] = side, t[i + du], t[j + dw]
                        quad.append(vid(tuple(p)))
                    if side == 0.0:
                        quad = quad[::-1]
                    faces += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    return np.array(pts, F32), np.array(faces, np.int32)


def icosphere(level):
    """A unit icosphere: 20 * 4^level faces."""
    phi = (1 + 5 ** 0.5) / 2
    v = [(-1, phi, 0), (1, phi, 0), (-1, -phi, 0), (1, -phi, 0), (0, -1, phi), (0, 1, phi), (0, -1, -phi), (0, 1, -phi),
         (phi, 0, -1), (phi, 0, 1), (-phi, 0, -1), (-phi, 0, 1)]
    v = [np.array(p, F64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v, F32), np.array(f, np.int32)
