"""Plain numpy statement of dg-mesh_amd/mesh_clean.py (csrc/mesh_clean.hip): labels, the component table, the selection and the
order-preserving compaction.  Integers, comparisons and copies only; the one float expression (the squared box diagonal) is written
in float32 in the kernel's order.  This project's own reference: nothing here comes from igl, trimesh or pymeshlab."""
import numpy as np

F32 = np.float32


def valid_faces(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    inr = ((f >= 0) & (f < V)).all(1)
    return inr & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def labels(faces, V):
    """labels[v] = the smallest vertex index of v's component (union-find by minimum with path halving)."""
    parent = list(range(V))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    f = np.asarray(faces, np.int64).reshape(-1, 3)
    for a, b, c in f[valid_faces(f, V)].tolist():
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    return np.array([find(v) for v in range(V)], np.int32).reshape(V)


def float_key(x):
    """Order-preserving uint32 of float32 bits (-0 < +0; a NaN beyond the infinity of its sign)."""
    u = np.ascontiguousarray(x, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def key_float(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(F32)


def table(verts, faces, lab):
    """Rows ordered by label: label, faces (valid), verts, bbox_min, bbox_max."""
    verts, V = np.ascontiguousarray(verts, F32).reshape(-1, 3), len(lab)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    roots = np.unique(lab).astype(np.int32)
    nf = np.bincount(lab[f[valid_faces(f, V), 0]], minlength=max(V, 1))[roots].astype(np.int32)
    nv = np.bincount(lab, minlength=max(V, 1))[roots].astype(np.int32)
    key = float_key(verts)
    order = np.argsort(lab, kind="stable")
    starts = np.searchsorted(lab[order], roots)
    mn = key_float(np.minimum.reduceat(key[order], starts, axis=0)) if V else np.zeros((0, 3), F32)
    mx = key_float(np.maximum.reduceat(key[order], starts, axis=0)) if V else np.zeros((0, 3), F32)
    return {"label": roots, "faces": nf, "verts": nv, "bbox_min": mn.reshape(-1, 3), "bbox_max": mx.reshape(-1, 3)}


def diag2(mn, mx):
    d = (np.asarray(mx, F32) - np.asarray(mn, F32)).astype(F32)
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(F32) + d[..., 2] * d[..., 2]).astype(F32)


def keep_mask(verts, faces, lab, largest=False, min_faces=0, min_diameter_frac=0.0):
    V, f = len(lab), np.asarray(faces, np.int64).reshape(-1, 3)
    keep = valid_faces(f, V)
    if not keep.any():
        return keep.astype(np.uint8)
    t = table(verts, faces, lab)
    ok = np.ones(len(t["label"]), bool)
    if largest:
        ok &= np.arange(len(ok)) == np.argmax(t["faces"])  # (argmax: the first maximum, rows are ordered by label)
    if min_faces > 0:
        ok &= t["faces"] >= min_faces
    if min_diameter_frac > 0:
        whole = diag2(key_float(float_key(t["bbox_min"]).min(0)), key_float(float_key(t["bbox_max"]).max(0)))
        frac = F32(min_diameter_frac)
        ok &= diag2(t["bbox_min"], t["bbox_max"]) >= F32(F32(frac * frac) * whole)
    row = np.searchsorted(t["label"], lab[np.where(keep, f[:, 0], 0)])
    return (keep & ok[row]).astype(np.uint8)


def compact(verts, faces, keep):
    """verts', faces' (re-indexed), vert_index, face_index: the survivors in their old order."""
    verts = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    fi = np.flatnonzero(np.asarray(keep) != 0).astype(np.int32)
    used = np.zeros(len(verts), bool)
    used[f[fi].reshape(-1)] = True
    vi = np.flatnonzero(used).astype(np.int32)
    new = np.cumsum(used) - 1
    return verts[vi], new[f[fi]].astype(np.int32).reshape(-1, 3), vi, fi


def clean(verts, faces, **criteria):
    V = len(np.asarray(verts).reshape(-1, 3))
    return compact(verts, faces, keep_mask(verts, faces, labels(faces, V), **criteria))
