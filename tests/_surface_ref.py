"""Plain numpy statement of dg-mesh_amd/csrc/surface.hip: the closest point on a triangle mesh, the barycentric
interpolation and the correspondence palette, op for op in the order the kernel file's header writes down.  closest32 is what the kernel
is held to bit for bit; closest64 is the same statement in float64 and qualifies it (tests/test_surface_host.py).  Dense over the faces,
chunked over the queries by 256, as _anchor_ref.nearest32 is."""
import numpy as np

# fp32 statement against float64 in units of error_unit(): twice the ratios measured on torus_input() (tests/test_surface_host.py)
K_MIN, K_CHOSEN = 2 * 2.33, 2 * 0.71


def torus(nu, nv, R=1.0, r=0.4, dtype=np.float32):
    """A torus around z with nu x nv vertices and 2 nu nv faces: (verts (V, 3), faces (F, 3) int32)."""
    u = np.arange(nu) * (2 * np.pi / nu)
    v = np.arange(nv) * (2 * np.pi / nv)
    U, W = np.meshgrid(u, v, indexing="ij")
    verts = np.stack([(R + r * np.cos(W)) * np.cos(U), (R + r * np.cos(W)) * np.sin(U), r * np.sin(W)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a = (i * nv + j).ravel()
    b = (((i + 1) % nu) * nv + j).ravel()
    c = (((i + 1) % nu) * nv + (j + 1) % nv).ravel()
    d = (i * nv + (j + 1) % nv).ravel()
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)
    return verts.astype(dtype), faces


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def face_ok(verts, faces, dtype=np.float32):
    """The candidates: indices in [0, V) and a positive, finite normal length in `dtype`."""
    V = len(verts)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < V)).all(1)
    g = np.where(ok[:, None], f, 0)
    v = np.asarray(verts, dtype).reshape(-1, 3)
    if V == 0:
        return np.zeros(len(f), bool)
    a, b, c = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        return ok & (ln > 0) & (ln < np.inf)


def pair_vw(p, a, b, c):
    """The pair arithmetic on broadcastable (..., 3) arrays of one dtype: (v, w, dist2)."""
    one, zero = p.dtype.type(1), p.dtype.type(0)
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        ap, bp, cp = p - a, p - b, p - c
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        den = one / ((va + vb) + vc)
        v, w = vb * den, vc * den                                     # 7. interior
        m = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)           # 6. edge BC
        wbc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        v, w = np.where(m, one - wbc, v), np.where(m, wbc, w)
        m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)                         # 5. edge AC
        v, w = np.where(m, zero, v), np.where(m, d2 / (d2 - d6), w)
        m = (d6 >= 0) & (d5 <= d6)                                    # 4. vertex C
        v, w = np.where(m, zero, v), np.where(m, one, w)
        m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)                         # 3. edge AB
        v, w = np.where(m, d1 / (d1 - d3), v), np.where(m, zero, w)
        m = (d3 >= 0) & (d4 <= d3)                                    # 2. vertex B
        v, w = np.where(m, one, v), np.where(m, zero, w)
        m = (d1 <= 0) & (d2 <= 0)                                     # 1. vertex A
        v, w = np.where(m, zero, v), np.where(m, zero, w)
        q = (a + ab * v[..., None]) + ac * w[..., None]
        e = p - q
        return v, w, _dot(e, e)


def pair_d2(points, verts, faces, dtype, chunk=256):
    """dist2 of every (query, face) pair in `dtype`, (N, F); inf where the face is no candidate or dist2 is NaN."""
    p = np.asarray(points, dtype).reshape(-1, 3)
    v = np.asarray(verts, dtype).reshape(-1, 3)
    ok = face_ok(verts, faces, dtype)
    f = np.where(ok[:, None], np.asarray(faces).astype(np.int64).reshape(-1, 3), 0)
    out = np.full((len(p), len(f)), np.inf, dtype)
    if len(f) == 0 or len(v) == 0:
        return out
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    for s in range(0, len(p), chunk):
        d = pair_vw(p[s:s + chunk, None, :], a, b, c)[2]
        out[s:s + chunk] = np.where(ok[None, :] & ~np.isnan(d), d, np.inf)
    return out


def _closest(points, verts, faces, max_d2, dtype):
    p = np.asarray(points, dtype).reshape(-1, 3)
    N = len(p)
    face = np.full(N, -1, np.int32)
    d2 = np.full(N, np.inf, dtype)
    bary = np.zeros((N, 3), dtype)
    F = len(np.asarray(faces).reshape(-1, 3))
    if N == 0 or F == 0 or len(verts) == 0:
        return face, d2, bary
    D = pair_d2(p, verts, faces, dtype)
    j = D.argmin(1)  # (the first index of the minimum: ties to the smaller face)
    m = D[np.arange(N), j]
    found = m < dtype(max_d2)
    v = np.asarray(verts, dtype).reshape(-1, 3)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)[j[found]]
    vv, ww, dd = pair_vw(p[found], v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
    assert np.array_equal(dd, m[found])
    face[found] = j[found]
    d2[found] = m[found]
    bary[found] = np.stack([(dtype(1) - vv) - ww, vv, ww], 1)
    return face, d2, bary


def closest32(points, verts, faces, max_d2=np.inf):
    """(face int32, d2 fp32, bary (N, 3) fp32): the kernel's answer, bit for bit."""
    return _closest(points, verts, faces, max_d2, np.float32)


def closest64(points, verts, faces, max_d2=np.inf):
    """The same statement in float64 (on the float32 inputs)."""
    return _closest(points, verts, faces, max_d2, np.float64)


def interp32(attr, faces, face, bary, fill=np.nan):
    attr = np.asarray(attr, np.float32)
    attr = attr.reshape(len(attr), -1)
    V, F = len(attr), len(faces)
    face = np.asarray(face).astype(np.int64)
    bary = np.asarray(bary, np.float32).reshape(-1, 3)
    out = np.full((len(face), attr.shape[1]), np.float32(fill), np.float32)
    ok = (face >= 0) & (face < F)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)[np.where(ok, face, 0)] if F else np.zeros((len(face), 3), np.int64)
    ok &= ((f >= 0) & (f < V)).all(1)
    f, b = f[ok], bary[ok]
    with np.errstate(all="ignore"):
        out[ok] = (attr[f[:, 0]] * b[:, 0:1] + attr[f[:, 1]] * b[:, 1:2]) + attr[f[:, 2]] * b[:, 2:3]
    return out


def palette32(xyz, center, scale, mode="rgb", cells=8):
    x = np.asarray(xyz, np.float32).reshape(-1, 3)
    c = np.asarray(center, np.float32).reshape(1, 3)
    s = np.float32(np.asarray(scale, np.float32).reshape(-1)[0])
    with np.errstate(all="ignore"):
        t = ((x - c) / s) * np.float32(0.5) + np.float32(0.5)
        lost = np.isnan(t).any(1)
        u = np.minimum(np.maximum(np.where(np.isnan(t), np.float32(0), t), np.float32(0)), np.float32(1))
        k = np.floor(u * np.float32(cells)).astype(np.int64).sum(1)
    shade = np.where((k & 1) == 1, np.float32(0.55), np.float32(1)) if mode == "checker" else np.ones(len(x), np.float32)
    out = (u * shade[:, None]).astype(np.float32)
    out[lost] = np.array([1, 0, 1], np.float32)
    return out


def torus_input(seed=0):
    """The qualification input: torus(40, 20) (V 800, F 1600) and 4200 queries -- 3000 uniform in the box, 300 exactly on vertices, 300 on
    edge midpoints, 300 on face centroids, 300 centroids + 1e-3 noise (all float32)."""
    verts, faces = torus(40, 20)
    rng = np.random.RandomState(seed)
    lo, hi = verts.min(0) - 0.2, verts.max(0) + 0.2
    box = rng.uniform(lo, hi, (3000, 3))
    on_v = verts[rng.randint(0, len(verts), 300)]
    fe = faces[rng.randint(0, len(faces), 300)]
    k = rng.randint(0, 3, 300)
    mid = (verts[fe[np.arange(300), k]] + verts[fe[np.arange(300), (k + 1) % 3]]) * np.float32(0.5)
    fc = faces[rng.randint(0, len(faces), 300)]
    cen = (verts[fc[:, 0]] + verts[fc[:, 1]] + verts[fc[:, 2]]) / np.float32(3)
    fn = faces[rng.randint(0, len(faces), 300)]
    near = (verts[fn[:, 0]] + verts[fn[:, 1]] + verts[fn[:, 2]]) / np.float32(3) + 1e-3 * rng.standard_normal((300, 3))
    points = np.concatenate([box, on_v, mid, cen, near]).astype(np.float32)
    return verts, faces, points


def error_unit(verts, points, d):
    """E(d) = eps S (d + eps S): eps = 2^-24, S the largest |coordinate| of the input, d the float64 distance."""
    eps = 2.0 ** -24
    S = max(float(np.abs(verts).max()), float(np.abs(points).max()))
    return eps * S * (np.asarray(d, np.float64) + eps * S)
