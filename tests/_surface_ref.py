"""Plain numpy statement of dg-mesh_amd/csrc/surface.hip: the closest point on a triangle mesh, the barycentric
interpolation and the correspondence palette, op for op in the order the kernel file's header writes down.  closest32 is what the kernel
is held to bit for bit; closest64 is the same statement in float64 and qualifies it (tests/test_surface_host.py).  Dense over the faces,
chunked over the queries by 256, as _anchor_ref.nearest32 is.  The second half builds the inputs with thin faces -- marching-cubes
spheres, split tori, sliver soups, micro triangles -- and their queries, and evaluates each once per process (sliver_case)."""
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


def pair_vw(p, a, b, c, with_q=False):
    """The pair arithmetic on broadcastable (..., 3) arrays of one dtype: (v, w, dist2), and q with with_q."""
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
        return (v, w, _dot(e, e), q) if with_q else (v, w, _dot(e, e))


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


def dense_min(points, verts, faces, dtype, visit=None, chunk=256):
    """(argmin, min) over the faces of pair_d2's rows without holding the N x F table (F > 0, V > 0).  visit(rows, ok, a, b, c, v, w, d,
    q), when given, sees every chunk of the pair arithmetic: ok (F,) the candidates, a, b, c (1, F, 3) their corners, v, w, d (n, F)
    and q (n, F, 3) unmasked."""
    p = np.asarray(points, dtype).reshape(-1, 3)
    v = np.asarray(verts, dtype).reshape(-1, 3)
    ok = face_ok(verts, faces, dtype)
    f = np.where(ok[:, None], np.asarray(faces).astype(np.int64).reshape(-1, 3), 0)
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    j, m = np.zeros(len(p), np.int64), np.full(len(p), np.inf, dtype)
    for s in range(0, len(p), chunk):
        rows = slice(s, min(s + chunk, len(p)))
        vv, ww, d, q = pair_vw(p[rows, None, :], a, b, c, with_q=True)
        if visit is not None:
            visit(rows, ok, a, b, c, vv, ww, d, q)
        D = np.where(ok[None, :] & ~np.isnan(d), d, np.inf)
        j[rows] = D.argmin(1)  # (the first index of the minimum: ties to the smaller face)
        m[rows] = D[np.arange(len(D)), j[rows]]
    return j, m


def _closest(points, verts, faces, max_d2, dtype, visit=None):
    p = np.asarray(points, dtype).reshape(-1, 3)
    N = len(p)
    face = np.full(N, -1, np.int32)
    d2 = np.full(N, np.inf, dtype)
    bary = np.zeros((N, 3), dtype)
    F = len(np.asarray(faces).reshape(-1, 3))
    if N == 0 or F == 0 or len(verts) == 0:
        return face, d2, bary
    j, m = dense_min(p, verts, faces, dtype, visit)
    found = m < dtype(max_d2)
    v = np.asarray(verts, dtype).reshape(-1, 3)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)[j[found]]
    vv, ww, dd = pair_vw(p[found], v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
    assert np.array_equal(dd, m[found])
    face[found] = j[found]
    d2[found] = m[found]
    bary[found] = np.stack([(dtype(1) - vv) - ww, vv, ww], 1)
    return face, d2, bary


def closest32(points, verts, faces, max_d2=np.inf, visit=None):
    """(face int32, d2 fp32, bary (N, 3) fp32): the kernel's answer, bit for bit.  visit: dense_min's."""
    return _closest(points, verts, faces, max_d2, np.float32, visit)


def closest64(points, verts, faces, max_d2=np.inf, visit=None):
    """The same statement in float64 (on the float32 inputs)."""
    return _closest(points, verts, faces, max_d2, np.float64, visit)


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


# ---- thin faces: marching-cubes meshes, split tori, sliver soups and micro triangles ----------------------------
def thinness(verts, faces):
    """Height over the longest edge of every face, in float64 (0 for a face without extent)."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    longest = np.sqrt(np.maximum(np.maximum(((b - a) ** 2).sum(1), ((c - b) ** 2).sum(1)), ((a - c) ** 2).sum(1)))
    area2 = np.sqrt((np.cross(b - a, c - a) ** 2).sum(1))
    return np.where(longest > 0, area2 / np.where(longest > 0, longest, 1.0) ** 2, 0.0)


def mc_sphere(delta, R=24):
    """Marching cubes (tests/_mc_ref.py) of a sphere on the R^3 lattice of the unit cube whose surface lies delta h outside the lattice
    nodes on its axes (h = 1 / (R - 1), centre at node (12, 12, 12), radius 6 h + delta h): the isosurface grazes those nodes, and the
    five vertices around each of them are delta h to ~12 delta h apart -- tiny faces, and slivers from there to the next nodes."""
    import _mc_ref
    h = 1.0 / (R - 1)
    x = np.arange(R) * h - 12 * h
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    field = np.sqrt(X * X + Y * Y + Z * Z) - (6 * h + delta * h)
    verts, faces, _ = _mc_ref.marching_cubes(field.astype(np.float32), 0.0)
    return verts.astype(np.float32), faces.astype(np.int32)


def split_torus(h, every=4):
    """torus(40, 20) with every `every`-th face (a, b, c) split by a new vertex m = mid(a, b) + h unit(c - mid(a, b)) into the cap
    sliver (a, b, m) of height h and the two ordinary faces (a, m, c), (m, b, c), in the place of the face: V 1200, F 2400."""
    verts, faces = torus(40, 20)
    v = verts.astype(np.float64)
    picked = np.zeros(len(faces), bool)
    picked[::every] = True
    f = faces[picked]
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    mid = 0.5 * (a + b)
    u = c - mid
    m = mid + h * u / np.sqrt((u * u).sum(1, keepdims=True))
    mi = (len(verts) + np.arange(len(f))).astype(np.int32)
    start = np.cumsum(np.where(picked, 3, 1)) - np.where(picked, 3, 1)
    out = np.empty((len(faces) + 2 * len(f), 3), np.int32)
    out[start[~picked]] = faces[~picked]
    out[start[picked]] = np.stack([f[:, 0], f[:, 1], mi], 1)
    out[start[picked] + 1] = np.stack([f[:, 0], mi, f[:, 2]], 1)
    out[start[picked] + 2] = np.stack([mi, f[:, 1], f[:, 2]], 1)
    return np.concatenate([verts, m.astype(np.float32)]), out


def _unit(x):
    return x / np.sqrt((x * x).sum(-1, keepdims=True))


def sliver_soup(n, L, h, S, seed=0):
    """n isolated cap triangles (a, b, apex): |ab| = L, the apex h above the midpoint of ab, random orientation, centres uniform in
    [-S, S]^3.  With h below the spacing of float32 at S the rounded apex is anywhere within a few ulps of the line ab."""
    rng = np.random.RandomState(seed)
    c = rng.uniform(-S, S, (n, 3))
    u = _unit(rng.standard_normal((n, 3)))
    t = rng.standard_normal((n, 3))
    t = _unit(t - (t * u).sum(1, keepdims=True) * u)
    verts = np.stack([c - 0.5 * L * u, c + 0.5 * L * u, c + h * t], 1).reshape(-1, 3).astype(np.float32)
    return verts, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def micro_triangles(seed=0):
    """208 well-shaped triangles within 1e-3 of the origin with edges L from 1e-9 down to 1e-22, log-spaced, the first half down to
    1e-12 and the second half from there: the fp32 products that form n are of size L^2 and |n|^2 of size L^4, so |n|^2 is normal
    down to L ~ 3e-10, denormal down to L ~ 6e-12 and 0 below -- the candidate rule (len > 0 and finite) on its boundary, where a
    kernel that flushed denormals would decide otherwise.  (Edges of 1e-10 alone would start in the denormal range: the first
    decade is there for the normal one.)  A triangle lies 64 L from the origin, so that its shape survives the rounding to
    float32, except every eighth of those with L > 1e-10, which lies up to 1e-3 out, where the float32 spacing is of its own size."""
    rng = np.random.RandomState(seed)
    n = 208
    L = 10.0 ** np.concatenate([np.linspace(-9, -12, n // 2, endpoint=False), np.linspace(-12, -22, n // 2)])
    r = 64 * L
    far = (np.arange(n) % 8 == 3) & (L > 1e-10)
    r[far] = 1e-3 * rng.uniform(0.1, 1.0, far.sum())
    o = _unit(rng.standard_normal((n, 3))) * r[:, None]
    u = _unit(rng.standard_normal((n, 3)))
    t = rng.standard_normal((n, 3))
    t = _unit(t - (t * u).sum(1, keepdims=True) * u)
    th = rng.uniform(np.pi / 9, 8 * np.pi / 9, (n, 1))
    s = rng.uniform(0.5, 1.0, (n, 1))
    verts = np.stack([o, o + L[:, None] * u, o + L[:, None] * s * (np.cos(th) * u + np.sin(th) * t)], 1).reshape(-1, 3).astype(np.float32)
    return verts, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


N_ON, N_FAR = 400, 16  # queries per on-face group of sliver_queries, and in its last group


def sliver_queries(verts, faces, seed, thin=1e-3):
    """Queries of a mesh with thin faces, in this order (float32):
      [0, 400) [400, 800) [800, 1200)   points at random barycentrics of faces with thinness < thin (of all faces where none is
                                        that thin), displaced by 0, 1e-6 and 1e-4 N(0, 1);
      [1200, 2400)                      points of random faces displaced by 0.02 N(0, 1);
      [2400, 2400 + V)                  every mesh vertex itself;
      [2400 + V, 2400 + V + 16)         points 12 mean edge lengths outside the sphere around the mesh's box: farther than any bound
                                        the tests search with (10 mean edges), so that every bounded search leaves some unmatched."""
    rng = np.random.RandomState(seed)
    v = np.asarray(verts, np.float64)
    pool = np.nonzero(thinness(verts, faces) < thin)[0]
    if len(pool) == 0:
        pool = np.arange(len(faces))

    def near(idx, sigma):
        f = faces[idx]
        b = rng.dirichlet((1, 1, 1), len(f))
        return v[f[:, 0]] * b[:, 0:1] + v[f[:, 1]] * b[:, 1:2] + v[f[:, 2]] * b[:, 2:3] + sigma * rng.standard_normal((len(f), 3))

    parts = [near(pool[rng.randint(0, len(pool), N_ON)], sigma) for sigma in (0.0, 1e-6, 1e-4)]
    parts.append(near(rng.randint(0, len(faces), 1200), 0.02))
    parts.append(v)
    f = np.asarray(faces).astype(np.int64)
    edge = np.sqrt(((np.concatenate([v[f[:, 0]] - v[f[:, 1]], v[f[:, 1]] - v[f[:, 2]]])) ** 2).sum(1)).mean()
    lo, hi = v.min(0), v.max(0)
    parts.append(0.5 * (lo + hi) + (0.5 * np.sqrt(((hi - lo) ** 2).sum()) + 12 * edge) * _unit(rng.standard_normal((N_FAR, 3))))
    return np.concatenate(parts).astype(np.float32)


class PairCheck:
    """A visit of dense_min for the fp32 pass: over every (query, candidate face) pair with a finite dist2 (no other can be
    reported), how far q leaves the face's exact AABB in units of 2^-24 S_face (S_face the face's largest |coordinate|); how many
    pairs of a candidate face have a NaN dist2, how many an infinite one, and which faces those are."""

    def __init__(self):
        self.excursion, self.nan_pairs, self.inf_pairs, self.pairs, self.bad_faces = 0.0, 0, 0, 0, set()
        self.bary_min, self.bary_max = np.float32(0), np.float32(1)  # of v, w and (1 - v) - w over the same pairs

    def __call__(self, rows, ok, a, b, c, v, w, d, q):
        lo = np.minimum(np.minimum(a, b), c).astype(np.float64)
        hi = np.maximum(np.maximum(a, b), c).astype(np.float64)
        S = np.maximum(np.abs(lo), np.abs(hi)).max(-1)
        q = q.astype(np.float64)
        with np.errstate(all="ignore"):
            out = np.maximum(np.maximum(lo - q, q - hi), 0.0).max(-1) / (2.0 ** -24 * np.where(ok[None, :], S, 1.0))
        nan, inf = ok[None, :] & np.isnan(d), ok[None, :] & np.isinf(d)
        cand = ok[None, :] & np.isfinite(d)
        self.pairs += int(ok.sum()) * d.shape[0]
        self.nan_pairs += int(nan.sum())
        self.inf_pairs += int(inf.sum())
        self.bad_faces |= set(np.nonzero((nan | inf).any(0))[0].tolist())
        if cand.any():
            self.excursion = max(self.excursion, float(out[cand].max()))
            u = (np.float32(1) - v[cand]) - w[cand]
            self.bary_min = min(self.bary_min, v[cand].min(), w[cand].min(), u.min())
            self.bary_max = max(self.bary_max, v[cand].max(), w[cand].max(), u.max())


MESH_CASES = {
    "mc_sphere_1e-3": lambda: mc_sphere(1e-3), "mc_sphere_1e-5": lambda: mc_sphere(1e-5), "mc_sphere_1e-6": lambda: mc_sphere(1e-6),
    "split_torus_1e-4": lambda: split_torus(1e-4), "split_torus_1e-6": lambda: split_torus(1e-6),
    "split_torus_1e-7": lambda: split_torus(1e-7),
}
SOUP_CASES = {f"soup_h{h:g}_S{S}": (lambda h=h, S=S, k=k: sliver_soup(500, 1e-2, h, S, seed=20 + k))
              for k, (h, S) in enumerate((h, S) for h in (1e-5, 3e-7, 3e-8) for S in (1, 10))}
SLIVER_CASES = {**MESH_CASES, **SOUP_CASES, "micro": micro_triangles}
SLIVER_HEIGHT = {"split_torus_1e-4": 1e-4, "split_torus_1e-6": 1e-6, "split_torus_1e-7": 1e-7,
                 **{f"soup_h{h:g}_S{S}": h for h in (1e-5, 3e-7, 3e-8) for S in (1, 10)}}
# the faces counted as thin: thinness < 1e-3, except on mc_sphere(1e-3), which has none (its thinnest 48 faces, the slivers at the six
# grazed nodes, have 1.64e-3 to 1.9e-3: thinness goes with delta there; the next are at 1.2e-2)
THIN = {"mc_sphere_1e-3": 2e-3}
_cases = {}


def sliver_case(name):
    """One input of SLIVER_CASES with its sliver_queries and the fp32 statement's unbounded answer, evaluated once per process and
    shared by tests/test_surface_host.py and tests/test_surface_kernels.py: dict(verts, faces, points, ref, check) -- ref is
    closest32's (face, d2, bary), check the PairCheck of that evaluation.  Callers do not modify it."""
    if name not in _cases:
        verts, faces = SLIVER_CASES[name]()
        points = sliver_queries(verts, faces, seed=100 + list(SLIVER_CASES).index(name), thin=THIN.get(name, 1e-3))
        check = PairCheck()
        ref = closest32(points, verts, faces, visit=check)
        _cases[name] = dict(verts=verts, faces=faces, points=points, ref=ref, check=check)
    return _cases[name]
