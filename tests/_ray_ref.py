"""numpy restatement of ray casting against a mesh (dg-mesh_amd/mesh_ray.py, csrc/mesh_ray.hip; the definition is in
include/dgmesh_hip.h and the order of every operation at the head of the .hip file).  No torch, nothing from the reference project.

cast(origins, dirs, verts, faces, t_min, t_max, dtype) evaluates the definition in `dtype`: np.float32 is the device's arithmetic
operation for operation -- the watertight pair test of Woop, Benthin and Wald with its fp64 fallback when an edge value is exactly 0,
the lexicographic minimum of (t, face index) -- and np.float64 is the same statement with every operation in fp64, the reference the
device is held to.  numpy's elementwise operations round once each and never contract a product and a sum."""
import numpy as np

RAY_BLOCK = 256  # rays per pass (memory only: no result depends on it)


def frame(origins, dirs, dtype):
    """Per ray: kx, ky, kz, Sx, Sy, Sz and whether the ray tests anything (finite components, d != 0)."""
    o, d = origins.astype(dtype), dirs.astype(dtype)
    ad = np.abs(d)
    valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (ad.max(1, initial=0) > 0)
    kz = np.argmax(np.where(np.isnan(ad), 0, ad), axis=1)  # the first largest: ties go to the lowest index
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    rows = np.arange(len(d))
    dz = d[rows, kz]
    swap = dz < 0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    with np.errstate(all="ignore"):
        Sx, Sy, Sz = d[rows, kx] / dz, d[rows, ky] / dz, dtype(1) / dz
    return kx, ky, kz, Sx, Sy, Sz, valid


def pair(origins, dirs, corners, dtype):
    """The pair arithmetic of n rays against corners (n or 1, M, 3, 3): a dict of (n, M) arrays -- U, V, W, det, t in dtype, `mixed`
    (one edge value < 0 and one > 0: a miss) -- and `valid` (n,).  No acceptance test: accept() applies the bounds."""
    dtype = np.dtype(dtype).type
    o = origins.astype(dtype)
    kx, ky, kz, Sx, Sy, Sz, valid = frame(origins, dirs, dtype)
    with np.errstate(all="ignore"):
        a = corners.astype(dtype) - o[:, None, None, :]  # (n, M, corner, axis)
        axis = lambda k: np.take_along_axis(a, k[:, None, None, None], axis=3)[..., 0]  # (n, M, corner)
        az = axis(kz)
        X = axis(kx) - Sx[:, None, None] * az
        Y = axis(ky) - Sy[:, None, None] * az
        Z = Sz[:, None, None] * az
        (Ax, Bx, Cx), (Ay, By, Cy), (Az, Bz, Cz) = (np.moveaxis(q, 2, 0) for q in (X, Y, Z))
        U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        assert U.dtype == dtype
        zero = (U == 0) | (V == 0) | (W == 0)
        f64 = lambda q: q.astype(np.float64)
        u = f64(Cx) * f64(By) - f64(Cy) * f64(Bx)
        v = f64(Ax) * f64(Cy) - f64(Ay) * f64(Cx)
        w = f64(Bx) * f64(Ay) - f64(By) * f64(Ax)
        neg = np.where(zero, (u < 0) | (v < 0) | (w < 0), (U < 0) | (V < 0) | (W < 0))
        pos = np.where(zero, (u > 0) | (v > 0) | (w > 0), (U > 0) | (V > 0) | (W > 0))
        U, V, W = np.where(zero, u.astype(dtype), U), np.where(zero, v.astype(dtype), V), np.where(zero, w.astype(dtype), W)
        det = (U + V) + W
        t = ((U * Az + V * Bz) + W * Cz) / det
    assert t.dtype == dtype
    return {"U": U, "V": V, "W": W, "det": det, "t": t, "mixed": neg & pos, "valid": valid}


def accept(p, t_min, t_max):
    """(n, M) bool: the faces the pair test accepts (before the mesh's own validity)."""
    t = p["t"]
    with np.errstate(all="ignore"):
        return p["valid"][:, None] & ~p["mixed"] & (p["det"] != 0) & (t >= np.float32(t_min)) & (t < np.float32(t_max)) & np.isfinite(t)


def face_corners(verts, faces):
    """corners (F, 3, 3) float32 (zeros where the face can never hit) and ok (F,): every index inside [0, V) and every corner finite."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    inside = ((faces >= 0) & (faces < len(verts))).all(1)
    corners = np.zeros((len(faces), 3, 3), np.float32)
    corners[inside] = verts[faces[inside]]
    ok = inside & np.isfinite(corners).all((1, 2))
    corners[~ok] = 0
    return corners, ok


def cast(origins, dirs, verts, faces, t_min=0.0, t_max=np.inf, dtype=np.float32):
    """-> face (N,) int32, t (N,) dtype, bary (N, 3) dtype: the lexicographic minimum of (t, face index) over the accepted faces;
    none: -1, +inf, 0."""
    dtype = np.dtype(dtype).type
    origins = np.asarray(origins, np.float32).reshape(-1, 3)
    dirs = np.asarray(dirs, np.float32).reshape(-1, 3)
    corners, ok = face_corners(verts, faces)
    N, F = len(origins), len(corners)
    face = np.full(N, -1, np.int32)
    t = np.full(N, np.inf, dtype)
    bary = np.zeros((N, 3), dtype)
    if F == 0:
        return face, t, bary
    for r0 in range(0, N, RAY_BLOCK):
        sl = slice(r0, r0 + RAY_BLOCK)
        p = pair(origins[sl], dirs[sl], corners[None], dtype)
        acc = accept(p, t_min, t_max) & ok[None]
        tt = np.where(acc, p["t"], dtype(np.inf))
        best = tt.min(1)
        first = np.argmax(acc & (tt == best[:, None]), axis=1)  # the lowest index among the nearest
        hit = acc.any(1)
        rows = np.arange(len(first))
        with np.errstate(all="ignore"):
            b = np.stack([p[k][rows, first] / p["det"][rows, first] for k in ("U", "V", "W")], axis=1)
        face[sl] = np.where(hit, first, -1)
        t[sl] = np.where(hit, best, dtype(np.inf))
        bary[sl] = np.where(hit[:, None], b, dtype(0))
    return face, t, bary


def on_face(origins, dirs, verts, faces, face, dtype=np.float64):
    """The pair arithmetic of ray n against face[n] alone (face[n] >= 0): a dict of (N,) arrays as pair() gives, plus `bary` (N, 3)."""
    origins = np.asarray(origins, np.float32).reshape(-1, 3)
    dirs = np.asarray(dirs, np.float32).reshape(-1, 3)
    corners, _ = face_corners(verts, faces)
    p = pair(origins, dirs, corners[np.asarray(face)][:, None], dtype)
    out = {k: (q[:, 0] if q.ndim == 2 else q) for k, q in p.items()}
    with np.errstate(all="ignore"):
        out["bary"] = np.stack([out[k] / out["det"] for k in ("U", "V", "W")], axis=1)
    return out


# ---- the meshes and rays of the tests ---------------------------------------------------------------------------------------------------
def torus(n_major=24, n_minor=12, R=1.0, r=0.35):
    """A closed torus about the z axis, 2 n_major n_minor faces."""
    u = np.arange(n_major) * (2 * np.pi / n_major)
    v = np.arange(n_minor) * (2 * np.pi / n_minor)
    uu, vv = np.meshgrid(u, v, indexing="ij")
    verts = np.stack([(R + r * np.cos(vv)) * np.cos(uu), (R + r * np.cos(vv)) * np.sin(uu), r * np.sin(vv)], axis=-1).reshape(-1, 3)
    idx = lambda i, j: (i % n_major) * n_minor + (j % n_minor)
    faces = []
    for i in range(n_major):
        for j in range(n_minor):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            faces += [(a, b, c), (a, c, d)]
    return verts.astype(np.float32), np.array(faces, np.int32)


def cube(lo=0.0, hi=1.0):
    """The axis-aligned cube [lo, hi]^3, 12 faces wound outwards; faces 2k and 2k + 1 share the diagonal of side k."""
    c = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], np.float32)  # index 4 x + 2 y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = []
    for a, b, cc, d in quads:
        faces += [(a, b, cc), (a, cc, d)]
    return c, np.array(faces, np.int32)


def lattice(n):
    """Unit quads on the integer planes of [0, n]^3, every quad split into two triangles: 3 (n + 1) n^2 quads, 6 (n + 1) n^2 faces;
    vertices on the integer lattice."""
    g = np.arange(n + 1)
    verts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    vid = lambda p: (p[0] * (n + 1) + p[1]) * (n + 1) + p[2]
    faces = []
    for axis in range(3):
        e1, e2 = np.eye(3, dtype=int)[(axis + 1) % 3], np.eye(3, dtype=int)[(axis + 2) % 3]
        for k in range(n + 1):
            for i in range(n):
                for j in range(n):
                    p = k * np.eye(3, dtype=int)[axis] + i * e1 + j * e2
                    a, b, c, d = vid(p), vid(p + e1), vid(p + e1 + e2), vid(p + e2)
                    faces += [(a, b, c), (a, c, d)]
    return verts, np.array(faces, np.int32)


def lattice_rays(n):
    """Axis-parallel rays with their origins exactly on lattice planes and lines (and half-way between them), from outside and from
    inside the lattice, in both directions of every axis: direction components of exactly 0."""
    coords = np.arange(0, n + 0.25, 0.5)
    origins, dirs = [], []
    for axis in range(3):
        for sign in (1.0, -1.0):
            for start in (-1.0, n + 1.0, 0.0, 1.0, 0.5):
                a, b = np.meshgrid(coords, coords, indexing="ij")
                o = np.zeros((a.size, 3))
                o[:, axis] = start
                o[:, (axis + 1) % 3], o[:, (axis + 2) % 3] = a.reshape(-1), b.reshape(-1)
                d = np.zeros((a.size, 3))
                d[:, axis] = sign
                origins.append(o)
                dirs.append(d)
    return np.concatenate(origins).astype(np.float32), np.concatenate(dirs).astype(np.float32)


def soup(F, seed, V=None):
    """Random triples over a few vertices, some indices outside [0, V) and a NaN vertex (test_mesh_inside_redzone.scene's recipe)."""
    rng = np.random.default_rng(seed)
    V = max(3, min(F, 1000)) if V is None else V
    verts = rng.standard_normal((V, 3)).astype(np.float32)
    faces = rng.integers(0, V, (F, 3)).astype(np.int32)
    faces[::11, 0], faces[5::13, 2] = -1, V
    if V > 3:
        verts[V // 2, 1] = np.nan
    return verts, faces


def random_rays(n, seed, scale=1.5):
    """n rays: origins normal about 0 with deviation `scale` / 2 (inside and outside a unit mesh), directions normal, not normalised."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 3)) * scale / 2).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)


def watertight_rays(verts, faces, origin, n_random, seed):
    """From `origin`: n_random random directions, then a direction to every vertex and to every edge midpoint -> origins, dirs,
    n_random (the rays behind it aim at vertices and edges)."""
    rng = np.random.default_rng(seed)
    origin = np.asarray(origin, np.float32)
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    e = np.unique(e, axis=0)
    mid = ((verts[e[:, 0]].astype(np.float64) + verts[e[:, 1]].astype(np.float64)) / 2).astype(np.float32)
    targets = np.concatenate([verts, mid])
    dirs = np.concatenate([rng.standard_normal((n_random, 3)).astype(np.float32), targets - origin])
    return np.broadcast_to(origin, dirs.shape).copy(), dirs, n_random
