"""numpy restatement of the generalised winding number (dg-mesh_amd/mesh_inside.py, csrc/mesh_inside.hip; the definition and the
summation order are in include/dgmesh_hip.h).  No torch, nothing from the reference project.

winding(points, verts, faces, dtype) evaluates the definition in `dtype`: np.float64 is the reference the device is held to,
np.float32 is the same statement in the device's number format and the device's summation order -- its distance from the fp64
result is the measure of what fp32 can give on a case, from which the GPU test takes its tolerance.  numpy's elementwise operations
round once each and never contract a product and a sum; sums run through np.add.accumulate, which adds one after the other (never
np.sum, which adds pairwise)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

CHUNK = 256          # faces per fp32 chunk sum
SLICE_CHUNKS = 64    # chunks per fp64 slice sum
QUERY_BLOCK = 2048   # rows per pass (memory only: no result depends on it)
THREADS = 8          # passes in flight (time only)


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def solid_angles(points, corners, ok, dtype):
    """omega (N, M) of N queries against M faces: corners (M, 3, 3) in dtype, ok (M,) = the face may contribute at all."""
    p = points[:, None, :]
    a, b, c = corners[None, :, 0] - p, corners[None, :, 1] - p, corners[None, :, 2] - p
    n0 = b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1]
    n1 = b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2]
    n2 = b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]
    det = (a[..., 0] * n0 + a[..., 1] * n1) + a[..., 2] * n2
    la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
    ab, bc, ca = _dot(a, b), _dot(b, c), _dot(c, a)
    den = (((la * lb) * lc + ab * lc) + bc * la) + ca * lb
    omega = dtype(2) * np.arctan2(det, den)
    assert omega.dtype == dtype
    keep = ok[None, :] & (det != 0) & np.isfinite(det)
    return np.where(keep, omega, dtype(0))


def winding(points, verts, faces, dtype=np.float64):
    """w (N,) float32 for dtype float32 -- the device's statement: omega summed in fp32 per chunk of 256 faces, the chunk sums in
    fp64 per slice of 64 chunks, the slice sums in fp64, w = float32(sum / (4 pi)) -- and w (N,) float64 for dtype float64: every
    operation in fp64, the same order."""
    dtype = np.dtype(dtype).type
    points = np.asarray(points, np.float32).reshape(-1, 3)
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    N, V, F = len(points), len(verts), len(faces)
    inside = ((faces >= 0) & (faces < V)).all(1)
    corners = np.zeros((F, 3, 3), np.float32)
    corners[inside] = verts[faces[inside]]
    ok = inside & np.isfinite(corners).all((1, 2))
    corners[~ok] = 0
    corners = corners.astype(dtype)
    def block(q0):
        with np.errstate(all="ignore"):
            p = points[q0:q0 + QUERY_BLOCK].astype(dtype)
            total = np.zeros(len(p), np.float64)
            for s0 in range(0, F, CHUNK * SLICE_CHUNKS):
                slice_sum = np.zeros(len(p), np.float64)
                for c0 in range(s0, min(s0 + CHUNK * SLICE_CHUNKS, F), CHUNK):
                    omega = solid_angles(p, corners[c0:c0 + CHUNK], ok[c0:c0 + CHUNK], dtype)
                    chunk_sum = np.add.accumulate(omega, axis=1, dtype=dtype)[:, -1]  # from the first face on, one after the other
                    slice_sum = slice_sum + chunk_sum.astype(np.float64)
                total = total + slice_sum
            return total / (4.0 * np.pi)

    starts = range(0, N, QUERY_BLOCK)
    if len(starts) > 1:  # rows are independent of each other: blocks of them on a few threads (numpy releases the lock inside its loops)
        with ThreadPoolExecutor(max_workers=THREADS) as pool:
            parts = list(pool.map(block, starts))
    else:
        parts = [block(q0) for q0 in starts]
    out = np.concatenate(parts) if parts else np.zeros(0, np.float64)
    out[~np.isfinite(points).all(1)] = np.nan
    return out.astype(np.float32) if dtype is np.float32 else out


def box_queries(verts, n, seed, scale=1.1):
    """n points uniform in the bounding box of the finite vertices, scaled by `scale` about its centre (float32)."""
    v = np.asarray(verts, np.float64)
    v = v[np.isfinite(v).all(1)]
    lo, hi = v.min(0), v.max(0)
    centre, half = (lo + hi) / 2, (hi - lo) / 2 * scale
    u = np.random.default_rng(seed).random((n, 3))
    return (centre - half + u * 2 * half).astype(np.float32)


# ---- the cases of the GPU test --------------------------------------------------------------------------------------------------------
def reversed_faces(faces):
    return np.ascontiguousarray(np.asarray(faces)[:, ::-1])


def join(*meshes):
    """One mesh of several: the vertex arrays appended, the indices shifted."""
    verts, faces, at = [], [], 0
    for v, f in meshes:
        verts.append(np.asarray(v, np.float32))
        faces.append(np.asarray(f, np.int32) + at)
        at += len(v)
    return np.concatenate(verts), np.concatenate(faces).astype(np.int32)


def open_icosphere(subdivisions=2, cut=0.3):
    """The icosphere without the faces whose centroid has z >= cut: a bowl with one rim."""
    from _edges_ref import icosphere
    verts, faces = icosphere(subdivisions)
    keep = verts[faces].mean(1)[:, 2] < cut
    return verts, np.ascontiguousarray(faces[keep])


def salted_icosphere(subdivisions=2):
    """The icosphere with faces that must add nothing mixed in: indices of -1 and V, a corner at a NaN vertex (appended, used by
    the salt only), and zero-area faces (a repeated corner; three corners on one line).  -> verts, faces, the salt: its first five
    faces add exactly 0, the zero-area ones a det of rounding noise (a . (a x c) is not exactly 0 in floating point)."""
    from _edges_ref import icosphere
    verts, faces = icosphere(subdivisions)
    n0 = len(verts)
    verts = np.concatenate([verts, np.array([[np.nan, 0.5, 0.5], [0, 0, 2], [0, 0, 3], [0, 0, 4]], np.float32)])
    V = len(verts)
    salt = np.array([[-1, 0, 1], [0, 1, V], [2, 3, V + 7], [0, 1, n0], [n0, 4, 5], [6, 6, 7], [8, 9, 8], [n0 + 1, n0 + 2, n0 + 3]], np.int32)
    faces = np.concatenate([faces[:100], salt[:4], faces[100:], salt[4:]]).astype(np.int32)
    return verts, faces, salt
