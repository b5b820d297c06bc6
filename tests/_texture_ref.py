"""numpy restatement of texture sampling and the texture atlas (dg-mesh_amd/mesh_raster.texture, dg-mesh_amd/mesh_texture.py,
csrc/mesh_texture.hip).  Every function takes the number format: np.float64 is the reference, np.float32 follows the device's
operation order step by step (no FMA, one rounding per operation), so its deviation from the fp64 statement is what the number format
gives on a case -- the tests' tolerance is a multiple of it.

Conventions: tex (Ht, Wt, C), uv (n, 2); texel (i, j) is centred at u = (i + .5) / Wt, v = (j + .5) / Ht, row 0 of memory at v = 0."""
import numpy as np

FILTERS = ("nearest", "linear")
BOUNDARIES = ("wrap", "clamp", "zero")


def _axis_linear(u, N, boundary, dt):
    """-> (i0, i1, fx): the two texel indices of one axis (-1: not read, counts as 0) and the weight of the second."""
    W, half = dt(N), dt(0.5)
    with np.errstate(all="ignore"):
        if boundary == "wrap":
            x = (u - np.floor(u)) * W - half
        elif boundary == "clamp":
            x = np.minimum(np.maximum(u * W - half, dt(-1)), W)
        else:
            x = np.minimum(np.maximum(u * W - half, dt(-2)), W + dt(1))
    x0 = np.floor(x)
    fx = x - x0
    i0 = x0.astype(np.int64)
    i1 = i0 + 1
    if boundary == "wrap":
        i0, i1 = np.where(i0 < 0, i0 + N, i0), np.where(i1 >= N, i1 - N, i1)
    elif boundary == "clamp":
        i0, i1 = np.clip(i0, 0, N - 1), np.clip(i1, 0, N - 1)
    else:
        i0, i1 = np.where((i0 < 0) | (i0 >= N), -1, i0), np.where((i1 < 0) | (i1 >= N), -1, i1)
    return i0, i1, fx


def _axis_nearest(u, N, boundary, dt):
    W = dt(N)
    with np.errstate(all="ignore"):
        if boundary == "wrap":
            i = np.floor((u - np.floor(u)) * W).astype(np.int64)
            return np.where(i >= N, i - N, i)
        i = np.floor(np.minimum(np.maximum(u * W, dt(-1)), W)).astype(np.int64)
    if boundary == "clamp":
        return np.clip(i, 0, N - 1)
    return np.where((i < 0) | (i >= N), -1, i)


def _texels(tex, i, j):
    """tex[j, i] with zeros where either index is -1."""
    ok = (i >= 0) & (j >= 0)
    return np.where(ok[:, None], tex[np.where(ok, j, 0), np.where(ok, i, 0)], tex.dtype.type(0))


def _split(uv, dt):
    uv = np.asarray(uv)
    finite = np.isfinite(uv).all(1)
    safe = np.where(finite[:, None], uv, 0).astype(dt)
    return safe[:, 0], safe[:, 1], finite


def taps(uv, Ht, Wt, boundary, dt):
    """The four taps of a linear sample: (i0, i1, j0, j1, fx, fy, finite)."""
    u, v, finite = _split(uv, dt)
    i0, i1, fx = _axis_linear(u, Wt, boundary, dt)
    j0, j1, fy = _axis_linear(v, Ht, boundary, dt)
    return i0, i1, j0, j1, fx, fy, finite


def sample(tex, uv, filter_mode="linear", boundary_mode="wrap", dtype=np.float64):
    """out (n, C) in `dtype`; zeros where u or v is not finite."""
    dt = dtype
    tex = np.asarray(tex).astype(dt)
    Ht, Wt = tex.shape[:2]
    if filter_mode == "nearest":
        u, v, finite = _split(uv, dt)
        out = _texels(tex, _axis_nearest(u, Wt, boundary_mode, dt), _axis_nearest(v, Ht, boundary_mode, dt))
    else:
        i0, i1, j0, j1, fx, fy, finite = taps(uv, Ht, Wt, boundary_mode, dt)
        gx, gy = dt(1) - fx, dt(1) - fy
        w00, w10, w01, w11 = (gx * gy)[:, None], (fx * gy)[:, None], (gx * fy)[:, None], (fx * fy)[:, None]
        out = ((w00 * _texels(tex, i0, j0) + w10 * _texels(tex, i1, j0)) + w01 * _texels(tex, i0, j1)) + w11 * _texels(tex, i1, j1)
    return np.where(finite[:, None], out, dt(0)).astype(dt)


def sample_grads(tex, uv, dout, filter_mode="linear", boundary_mode="wrap", dtype=np.float64):
    """Gradients of sum(sample * dout) in `dtype`: dtex (Ht, Wt, C), the transpose of the weights (terms w * dout added in sample order;
    the device adds them in any order), and duv (n, 2), analytic and in the device's order:
    du = W * sum_c dout_c * (gy * (t10 - t00) + fy * (t11 - t01)), dv alike, the sums from 0 in channel order; zero for nearest and
    for non-finite samples."""
    dt = dtype
    tex = np.asarray(tex).astype(dt)
    dout = np.asarray(dout).astype(dt)
    Ht, Wt, C = tex.shape
    dtex, duv = np.zeros_like(tex), np.zeros((len(uv), 2), dt)

    def scatter(i, j, w):
        ok = (i >= 0) & (j >= 0) & finite
        np.add.at(dtex, (j[ok], i[ok]), w[ok, None] * dout[ok])

    if filter_mode == "nearest":
        u, v, finite = _split(uv, dt)
        scatter(_axis_nearest(u, Wt, boundary_mode, dt), _axis_nearest(v, Ht, boundary_mode, dt), np.ones(len(uv), dt))
        return dtex, duv
    i0, i1, j0, j1, fx, fy, finite = taps(uv, Ht, Wt, boundary_mode, dt)
    gx, gy = dt(1) - fx, dt(1) - fy
    for i, j, w in ((i0, j0, gx * gy), (i1, j0, fx * gy), (i0, j1, gx * fy), (i1, j1, fx * fy)):
        scatter(i, j, w)
    t00, t10, t01, t11 = _texels(tex, i0, j0), _texels(tex, i1, j0), _texels(tex, i0, j1), _texels(tex, i1, j1)
    su, sv = np.zeros(len(uv), dt), np.zeros(len(uv), dt)
    for c in range(C):
        su = su + dout[:, c] * (gy * (t10[:, c] - t00[:, c]) + fy * (t11[:, c] - t01[:, c]))
        sv = sv + dout[:, c] * (gx * (t01[:, c] - t00[:, c]) + fx * (t11[:, c] - t10[:, c]))
    duv[:, 0], duv[:, 1] = np.where(finite, dt(Wt) * su, dt(0)), np.where(finite, dt(Ht) * sv, dt(0))
    return dtex, duv


def dtex_bound(tex_shape, uv, dout, filter_mode="linear", boundary_mode="wrap"):
    """An a-priori bound on the error of an fp32 dtex, per texel and channel, whatever the order of the additions: a texel's value is a
    sum of m terms w * dout, each term carrying the roundings of its weight (1 - f, the product of two factors) and of the product with
    dout, and a recursive fp32 sum of m terms adds at most (m - 1) u sum|terms|; so |error| <= (m + 3) u sum|terms| / (1 - (m + 3) u) with
    u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  The weights themselves come from fx, fy, whose
    own fp32 error is at most 2 u r texels per axis, r = max(|u|, |v|, 1) max(Wt, Ht) + 2 bounding every intermediate of
    (u - floor(u)) * W - .5 and u * W - .5 in texels; a weight's slope is at most 1 per texel and axis, so a term moves by at most
    4 u r |dout|: added as such.  Valid for |uv| <= 4 (r is capped there) and for |uv| >= 2^24, where u - floor(u) is exactly 0 and
    the clamps saturate in either number format."""
    Ht, Wt, C = tex_shape
    dt = np.float64
    dout = np.abs(np.asarray(dout).astype(dt))
    mag, cnt, coord = np.zeros(tex_shape, dt), np.zeros((Ht, Wt, 1), dt), np.zeros(tex_shape, dt)
    u, v, finite = _split(uv, dt)
    if filter_mode == "nearest":
        tap_list = [(_axis_nearest(u, Wt, boundary_mode, dt), _axis_nearest(v, Ht, boundary_mode, dt), np.ones(len(uv), dt))]
    else:
        i0, i1, j0, j1, fx, fy, finite = taps(uv, Ht, Wt, boundary_mode, dt)
        tap_list = [(i0, j0, (1 - fx) * (1 - fy)), (i1, j0, fx * (1 - fy)), (i0, j1, (1 - fx) * fy), (i1, j1, fx * fy)]
    with np.errstate(all="ignore"):
        reach = np.where(finite, np.minimum(np.maximum(np.maximum(np.abs(u), np.abs(v)), 1.0), 4.0) * max(Ht, Wt) + 2.0, 0.0)
    for i, j, w in tap_list:
        ok = (i >= 0) & (j >= 0) & finite
        np.add.at(mag, (j[ok], i[ok]), w[ok, None] * dout[ok])
        np.add.at(cnt, (j[ok], i[ok]), 1.0)
        np.add.at(coord, (j[ok], i[ok]), reach[ok, None] * dout[ok])
    eps = 2.0 ** -24
    k = (cnt + 3) * eps
    return k / (1 - k) * mag + (0.0 if filter_mode == "nearest" else 4 * eps * coord)


def lattice_distance(uv, Ht, Wt):
    """The distance, in texels, of every sample from the nearest line of the texel-centre lattice (where the bilinear weights have a
    kink and duv is not defined), per axis: (n, 2)."""
    x = np.asarray(uv, np.float64) * np.array([Wt, Ht], np.float64) - 0.5
    return np.abs(x - np.round(x))


# ---- the atlas ------------------------------------------------------------------------------------------------------------------------
def per_row(F):
    """ceil(sqrt(ceil(F / 2))) in integers."""
    n, r = (F + 1) // 2, 0
    while r * r < n:
        r += 1
    return max(r, 1)


def corner_local(s):
    """(2, 3, 2): the cell-local texel-centre index coordinates (i, j) of the corners 0, 1, 2 of the even and the odd face."""
    L = s - 3
    return np.array([[(0, 0), (L, 0), (0, L)], [(s - 1, s - 1), (2, s - 1), (s - 1, 2)]], np.int64)


def atlas_uv(F, size, cell, dtype=np.float32):
    dt = dtype
    f = np.arange(F)
    c, odd = f // 2, f % 2
    cpr = size // cell
    base = np.stack([(c % cpr) * cell, (c // cpr) * cell], 1)  # (F, 2): the cell's first texel
    idx = base[:, None, :] + corner_local(cell)[odd]             # (F, 3, 2)
    return ((idx.astype(dt) + dt(0.5)) / dt(size)).astype(dt)


def owner(size, cell, F):
    """-> (face (size, size) int64 with -1 for unowned, i, j): the owning face of every texel before the faces' indices are looked at,
    and the texel's cell-local coordinates."""
    s, cpr = cell, size // cell
    y, x = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    cx, cy = x // s, y // s
    i, j = x - cx * s, y - cy * s
    c = cy * cpr + cx
    face = np.where(i + j <= s - 2, 2 * c, np.where(i + j >= s, 2 * c + 1, -1))
    face = np.where((cx < cpr) & (cy < cpr) & (face < F), face, -1)
    return face, i, j


def atlas_interpolate(attr, faces, size, cell, dtype=np.float64):
    """-> (out (size, size, C) in `dtype`, face_id (size, size) int32)."""
    dt = dtype
    attr = np.asarray(attr)
    V, F, s = len(attr), len(faces), cell
    face, i, j = owner(size, cell, F)
    fz = np.where(face >= 0, face, 0)
    idx = np.asarray(faces, np.int64)[fz] if F else np.zeros(face.shape + (3,), np.int64)
    face = np.where((face >= 0) & ((idx >= 0) & (idx < V)).all(-1), face, -1)
    odd = (face % 2 == 1) & (face >= 0)
    L = dt(s - 3)
    b1 = np.where(odd, s - 1 - i, i).astype(dt) / L
    b2 = np.where(odd, s - 1 - j, j).astype(dt) / L
    b0 = (dt(1) - b1) - b2
    a = attr.astype(dt)[np.clip(idx, 0, max(V - 1, 0))] if V else np.zeros(face.shape + (3, attr.shape[1]), dt)
    with np.errstate(invalid="ignore"):
        out = (b0[..., None] * a[..., 0, :] + b1[..., None] * a[..., 1, :]) + b2[..., None] * a[..., 2, :]
    return np.where((face >= 0)[..., None], out, dt(0)).astype(dt), face.astype(np.int32)


def footprint(points):
    """The set of texels (i, j) that carry a non-zero bilinear weight for any of the points (n, 2), given in texel-centre index
    coordinates (texel k is centred at k): per axis floor(x), and floor(x) + 1 when x is not an integer."""
    out = set()
    for x, y in np.asarray(points, np.float64):
        xs = [int(np.floor(x))] + ([int(np.floor(x)) + 1] if x != np.floor(x) else [])
        ys = [int(np.floor(y))] + ([int(np.floor(y)) + 1] if y != np.floor(y) else [])
        out.update((a, b) for a in xs for b in ys)
    return out


def chart_points(s, odd, n=24):
    """A barycentric lattice of points over a chart's triangle, corners and edges included, in cell-local texel-centre coordinates."""
    c = corner_local(s)[odd].astype(np.float64)
    pts = [(a * c[0] + b * c[1] + (n - a - b) * c[2]) / n for a in range(n + 1) for b in range(n + 1 - a)]
    return np.array(pts)


def interp_uv(rast, uv_corners, dtype):
    """mesh_raster.interpolate of per-corner uv (F, 3, 2) on a rast buffer (H, W, 4) in the device's order: w2 = (1 - u) - v,
    (u a0 + v a1) + w2 a2; -> (uv (H * W, 2) in `dtype`, covered (H * W,) bool)."""
    dt = dtype
    r = np.asarray(rast).reshape(-1, 4)
    fid = r[:, 3].astype(np.int64) - 1
    covered = fid >= 0
    a = np.asarray(uv_corners).astype(dt)[np.where(covered, fid, 0)]
    u, v = r[:, 0].astype(dt)[:, None], r[:, 1].astype(dt)[:, None]
    w2 = (dt(1) - u) - v
    return ((u * a[:, 0] + v * a[:, 1]) + w2 * a[:, 2]).astype(dt), covered
