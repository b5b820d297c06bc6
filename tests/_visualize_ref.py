"""Plain numpy restatement of the passes of dg-mesh_amd/visualize.py (csrc/visualize.hip) and of its pose conversion.  Every float
pass takes `dtype`: np.float64 is the reference the GPU tests compare against, np.float32 is the same formulas with every
intermediate rounded to float32 -- the GPU tests take their tolerance from the distance between the two (tolerance()), never from
the kernel's output.  The integer-valued passes (splat, compose) are restated in float32 with the kernel's operation order: every
operation in them is a single correctly rounded IEEE operation, so they are expected to match bit for bit.  No HIP, no torch."""
import numpy as np

MATERIAL = dict(ambient=0.5, diffuse=0.3, specular=0.2 * 0.2, shininess=10.0, base_color=(1.0, 1.0, 1.0))


def tolerance(f32, f64, floor=1e-6):
    """4 x the largest deviation of the float32 restatement from the float64 one, at least `floor`."""
    dev = float(np.abs(np.asarray(f32, np.float64) - np.asarray(f64, np.float64)).max()) if np.size(f64) else 0.0
    return max(4.0 * dev, floor), dev


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _unit_or_zero(n, dtype):
    length = np.sqrt(_dot(n, n))
    ok = length >= dtype(1e-6)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ok[..., None], n / np.where(ok, length, dtype(1))[..., None], dtype(0)).astype(dtype)


def vertex_normals(verts, faces, dtype=np.float64):
    """Area-weighted vertex normals: cross(v1 - v0, v2 - v0) of every face with all indices in [0, V) added to its three vertices,
    normalised; length < 1e-6 -> 0."""
    v = np.asarray(verts, dtype)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(v)
    f = f[((f >= 0) & (f < V)).all(1)]
    a, b = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    acc = np.zeros((V, 3), dtype)
    for k in range(3):
        np.add.at(acc, f[:, k], n)
    return _unit_or_zero(acc, dtype)


def headlight(verts, camera_center, dtype=np.float64):
    d = np.asarray(camera_center, dtype) - np.asarray(verts, dtype).mean(0, dtype=dtype)
    return (d / np.sqrt(_dot(d, d))).astype(dtype)


def shade(verts, normals, faces, rast, light_dir, camera_center, dtype=np.float64, background=(1.0, 1.0, 1.0), normal_sign=1.0,
          clamp=True, **material):
    """The hard-Phong pass over rast (H, W, 4) = (u, v, z/w, id + 1): (H, W, 3).  light_dir: unit vector towards the light.
    clamp=False returns the colour before the clamp to [0, 1]."""
    m = dict(MATERIAL, **material)
    v, nv = np.asarray(verts, dtype), np.asarray(normals, dtype)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    r = np.asarray(rast, dtype).reshape(rast.shape[-3], rast.shape[-2], 4)
    V, F = len(v), len(f)
    ident = np.asarray(rast).reshape(r.shape)[..., 3].astype(np.int64)
    covered = (ident >= 1) & (ident <= F)
    t = f[np.clip(ident - 1, 0, max(F - 1, 0))] if F else np.zeros(ident.shape + (3,), np.int64)
    covered &= ((t >= 0) & (t < V)).all(-1)
    t = np.clip(t, 0, max(V - 1, 0))
    u, w1 = r[..., 0:1], r[..., 1:2]
    w2 = dtype(1) - u - w1
    lerp = lambda a: (u * a[t[..., 0]] + w1 * a[t[..., 1]]) + w2 * a[t[..., 2]]
    pos, n = lerp(v), _unit_or_zero(lerp(nv) * dtype(normal_sign), dtype)
    l, c = np.asarray(light_dir, dtype), np.asarray(camera_center, dtype)
    ndl = _dot(n, l)
    diffuse = np.maximum(ndl, dtype(0))
    refl = (dtype(2) * ndl)[..., None] * n - l
    view = c - pos
    vlen = np.sqrt(_dot(view, view))
    with np.errstate(divide="ignore", invalid="ignore"):
        view = view / vlen[..., None]
        vdr = np.maximum(_dot(view, refl), dtype(0))
        spec = np.where((ndl > 0) & (vlen > 0), np.power(vdr, dtype(m["shininess"])), dtype(0)).astype(dtype)
    lit = dtype(m["ambient"]) + dtype(m["diffuse"]) * diffuse
    col = lit[..., None] * np.asarray(m["base_color"], dtype) + (dtype(m["specular"]) * spec)[..., None]
    if clamp:
        col = np.clip(col, dtype(0), dtype(1))
    return np.where(covered[..., None], col, np.asarray(background, dtype)).astype(dtype)


def screen(pos_clip, H, W, dtype=np.float32):
    p = np.asarray(pos_clip, dtype).reshape(-1, 4)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sx = (p[:, 0] / p[:, 3] + dtype(1)) * (dtype(0.5) * dtype(W))
        sy = (p[:, 1] / p[:, 3] + dtype(1)) * (dtype(0.5) * dtype(H))
        zw = p[:, 2] / p[:, 3]
    return sx, sy, zw


def splat_ids(pos_clip, H, W, size=1):
    """(H, W) int64: the id of the point that wins each pixel (smallest z/w, ties to the lower id), -1 where none lands.  float32
    with the kernel's operations."""
    p = np.asarray(pos_clip, np.float32).reshape(-1, 4)
    sx, sy, zw = screen(p, H, W)
    ok = (p[:, 3] > 0) & np.isfinite(p).all(1) & np.isfinite(sx) & np.isfinite(sy) & np.isfinite(zw)
    half = size // 2
    with np.errstate(invalid="ignore"):
        fx, fy = np.floor(sx), np.floor(sy)
        ok &= (fx >= -half) & (fx <= W - 1 + half) & (fy >= -half) & (fy <= H - 1 + half)
    idx = np.nonzero(ok)[0]
    cx, cy = fx[idx].astype(np.int64), fy[idx].astype(np.int64)
    bits = zw[idx].view(np.uint32).astype(np.uint64)
    ordered = np.where(bits & np.uint64(0x80000000), ~bits & np.uint64(0xFFFFFFFF), bits | np.uint64(0x80000000))
    key = (ordered << np.uint64(32)) | idx.astype(np.uint64)
    keys = np.full(H * W, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    for dy in range(-half, half + 1):
        for dx in range(-half, half + 1):
            x, y = cx + dx, cy + dy
            inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            np.minimum.at(keys, (y * W + x)[inside], key[inside])
    ids = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ids[keys == np.uint64(0xFFFFFFFFFFFFFFFF)] = -1
    return ids.reshape(H, W)


def splat_image(ids, colors=None, color=(0.0, 0.0, 1.0), background=(1.0, 1.0, 1.0)):
    img = np.empty(ids.shape + (3,), np.float32)
    img[:] = np.asarray(background, np.float32)
    hit = ids >= 0
    img[hit] = np.asarray(colors, np.float32)[ids[hit]] if colors is not None else np.asarray(color, np.float32)
    return img


def compose(panels, downsample=1, dtype=np.float32):
    """panels: arrays (3, H, W) or (H, W, 3) -> uint8 (H/d, n W/d, 3): the 2x2 average ((a + b) + (c + d)) * 0.25 (top row first),
    clamp to [0, 1] (NaN -> 0), x 255, truncated."""
    out = []
    for p in panels:
        p = np.asarray(p, dtype)
        if p.shape[2] != 3:
            p = np.transpose(p, (1, 2, 0))
        if downsample == 2:
            p = ((p[0::2, 0::2] + p[0::2, 1::2]) + (p[1::2, 0::2] + p[1::2, 1::2])) * dtype(0.25)
        with np.errstate(invalid="ignore"):
            q = np.where(np.isnan(p), dtype(0), np.minimum(np.maximum(p, dtype(0)), dtype(1))) * dtype(255)
        out.append(np.trunc(q).astype(np.uint8))
    return np.concatenate(out, axis=1)


# ---- poses ---------------------------------------------------------------------------------------------------------------------------
def trajectory_poses(radius, elevation, total_frames, look_at=(0.0, 0.0, 0.0)):
    """(n, 4, 4) float64 OpenGL camera-to-world: columns right, up, -forward, eye; eye = (r sin th, -r cos th, elevation)."""
    out = []
    r = np.sqrt(radius ** 2 - elevation ** 2)
    for i in range(total_frames):
        th = 2 * np.pi * i / total_frames
        eye = np.array([r * np.sin(th), -r * np.cos(th), elevation], np.float64)
        fwd = np.asarray(look_at, np.float64) - eye
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, [0.0, 0.0, 1.0])
        right /= np.linalg.norm(right)
        up = np.cross(right, fwd)
        up /= np.linalg.norm(up)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, up, -fwd, eye
        out.append(m)
    return np.stack(out)


def world_view_from_pose(c2w_gl):
    """world_view_transform (= W2C^T, camera axes +x right, +y down, +z forward) of an OpenGL camera-to-world pose, float64."""
    c2w = np.array(c2w_gl, np.float64)
    c2w[:3, 1] *= -1
    c2w[:3, 2] *= -1
    return np.linalg.inv(c2w).T


def project_pixels(full_proj_transform, W, H, point):
    """Screen position (pixels, the rasterizer's mapping) of a world point under a full_proj_transform (row-vector convention)."""
    h = np.append(np.asarray(point, np.float64), 1.0) @ np.asarray(full_proj_transform, np.float64)
    return (h[0] / h[3] + 1.0) * W / 2, (h[1] / h[3] + 1.0) * H / 2
