"""A small Blender / D-NeRF scene written to a directory by the tests: transforms_train.json, transforms_test.json and RGBA PNGs
(encoded by tests/_png_ref.py with mixed filter types), whose poses are synthetic.make_camera's converted to OpenGL camera-to-world
matrices.  Every frame shows a shaded disc -- the silhouette of a ball at the origin, which all cameras look at -- over transparency."""
import json
import math
import os

import numpy as np

import _png_ref

FOVX = 0.6911


def frame_pixels(W, H, k, channels=4):
    """(H, W, channels) uint8 of frame k: an opaque, shaded, reddish disc with a soft rim on a transparent ground."""
    y, x = np.mgrid[0:H, 0:W]
    r = np.hypot(x - (W - 1) / 2, y - (H - 1) / 2) / (0.17 * W)
    alpha = np.clip((1.15 - r) / 0.3, 0.0, 1.0)
    shade = np.clip(1.0 - 0.5 * r, 0.0, 1.0)
    rgb = np.stack([230 * shade, 60 + 8 * k + 0 * r, 40 + 30 * np.sin(0.4 * x + k) ** 2], axis=2)
    px = np.concatenate([rgb, 255 * alpha[..., None]], axis=2)
    return np.clip(np.rint(px), 0, 255).astype(np.uint8)[..., :channels]


def poses(syn, n, W, H, start=0):
    return [syn.make_camera(W, H, azimuth=0.9 * (k + start) + 0.2, elevation=0.25 + 0.05 * ((k + start) % 3), fovx=FOVX,
                            fid=(k + start) / 10.0) for k in range(n)]


def opengl_c2w(cam):
    """The `transform_matrix` whose reading (flip y and z, invert) gives back cam's world-to-camera matrix."""
    c2w = np.linalg.inv(cam.world_view_transform.T.astype(np.float64))
    c2w[:3, 1:3] *= -1
    return c2w


def write_scene(root, syn, n_train=6, n_test=2, W=48, H=48, points=None, seed=0):
    """-> {"train": [(camera, pixels)], "test": [...]} of the scene written under `root`; points: (xyz float32 (N, 3),
    rgb uint8 (N, 3)) for a points3d.ply, or None for none."""
    rng = np.random.RandomState(seed)
    out = {}
    k0 = 0
    for split, n in (("train", n_train), ("test", n_test)):
        frames, items = [], []
        os.makedirs(os.path.join(root, split), exist_ok=True)
        for k, cam in enumerate(poses(syn, n, W, H, start=k0)):
            px = frame_pixels(W, H, k + k0)
            types = rng.randint(0, 5, H)
            types[:5] = [0, 1, 2, 3, 4][:min(5, H)]
            with open(os.path.join(root, split, f"r_{k:03d}.png"), "wb") as fh:
                fh.write(_png_ref.encode_png(px, types, idat_split=1 + k % 3))
            frames.append({"file_path": f"./{split}/r_{k:03d}", "time": cam.fid, "transform_matrix": opengl_c2w(cam).tolist()})
            items.append((cam, px))
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as fh:
            json.dump({"camera_angle_x": FOVX, "frames": frames}, fh)
        out[split] = items
        k0 += n
    if points is not None:
        xyz, rgb = points
        v = np.zeros(len(xyz), dtype=[(c, "<f4") for c in ("x", "y", "z", "nx", "ny", "nz")] + [(c, "u1") for c in ("red", "green", "blue")])
        for i, c in enumerate("xyz"):
            v[c] = xyz[:, i]
        for i, c in enumerate(("red", "green", "blue")):
            v[c] = rgb[:, i]
        head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
        head += [f"property float {c}" for c in ("x", "y", "z", "nx", "ny", "nz")] + [f"property uchar {c}" for c in ("red", "green", "blue")]
        with open(os.path.join(root, "points3d.ply"), "wb") as fh:
            fh.write(("\n".join(head + ["end_header"]) + "\n").encode("ascii") + v.tobytes())
    return out


def ball_points(n=2000, radius=0.45, seed=3):
    rng = np.random.RandomState(seed)
    d = rng.randn(n, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    xyz = (d * radius * rng.rand(n, 1) ** (1 / 3.0)).astype(np.float32)
    return xyz, np.full((n, 3), 128, np.uint8)
