"""Wavefront OBJ writer and reader for textured meshes (mesh_texture.py): name.obj + name.mtl (map_Kd) + name.png, the form Blender
and MeshLab open.  Standard library + numpy only; the PNG goes through png_io.

Conventions: this project's uv has its origin at the TOP-left texel corner (v = 0 is row 0 of the texture's memory, which is the top
row of the PNG: mesh_raster.texture's convention); OBJ's texture origin is the BOTTOM-left of the image, so the file holds
vt = (u, 1 - v) and the reader turns it back.  Positions are shared (V `v` lines); texture coordinates are per face corner (3F `vt`
lines, as mesh_texture's atlas gives every face its own chart): `f a/ta b/tb c/tc`, 1-based."""
import os

import numpy as np

from .png_io import read_png_host, write_png


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def texture_bytes(tex):
    """A texture as the (H, W, 3) uint8 image the writers store: uint8 as it is; floats as clamp(c, 0, 1) * 255 truncated -- the
    quantisation of ply_io's vertex colours."""
    t = _np(tex)
    if t.ndim == 4 and t.shape[0] == 1:
        t = t[0]
    if t.ndim != 3 or t.shape[2] != 3:
        raise ValueError(f"texture must be (H, W, 3), got {t.shape}")
    if t.dtype == np.uint8:
        return np.ascontiguousarray(t)
    return np.clip(t.astype(np.float32) * 255, 0, 255).astype(np.uint8)


def _checked(who, verts, faces, uv):
    v = np.ascontiguousarray(_np(verts), dtype=np.float32).reshape(-1, 3)
    f = np.asarray(_np(faces)).reshape(-1, 3).astype(np.int64)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"{who}: face index out of range")
    t = np.asarray(_np(uv), dtype=np.float32)
    if t.shape != (len(f), 3, 2):
        raise ValueError(f"{who}: uv must be ({len(f)}, 3, 2), one row per face corner, got {t.shape}")
    return v, f, t


def write_mesh_obj(path, verts, faces, uv, tex):
    """path: .../name.obj; also writes name.mtl and name.png beside it.  verts (V, 3), faces (F, 3), uv (F, 3, 2) per face corner with
    the origin top-left, tex (H, W, 3) uint8 or floats in [0, 1] (numpy arrays or tensors on any device).  -> [obj, mtl, png] paths."""
    v, f, t = _checked("write_mesh_obj", verts, faces, uv)
    stem = os.path.splitext(os.path.abspath(path))[0]
    name = os.path.basename(stem)
    os.makedirs(os.path.dirname(stem), exist_ok=True)
    write_png(stem + ".png", texture_bytes(tex))
    with open(stem + ".mtl", "w") as fh:
        fh.write(f"newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
    vt = t.reshape(-1, 2).astype(np.float64)
    lines = [f"mtllib {name}.mtl\nusemtl {name}\n"]
    lines += [f"v {p[0]:.9g} {p[1]:.9g} {p[2]:.9g}\n" for p in v]
    lines += [f"vt {q[0]:.9g} {1.0 - q[1]:.9g}\n" for q in vt]
    lines += [f"f {a + 1}/{3 * i + 1} {b + 1}/{3 * i + 2} {c + 1}/{3 * i + 3}\n" for i, (a, b, c) in enumerate(f)]
    with open(stem + ".obj", "w") as fh:
        fh.write("".join(lines))
    return [stem + ".obj", stem + ".mtl", stem + ".png"]


def read_mesh_obj(path):
    """-> (verts (V, 3) float32, faces (F, 3) int32, uv (F, 3, 2) float32 with the origin top-left, tex (H, W, 3) uint8) of a triangle
    OBJ whose every face entry is `a/ta` (or `a/ta/na`), with the texture its mtllib's map_Kd names; uv and tex are None when the file
    has no vt lines / no readable material.  ValueError with the line number for anything else."""
    verts, vts, faces, corners, mtllib = [], [], [], [], None
    with open(path, "r", errors="replace") as fh:
        for no, line in enumerate(fh, 1):
            tok = line.split()
            if not tok:
                continue
            try:
                if tok[0] == "v":
                    verts.append((float(tok[1]), float(tok[2]), float(tok[3])))
                elif tok[0] == "vt":
                    vts.append((float(tok[1]), float(tok[2])))
                elif tok[0] == "mtllib":
                    mtllib = line.split(None, 1)[1].strip()
                elif tok[0] == "f":
                    if len(tok) != 4:
                        raise ValueError("only triangles are supported")
                    ent = [e.split("/") for e in tok[1:]]
                    faces.append([int(e[0]) - 1 for e in ent])
                    if all(len(e) > 1 and e[1] for e in ent):
                        corners.append([int(e[1]) - 1 for e in ent])
            except (IndexError, ValueError) as e:
                raise ValueError(f"{path}:{no}: malformed line {line.strip()!r} ({e})") from None
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"{path}: face index out of range")
    uv = None
    if vts and len(corners) == len(faces):
        c = np.asarray(corners, np.int64).reshape(-1, 3)
        if c.size and (c.min() < 0 or c.max() >= len(vts)):
            raise ValueError(f"{path}: texture-coordinate index out of range")
        vt = np.asarray(vts, np.float64)
        uv = np.stack([vt[c, 0], 1.0 - vt[c, 1]], -1).astype(np.float32)
    tex = None
    if mtllib is not None:
        mtl = os.path.join(os.path.dirname(os.path.abspath(path)), mtllib)
        if os.path.exists(mtl):
            for line in open(mtl):
                if line.split()[:1] == ["map_Kd"]:
                    tex = read_png_host(os.path.join(os.path.dirname(mtl), line.split(None, 1)[1].strip()))[..., :3]
    return v, f, uv, tex
