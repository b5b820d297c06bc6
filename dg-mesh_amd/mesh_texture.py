"""Baking a mesh's appearance into a texture atlas, and the textured export (OBJ + MTL + PNG, or GLB).

An exported mesh carries one colour per vertex (evaluate.mesh_and_colors samples the appearance network at the vertices and nowhere
else), and mesh_simplify keeps one colour per cluster: a decimated mesh loses the appearance that was trained.  The appearance network
is a continuous function of position and time; bake() evaluates it once per texel of an atlas, so a 20 k-face mesh carries the colour
detail of the 1 M-face one.  The kernels are dgm_atlas_uv and dgm_atlas_interpolate of csrc/mesh_texture.hip;
looking the texture up again is mesh_raster.texture / render_mesh_textured.  The reference has no counterpart: it exports vertex
colours only.

The atlas is the trivial one -- one square cell per PAIR of faces, no parameterisation:
  * size = the texture's side (<= 16384), cell = s >= 4 texels, cells_per_row = size // s, L = s - 3;
  * faces 2c and 2c + 1 share cell c at cell column c % cells_per_row, cell row c // cells_per_row.  In texel-centre index coordinates
    local to the cell face 2c has its corners 0, 1, 2 at (0, 0), (L, 0), (0, L), face 2c + 1 at (s - 1, s - 1), (2, s - 1), (s - 1, 2);
    a corner at local (i, j) of cell (cx, cy) has u = (cx s + i + .5) / size, v alike (texel (i, j) is centred at ((i + .5) / size,
    (j + .5) / size), row 0 of memory at v = 0: mesh_raster.texture's convention);
  * local texel (i, j) belongs to face 2c when i + j <= s - 2 (b1 = i / L, b2 = j / L), to face 2c + 1 when i + j >= s
    (b1 = (s - 1 - i) / L, b2 = (s - 1 - j) / L), to nobody on the diagonal i + j = s - 1; b0 = 1 - b1 - b2;
  * the barycentrics are NOT clamped: the texels of a chart's bilinear footprint that lie outside the triangle hold the affine
    extrapolation, so bilinear sampling inside a chart is exact for anything affine over the face, a chart needs no dilation pass, and
    -- the footprints of a cell's two triangles being disjoint and inside the cell (tests/test_mesh_texture_host.py) -- no chart
    bleeds into another.  Sample such a texture with boundary_mode="clamp".
fp32 / int32, CUDA/HIP tensors only -- no CPU fallback.  Every output is identical bit for bit from run to run.

Deliberately out of scope:
  * mip-maps and uv_da: they need rast_db, which the rasterizer does not produce;
  * cube maps;
  * charts sized by face area: DiffMC and clustered meshes have near-uniform faces, so uniform cells are the honest first form;
  * seams: there are none to hide, each face is its own chart (minified far below one texel per cell, neighbouring charts do mix);
  * any glTF feature beyond glb_io's docstring.  The glTF files are not checked against an external loader: none was available.

bake_ambient_occlusion() bakes the mesh's self-shadowing into the same atlas by ray casting (mesh_ray.py);
TextureSpec(ao_samples=N) and --ao N multiply the colour texture by it, so that an exported mesh does not look flat in a viewer that
does not light it.

Command line: python -m dgmesh_amd.mesh_texture in.ply out.obj|out.glb (--size N | --cell S) [--ao N] bakes a PLY's vertex colours."""
import argparse
import math
import os
from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch

from . import _lib, mesh_args

MAX_SIZE = 16384
MIN_CELL = 4
FORMATS = ("obj", "glb")


class Atlas(NamedTuple):
    size: int
    cell: int
    cells_per_row: int
    n_faces: int


@dataclass(frozen=True)
class TextureSpec:
    """The parameters of the textured export: the atlas (size, or cell when given), the file format and ao_samples -- 0: the colour
    texture as baked; > 0: multiplied by the ambient occlusion of that many rays per texel (bake_ambient_occlusion)."""
    size: Optional[int] = 2048
    cell: Optional[int] = None
    format: str = "obj"
    ao_samples: int = 0

    def describe(self):
        return ((f"cell {int(self.cell)}" if self.cell is not None else f"size {int(self.size)}") + f" format {self.format}"
                + (f" ao {int(self.ao_samples)}" if self.ao_samples else ""))

    def atlas_args(self):
        return {"cell": self.cell} if self.cell is not None else {"size": self.size}


def as_spec(texture):
    """None, a TextureSpec or a dict of its fields -> TextureSpec or None ("do nothing")."""
    spec = mesh_args.spec_of("mesh_texture", "texture", TextureSpec, texture)
    if spec is not None and spec.format not in FORMATS:
        raise ValueError(f"mesh_texture: format must be one of {', '.join(FORMATS)}, got {spec.format!r}")
    if spec is not None and int(spec.ao_samples) < 0:
        raise ValueError(f"mesh_texture: ao_samples must be >= 0, got {spec.ao_samples}")
    return spec


def build_atlas(n_faces, *, size=None, cell=None):
    """The atlas of n_faces faces from exactly one of size (then cell = size // ceil(sqrt(ceil(F / 2)))) and cell (then
    size = cell * ceil(sqrt(ceil(F / 2)))).  ValueError: both or neither given, a cell below 4, a size above 16384."""
    F = int(n_faces)
    if F < 0:
        raise ValueError(f"build_atlas: n_faces must be >= 0, got {n_faces}")
    if (size is None) == (cell is None):
        raise ValueError("build_atlas: give exactly one of size and cell")
    pairs = (F + 1) // 2
    per_row = math.isqrt(pairs - 1) + 1 if pairs else 1  # ceil(sqrt(ceil(F / 2))), in integers
    if size is not None:
        size = int(size)
        if not 1 <= size <= MAX_SIZE:
            raise ValueError(f"build_atlas: size must be within [1, {MAX_SIZE}], got {size}")
        cell = size // per_row
    else:
        cell = int(cell)
        size = cell * per_row
    if cell < MIN_CELL:
        raise ValueError(f"build_atlas: {F} faces leave a cell of {cell} texels at size {size}, below the smallest cell {MIN_CELL}: "
                         f"decimate first (simplify=) or use a larger size (>= {MIN_CELL * per_row})")
    if size > MAX_SIZE:
        raise ValueError(f"build_atlas: {F} faces at cell {cell} need a texture of {size} texels a side, above {MAX_SIZE}: "
                         "decimate first (simplify=) or use a smaller cell")
    return Atlas(size, cell, size // cell, F)


def atlas_uv(atlas, device):
    """The per-corner texture coordinates (F, 3, 2) of the atlas, on `device` (dgm_atlas_uv)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("mesh_texture.atlas_uv needs a CUDA/HIP device (dg-mesh_amd has no CPU path)")
    uv = torch.empty((atlas.n_faces, 3, 2), dtype=torch.float32, device=device)
    with _lib.device_guard(device):
        _lib.check(_lib.lib().dgm_atlas_uv(atlas.n_faces, atlas.size, atlas.cell, _lib.vp(uv), _lib.stream_ptr()))
    return uv


def atlas_interpolate(atlas, attr, faces):
    """attr (V, C) interpolated into every texel of the atlas (dgm_atlas_interpolate): (out (size, size, C), face_id (size, size)
    int32) -- the unclamped affine interpolation over the owning face and its id; zeros and -1 on the unowned texels (module
    docstring; a face with an index outside [0, V) owns nothing)."""
    for t in (attr, faces):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("mesh_texture.atlas_interpolate needs CUDA/HIP tensors (dg-mesh_amd has no CPU path)")
    if attr.dtype != torch.float32 or faces.dtype != torch.int32:
        raise RuntimeError(f"mesh_texture.atlas_interpolate: attr must be float32 and faces int32, got {attr.dtype} and {faces.dtype}")
    if attr.dim() != 2 or attr.shape[1] < 1 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"mesh_texture.atlas_interpolate: attr must be (V, C) and faces (F, 3), got {tuple(attr.shape)} and {tuple(faces.shape)}")
    if int(faces.shape[0]) != atlas.n_faces:
        raise ValueError(f"mesh_texture.atlas_interpolate: the atlas was built for {atlas.n_faces} faces, got {int(faces.shape[0])}")
    if attr.device != faces.device:
        raise ValueError(f"mesh_texture.atlas_interpolate: attr on {attr.device}, faces on {faces.device}")
    attr, faces = attr.detach().contiguous(), faces.detach().contiguous()
    V, C = int(attr.shape[0]), int(attr.shape[1])
    out = torch.empty((atlas.size, atlas.size, C), dtype=torch.float32, device=attr.device)
    face_id = torch.empty((atlas.size, atlas.size), dtype=torch.int32, device=attr.device)
    with _lib.device_guard(attr.device):
        _lib.check(_lib.lib().dgm_atlas_interpolate(V, atlas.n_faces, C, atlas.size, atlas.cell, _lib.vp(attr), _lib.vp(faces), _lib.vp(out), _lib.vp(face_id),
                                                    _lib.stream_ptr()))
    return out, face_id


def bake(verts, faces, color_fn, *, size=None, cell=None, chunk=1 << 18):
    """Evaluates color_fn once per owned texel: (tex (size, size, 3), uv (F, 3, 2), atlas).  The texels' positions are
    atlas_interpolate(verts); color_fn(points (n, 3)) -> (n, 3) is called on the owned texels only, `chunk` at a time, and its colours
    are clamped to [0, 1]; unowned texels stay 0.  One read-back (the number of owned texels)."""
    atlas = build_atlas(int(faces.shape[0]), size=size, cell=cell)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"mesh_texture.bake: chunk must be >= 1, got {chunk}")
    pos, face_id = atlas_interpolate(atlas, verts, faces)
    owned = (face_id.reshape(-1) >= 0).nonzero().reshape(-1)
    points = pos.reshape(-1, 3)[owned]
    tex = torch.zeros((atlas.size * atlas.size, 3), dtype=torch.float32, device=pos.device)
    for lo in range(0, int(owned.shape[0]), chunk):
        colour = color_fn(points[lo:lo + chunk])
        if colour.shape != (min(chunk, int(owned.shape[0]) - lo), 3):
            raise ValueError(f"mesh_texture.bake: color_fn must return (n, 3), got {tuple(colour.shape)}")
        tex[owned[lo:lo + chunk]] = colour.detach().to(torch.float32).clamp(0.0, 1.0)
    return tex.reshape(atlas.size, atlas.size, 3), atlas_uv(atlas, pos.device), atlas


def bake_vertex_colors(verts, faces, colors, *, size=None, cell=None):
    """The texture that holds the vertex colours themselves: atlas_interpolate of `colors` (V, 3), unclamped (a chart's extrapolated
    texels must stay affine): (tex, uv, atlas).  `verts` is only checked against `colors`."""
    if tuple(colors.shape) != (int(verts.shape[0]), 3):
        raise ValueError(f"mesh_texture.bake_vertex_colors: colors must be ({int(verts.shape[0])}, 3), got {tuple(colors.shape)}")
    atlas = build_atlas(int(faces.shape[0]), size=size, cell=cell)
    tex, _ = atlas_interpolate(atlas, colors, faces)
    return tex, atlas_uv(atlas, tex.device), atlas


def bake_ambient_occlusion(verts, faces, *, size=None, cell=None, samples=64, max_dist=math.inf, offset=None, seed=0, flip=False,
                           accel="auto"):
    """The ambient occlusion of the mesh per texel of its atlas: (tex (size, size, 1), uv (F, 3, 2), atlas).  Per owned texel the
    position is atlas_interpolate(verts) and the normal the unit (v1 - v0) x (v2 - v0) of the owning face (negated with flip, for a
    mesh wound inwards); the value is mesh_ray.ambient_occlusion there (samples, max_dist, offset, seed as it takes them), the texel
    counting as point number "its rank among the owned texels".  Unowned texels and texels of a face without area hold 1, so that
    multiplying a colour texture by this one changes nothing there.  One read-back (the number of owned texels)."""
    from . import mesh_ray
    atlas = build_atlas(int(faces.shape[0]), size=size, cell=cell)
    pos, face_id = atlas_interpolate(atlas, verts, faces)
    verts, faces = verts.detach().contiguous(), faces.contiguous()
    owned = (face_id.reshape(-1) >= 0).nonzero().reshape(-1)
    points = pos.reshape(-1, 3)[owned].contiguous()
    corner = verts[faces[face_id.reshape(-1)[owned].long()].long()]  # (n, 3, 3)
    normal = torch.linalg.cross(corner[:, 1] - corner[:, 0], corner[:, 2] - corner[:, 0])
    if flip:
        normal = -normal
    held = accel if not (isinstance(accel, str) and accel == "auto") else mesh_ray._resolve("bake_ambient_occlusion", verts, faces, accel)[2]
    ao = mesh_ray.ambient_occlusion(points, normal.contiguous(), verts, faces, samples, max_dist, offset, seed, held)
    ao = torch.where(normal.abs().sum(dim=1) > 0, ao, torch.ones_like(ao))
    tex = torch.ones(atlas.size * atlas.size, dtype=torch.float32, device=pos.device)
    tex[owned] = ao
    return tex.reshape(atlas.size, atlas.size, 1), atlas_uv(atlas, pos.device), atlas


def apply_ambient_occlusion(tex, verts, faces, spec_or_samples, *, size=None, cell=None, **kwargs):
    """tex (size, size, 3) times bake_ambient_occlusion of the same atlas; tex itself when the sample count is 0."""
    samples = int(getattr(spec_or_samples, "ao_samples", spec_or_samples))
    if samples <= 0:
        return tex
    ao = bake_ambient_occlusion(verts, faces, size=size, cell=cell, samples=samples, **kwargs)[0]
    if tuple(ao.shape[:2]) != tuple(tex.shape[:2]):
        raise ValueError(f"mesh_texture.apply_ambient_occlusion: the texture is {tuple(tex.shape)}, the atlas gives {tuple(ao.shape)}")
    return tex * ao


def appearance_color_fn(mesh, deform_back, fid):
    """The colour of evaluate.mesh_and_colors at arbitrary points: points -> mesh.appearance.step(points + deform_back.step(points, t)[0], t)
    with t the one-element tensor `fid` repeated per point."""
    def color_fn(points):
        t = fid.reshape(1, 1).expand(points.shape[0], -1)
        return mesh.appearance.step(points + deform_back.step(points, t)[0], t)
    return color_fn


def write_textured(path_stem, fmt, verts, faces, uv, tex):
    """name.obj (+ .mtl, .png) or name.glb at path_stem: the path written."""
    if fmt == "obj":
        from .obj_io import write_mesh_obj
        return write_mesh_obj(path_stem + ".obj", verts, faces, uv, tex)[0]
    from .glb_io import write_mesh_glb
    return write_mesh_glb(path_stem + ".glb", verts, faces, uv=uv, tex=tex)


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m dgmesh_amd.mesh_texture",
                                 description="Bake a triangle-mesh PLY's vertex colours into a texture atlas on the GPU; write OBJ + MTL + PNG or GLB.")
    ap.add_argument("input")
    ap.add_argument("output", help="out.obj (with out.mtl and out.png beside it) or out.glb")
    group = ap.add_mutually_exclusive_group(required=True)
    group.add_argument("--size", type=int, help="the texture's side in texels")
    group.add_argument("--cell", type=int, help="texels a side per pair of faces (>= 4)")
    ap.add_argument("--ao", type=int, default=0, metavar="N", help="multiply the texture by the ambient occlusion of N rays per texel (0: none)")
    return ap


def main(argv=None):
    from .ply_io import read_mesh_ply_on_device
    args = build_parser().parse_args(argv)
    stem, ext = os.path.splitext(args.output)
    if ext.lower() not in (".obj", ".glb"):
        raise SystemExit(f"mesh_texture: the output must end in .obj or .glb, got {args.output}")
    verts, faces, colors = read_mesh_ply_on_device(args.input, torch.device("cuda"))
    if colors is None:
        raise SystemExit(f"mesh_texture: {args.input} has no vertex colours to bake")
    if args.ao < 0:
        raise SystemExit(f"mesh_texture: --ao must be >= 0, got {args.ao}")
    tex, uv, atlas = bake_vertex_colors(verts, faces, colors, size=args.size, cell=args.cell)
    tex = apply_ambient_occlusion(tex, verts, faces, args.ao, size=args.size, cell=args.cell)
    out = write_textured(stem, ext.lower()[1:], verts, faces, uv, tex)
    print(f"mesh_texture: V {len(verts)} F {len(faces)}  size {atlas.size} cell {atlas.cell}  -> {out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
