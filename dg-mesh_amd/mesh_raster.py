"""Differentiable triangle rasterizer with the call shapes of nvdiffrast.torch (the reference's mesh renderer,
R/utils/renderer.py:33-121; R/ = the reference's dgmesh/):

    rasterize(glctx, pos, tri, resolution)   -> (rast (1, H, W, 4), None)
    interpolate(attr, rast, tri)             -> (out (1, H, W, C), None)
    antialias(color, rast, pos, tri)         -> out (1, H, W, C)
    texture(tex, uv, ...)                    -> out (1, H, W, C)

so a caller of nvdiffrast.torch can switch imports.  `glctx` is accepted and ignored (None is fine).  The passes are HIP kernels
of libdgmesh_hip (csrc/mesh_raster.hip) behind torch.autograd.Function.  float32 / int32, CUDA/HIP tensors only, batch size 1 --
no CPU fallback; anything else raises.

Conventions chosen here (nvdiffrast is not vendored, so they are this project's, matched to nvdiffrast's documented ones where
that costs nothing):
  * pos (1, V, 4) clip space, tri (F, 3) int32, F < 2^24 (the id is stored as a float); resolution (H, W);
  * screen s = ((x/w + 1) W/2, (y/w + 1) H/2) in pixels, pixel (px, py) centred at (px + .5, py + .5), row 0 at NDC y = -1 -- as
    nvdiffrast, and as the Gaussian rasterizer's ndc2Pix (centres at integers, s - .5): clip_positions(cam, verts) puts mesh and
    Gaussians on the same pixels with no row flip (the reference flips because it builds a GL projection from K);
  * a face with a vertex at w <= 0 is dropped (nvdiffrast clips it; DG-Mesh's cameras never meet one), as is a face with an index
    outside [0, V) or zero screen area; no back-face culling;
  * coverage: the three edge functions, each evaluated with its endpoints in ascending vertex-id order, oriented by the sign of the
    triangle's screen area, all >= 0 (inclusive edges: faces sharing an edge see exactly negated values, so a closed mesh has no
    cracks);
  * depth z/w, linear in screen space; the smaller wins, ties to the lower face id (one 64-bit atomicMin per covered centre on
    (ordered z/w bits, id): the forward is bit-reproducible);
  * rast = (u, v, z/w, id + 1), zeros on background; (u, v) perspective-correct barycentrics of vertices 0 and 1, so an attribute
    interpolates as u a0 + v a1 + (1 - u - v) a2.  Gradients flow from rast[..., 0:2] to pos (x, y, w); z/w and id are not
    differentiable; no rast_db;
  * antialias: for every horizontal / vertical pair of neighbouring pixels with different ids, the front pixel (smaller z/w;
    background farthest) and its face T; the first silhouette edge of T (one face; two faces whose third vertices lie on the
    same screen side; more than two faces) whose line crosses the segment between the centres -- horizontal pairs consider only
    edges with |ds_y| >= |ds_x|, vertical pairs the others -- at distance t from the front centre: t > .5 adds
    (t - .5)(c_front - c_other) to the other pixel, t < .5 adds (.5 - t)(c_other - c_front) to the front pixel.  Exact for an
    axis-aligned straight edge; it reproduces coverage along each row and column.  The only path from a mask loss to the
    geometry.  The edge topology is rebuilt on the device every call (DiffMC's faces change every step);
  * float atomics only in the backward scatters (dpos, dattr): those agree to rounding run to run; every forward output is
    bit-identical run to run;
  * texture: tex (1, Ht, Wt, C), uv (1, ..., 2); texel (i, j) is centred at u = (i + .5) / Wt, v = (j + .5) / Ht and row 0 of memory is
    at v = 0 (nvdiffrast's documented convention).  filter_mode "linear" (= "auto"): bilinear over the four texels around
    (u Wt - .5, v Ht - .5); "nearest": texel (floor(u Wt), floor(v Ht)).  boundary_mode "wrap": indices modulo the size; "clamp":
    indices clamped; "zero": texels outside count as 0.  A non-finite uv gives zeros and no gradient; a finite uv of any magnitude
    reads nothing outside tex.  Gradients to tex (fp32 atomics, as dattr) and to uv (zero for "nearest").  csrc/mesh_texture.hip
    states the operation order.
Not provided: MSAA, mip-maps (uv_da, mip_level_bias, mip, max_mip_level, the linear-mipmap filters: they need rast_db), cube maps,
rast_db, depth peeling, range mode, batches larger than 1.
"""

import torch

from . import _lib


def _st():
    return _lib.stream_ptr()


def _need(name, t, what, dtype):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: {what} must be a CUDA/HIP tensor (dg-mesh_amd has no CPU path)")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: {what} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: {what} must be contiguous")


def _check_pos_tri(name, pos, tri):
    _need(name, pos, "pos", torch.float32)
    _need(name, tri, "tri", torch.int32)
    if pos.dim() != 3 or pos.shape[2] != 4:
        raise RuntimeError(f"{name}: pos must be (1, V, 4) clip-space positions, got {tuple(pos.shape)}")
    if pos.shape[0] != 1:
        raise RuntimeError(f"{name}: only batch size 1 is supported, got pos {tuple(pos.shape)}")
    if tri.dim() != 2 or tri.shape[1] != 3:
        raise RuntimeError(f"{name}: tri must be (F, 3), got {tuple(tri.shape)}")
    if tri.shape[0] >= 1 << 24:
        raise RuntimeError(f"{name}: {tri.shape[0]} faces; at most 2^24 - 1 (the id is stored as a float in rast)")
    if tri.device != pos.device:
        raise RuntimeError(f"{name}: pos and tri must be on one device")


def _check_rast(name, rast, dev):
    _need(name, rast, "rast", torch.float32)
    if rast.dim() != 4 or rast.shape[0] != 1 or rast.shape[3] != 4:
        raise RuntimeError(f"{name}: rast must be (1, H, W, 4), got {tuple(rast.shape)}")
    if rast.device != dev:
        raise RuntimeError(f"{name}: rast must be on the device of the other inputs")


class _Rasterize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, tri, H, W):
        L = _lib.lib()
        V, F = int(pos.shape[1]), int(tri.shape[0])
        dev = pos.device
        scratch = torch.empty(int(L.dgm_tri_raster_scratch_bytes(F, H, W)), dtype=torch.uint8, device=dev)
        rast = torch.empty((1, H, W, 4), dtype=torch.float32, device=dev)
        with _lib.device_guard(dev):
            _lib.check(L.dgm_tri_rasterize_forward(V, F, H, W, _lib.vp(pos), _lib.vp(tri), _lib.vp(scratch), _lib.vp(rast), _st()))
        ctx.save_for_backward(pos, tri, rast)
        return rast

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, drast):
        pos, tri, rast = ctx.saved_tensors
        V, F = int(pos.shape[1]), int(tri.shape[0])
        H, W = int(rast.shape[1]), int(rast.shape[2])
        drast = drast.contiguous().float()
        dpos = torch.empty_like(pos)
        with _lib.device_guard(pos.device):
            _lib.check(_lib.lib().dgm_tri_rasterize_backward(V, F, H, W, _lib.vp(pos), _lib.vp(tri), _lib.vp(rast), _lib.vp(drast), _lib.vp(dpos), _st()))
        return dpos, None, None, None


class _Interpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr, rast, tri):
        L = _lib.lib()
        V, C = int(attr.shape[0]), int(attr.shape[1])
        F = int(tri.shape[0])
        H, W = int(rast.shape[1]), int(rast.shape[2])
        out = torch.empty((1, H, W, C), dtype=torch.float32, device=attr.device)
        with _lib.device_guard(attr.device):
            _lib.check(L.dgm_tri_interpolate_forward(V, F, H, W, C, _lib.vp(attr), _lib.vp(rast), _lib.vp(tri), _lib.vp(out), _st()))
        ctx.save_for_backward(attr, rast, tri)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        attr, rast, tri = ctx.saved_tensors
        V, C = int(attr.shape[0]), int(attr.shape[1])
        F = int(tri.shape[0])
        H, W = int(rast.shape[1]), int(rast.shape[2])
        dout = dout.contiguous().float()
        dattr = torch.empty_like(attr)
        drast = torch.empty_like(rast)
        with _lib.device_guard(attr.device):
            _lib.check(_lib.lib().dgm_tri_interpolate_backward(V, F, H, W, C, _lib.vp(attr), _lib.vp(rast), _lib.vp(tri), _lib.vp(dout), _lib.vp(dattr),
                                                               _lib.vp(drast), _st()))
        return dattr, drast, None


class _Antialias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, rast, pos, tri):
        L = _lib.lib()
        V, F = int(pos.shape[1]), int(tri.shape[0])
        H, W, C = int(color.shape[1]), int(color.shape[2]), int(color.shape[3])
        dev = color.device
        scratch = torch.empty(int(L.dgm_tri_aa_scratch_bytes(F)), dtype=torch.uint8, device=dev)
        out = torch.empty_like(color)
        with _lib.device_guard(dev):
            _lib.check(L.dgm_tri_antialias_forward(V, F, H, W, C, _lib.vp(color), _lib.vp(rast), _lib.vp(pos), _lib.vp(tri), _lib.vp(scratch), _lib.vp(out),
                                                   _st()))
        ctx.save_for_backward(color, rast, pos, tri, scratch)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        color, rast, pos, tri, scratch = ctx.saved_tensors
        V, F = int(pos.shape[1]), int(tri.shape[0])
        H, W, C = int(color.shape[1]), int(color.shape[2]), int(color.shape[3])
        dout = dout.contiguous().float()
        dcolor = torch.empty_like(color)
        dpos = torch.empty_like(pos)
        with _lib.device_guard(color.device):
            _lib.check(_lib.lib().dgm_tri_antialias_backward(V, F, H, W, C, _lib.vp(color), _lib.vp(rast), _lib.vp(pos), _lib.vp(tri), _lib.vp(scratch),
                                                             _lib.vp(dout), _lib.vp(dcolor), _lib.vp(dpos), _st()))
        return dcolor, None, dpos, None


FILTER_MODES = ("nearest", "linear")          # the int of the C ABI is the index
BOUNDARY_MODES = ("wrap", "clamp", "zero")    # likewise


class _Texture(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, uv, filt, boundary):
        Ht, Wt, C = int(tex.shape[1]), int(tex.shape[2]), int(tex.shape[3])
        n = uv.numel() // 2
        out = torch.empty(tuple(uv.shape[:-1]) + (C,), dtype=torch.float32, device=tex.device)
        with _lib.device_guard(tex.device):
            _lib.check(_lib.lib().dgm_tri_texture_forward(n, Ht, Wt, C, filt, boundary, _lib.vp(tex), _lib.vp(uv), _lib.vp(out), _st()))
        ctx.save_for_backward(tex, uv)
        ctx.modes = (filt, boundary)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        tex, uv = ctx.saved_tensors
        filt, boundary = ctx.modes
        Ht, Wt, C = int(tex.shape[1]), int(tex.shape[2]), int(tex.shape[3])
        n = uv.numel() // 2
        dout = dout.contiguous().float()
        dtex = torch.empty_like(tex)
        duv = torch.empty_like(uv)
        with _lib.device_guard(tex.device):
            _lib.check(_lib.lib().dgm_tri_texture_backward(n, Ht, Wt, C, filt, boundary, _lib.vp(tex), _lib.vp(uv), _lib.vp(dout), _lib.vp(dtex), _lib.vp(duv),
                                                           _st()))
        return dtex, duv, None, None


def rasterize(glctx, pos, tri, resolution, ranges=None, grad_db=True):
    """nvdiffrast.torch.rasterize for batch size 1: (rast (1, H, W, 4) = (u, v, z/w, id + 1), None).  `glctx` and `grad_db` are
    ignored; `ranges` (range mode) is not supported."""
    _check_pos_tri("rasterize", pos, tri)
    if ranges is not None:
        raise RuntimeError("rasterize: range mode is not supported")
    H, W = (int(r) for r in resolution)
    if not (0 < H <= 16384 and 0 < W <= 16384):
        raise RuntimeError(f"rasterize: resolution must be within [1, 16384]^2, got {(H, W)}")
    return _Rasterize.apply(pos, tri, H, W), None


def interpolate(attr, rast, tri, rast_db=None, diff_attrs=None):
    """nvdiffrast.torch.interpolate for batch size 1: attr (V, C) or (1, V, C) -> (out (1, H, W, C), None), zeros on background.
    `rast_db` / `diff_attrs` (attribute derivatives) are not supported."""
    if rast_db is not None or diff_attrs is not None:
        raise RuntimeError("interpolate: attribute derivatives (rast_db, diff_attrs) are not supported")
    _need("interpolate", attr, "attr", torch.float32)
    _need("interpolate", tri, "tri", torch.int32)
    if attr.dim() == 3:
        if attr.shape[0] != 1:
            raise RuntimeError(f"interpolate: only batch size 1 is supported, got attr {tuple(attr.shape)}")
        attr = attr[0]
    if attr.dim() != 2 or attr.shape[1] < 1:
        raise RuntimeError(f"interpolate: attr must be (V, C) or (1, V, C) with C >= 1, got {tuple(attr.shape)}")
    if tri.dim() != 2 or tri.shape[1] != 3 or tri.shape[0] >= 1 << 24:
        raise RuntimeError(f"interpolate: tri must be (F, 3) with F < 2^24, got {tuple(tri.shape)}")
    _check_rast("interpolate", rast, attr.device)
    return _Interpolate.apply(attr, rast, tri), None


def antialias(color, rast, pos, tri, topology_hash=None, pos_gradient_boost=1.0):
    """nvdiffrast.torch.antialias for batch size 1: color (1, H, W, C) -> out (1, H, W, C) (module docstring for the rule).
    `topology_hash` is not supported (the topology is rebuilt every call); `pos_gradient_boost` must be 1."""
    if topology_hash is not None or pos_gradient_boost != 1.0:
        raise RuntimeError("antialias: topology_hash and pos_gradient_boost are not supported")
    _check_pos_tri("antialias", pos, tri)
    _need("antialias", color, "color", torch.float32)
    _check_rast("antialias", rast, pos.device)
    if color.dim() != 4 or tuple(color.shape[:3]) != tuple(rast.shape[:3]) or color.shape[3] < 1:
        raise RuntimeError(f"antialias: color must be (1, H, W, C) matching rast {tuple(rast.shape)}, got {tuple(color.shape)}")
    return _Antialias.apply(color, rast, pos, tri)


def texture(tex, uv, uv_da=None, mip_level_bias=None, mip=None, filter_mode="auto", boundary_mode="wrap", max_mip_level=None):
    """nvdiffrast.torch.texture for batch size 1 without mip-maps: tex (1, Ht, Wt, C), uv (1, H, W, 2) (or any (1, ..., 2)) ->
    out (1, H, W, C) (module docstring for the conventions).  filter_mode: "auto" (= "linear"), "linear" or "nearest";
    boundary_mode: "wrap", "clamp" or "zero".  Mip-maps (`uv_da`, `mip_level_bias`, `mip`, `max_mip_level`, the "linear-mipmap-*"
    filters) and cube maps are not supported."""
    if uv_da is not None or mip_level_bias is not None or mip is not None or max_mip_level is not None:
        raise RuntimeError("texture: mip-maps (uv_da, mip_level_bias, mip, max_mip_level) are not supported")
    if isinstance(filter_mode, str) and filter_mode.startswith("linear-mipmap"):
        raise RuntimeError(f"texture: mip-maps (filter_mode {filter_mode!r}) are not supported")
    if boundary_mode == "cube":
        raise RuntimeError("texture: cube maps (boundary_mode 'cube') are not supported")
    filter_mode = "linear" if filter_mode == "auto" else filter_mode
    if filter_mode not in FILTER_MODES:
        raise RuntimeError(f"texture: filter_mode must be one of auto, {', '.join(FILTER_MODES)}, got {filter_mode!r}")
    if boundary_mode not in BOUNDARY_MODES:
        raise RuntimeError(f"texture: boundary_mode must be one of {', '.join(BOUNDARY_MODES)}, got {boundary_mode!r}")
    _need("texture", tex, "tex", torch.float32)
    _need("texture", uv, "uv", torch.float32)
    if tex.dim() != 4 or tex.shape[3] < 1:
        raise RuntimeError(f"texture: tex must be (1, Ht, Wt, C) with C >= 1, got {tuple(tex.shape)}")
    if uv.dim() < 2 or uv.shape[-1] != 2:
        raise RuntimeError(f"texture: uv must be (1, ..., 2), got {tuple(uv.shape)}")
    if tex.shape[0] != 1 or uv.shape[0] != 1:
        raise RuntimeError(f"texture: only batch size 1 is supported, got tex {tuple(tex.shape)} and uv {tuple(uv.shape)}")
    if not (0 < tex.shape[1] <= 16384 and 0 < tex.shape[2] <= 16384):
        raise RuntimeError(f"texture: the texture's sides must be within [1, 16384], got {tuple(tex.shape)}")
    if uv.device != tex.device:
        raise RuntimeError("texture: tex and uv must be on one device")
    return _Texture.apply(tex, uv, FILTER_MODES.index(filter_mode), BOUNDARY_MODES.index(boundary_mode))


def clip_positions(cam, verts):
    """[verts, 1] @ cam.full_proj_transform as (1, V, 4) clip-space positions (differentiable w.r.t. verts)."""
    hom = torch.cat([verts, torch.ones_like(verts[:, :1])], dim=1)
    return (hom @ cam.full_proj_transform).unsqueeze(0).contiguous()


def _resolution(cam, resolution):
    return (int(cam.image_height), int(cam.image_width)) if resolution is None else tuple(int(r) for r in resolution)


def render_mask_and_mesh(glctx, verts, faces, vtx_color, cam, resolution=None, whitebackground=False, rast=None):
    """render_mask and render_mesh of R/utils/renderer.py:33-121 from one rasterize and one 4-channel interpolate / antialias
    (colour + ones; antialias is linear per channel, so this equals the reference's separate calls): (mask (H, W, 1), image
    (3, H, W)).  verts (V, 3) world space, faces (F, 3) int32, vtx_color (V, 3), cam: a TorchCamera.  rast: the (1, H, W, 4) result
    of rasterize(clip_positions(cam, verts), faces, (H, W)) when the caller already has it (visualize.py shades the same buffer)."""
    H, W = _resolution(cam, resolution)
    pos = clip_positions(cam, verts)
    faces = faces.contiguous()
    if rast is None:
        rast, _ = rasterize(glctx, pos, faces, (H, W))
    else:
        _check_rast("render_mesh", rast, pos.device)
        if tuple(rast.shape[1:3]) != (H, W):
            raise RuntimeError(f"render_mesh: rast {tuple(rast.shape)} does not match the resolution {(H, W)}")
    attr = torch.cat([vtx_color, torch.ones_like(vtx_color[:, :1])], dim=1).contiguous()
    col, _ = interpolate(attr, rast, faces)
    col = antialias(col, rast, pos, faces)[0]
    mask = col[..., 3:4]
    bg = 1.0 if whitebackground else 0.0
    image = torch.where(mask != 0, col[..., :3], torch.full_like(col[..., :3], bg)).clamp(0.0, 1.0)
    return mask, image.permute(2, 0, 1)


def render_mesh_textured(glctx, verts, faces, uv, tex, cam, resolution=None, whitebackground=False, rast=None):
    """render_mesh with the colour looked up in a texture instead of interpolated from the vertices: rasterize, interpolate of the
    per-corner uv (F, 3, 2) (its own index array arange(3F): every face has its own three uv rows, as mesh_texture's atlas gives
    them), texture(..., boundary_mode="clamp"), antialias, then render_mesh's background rule; (3, H, W).  tex (Ht, Wt, 3) or
    (1, Ht, Wt, 3).  Background pixels carry colour 0 and coverage 0 into antialias, as in render_mesh."""
    H, W = _resolution(cam, resolution)
    pos = clip_positions(cam, verts)
    faces = faces.contiguous()
    F = int(faces.shape[0])
    if tuple(uv.shape) != (F, 3, 2):
        raise RuntimeError(f"render_mesh_textured: uv must be ({F}, 3, 2), one row per face corner, got {tuple(uv.shape)}")
    if tex.dim() == 3:
        tex = tex.unsqueeze(0)
    if rast is None:
        rast, _ = rasterize(glctx, pos, faces, (H, W))
    else:
        _check_rast("render_mesh_textured", rast, pos.device)
        if tuple(rast.shape[1:3]) != (H, W):
            raise RuntimeError(f"render_mesh_textured: rast {tuple(rast.shape)} does not match the resolution {(H, W)}")
    corner = torch.arange(3 * F, dtype=torch.int32, device=faces.device).reshape(F, 3)
    uv_px, _ = interpolate(uv.reshape(3 * F, 2).contiguous(), rast, corner)
    rgb = texture(tex.contiguous(), uv_px, filter_mode="linear", boundary_mode="clamp")
    covered = (rast[..., 3:4] > 0).to(rgb.dtype)
    col = (torch.cat([rgb, torch.ones_like(rgb[..., :1])], dim=3) * covered).contiguous()
    col = antialias(col, rast, pos, faces)[0]
    mask = col[..., 3:4]
    bg = 1.0 if whitebackground else 0.0
    image = torch.where(mask != 0, col[..., :3], torch.full_like(col[..., :3], bg)).clamp(0.0, 1.0)
    return image.permute(2, 0, 1)


def render_mask(glctx, verts, faces, cam, resolution=None):
    """R/utils/renderer.py:33-66: the antialiased interpolation of ones, (H, W, 1)."""
    H, W = _resolution(cam, resolution)
    pos = clip_positions(cam, verts)
    faces = faces.contiguous()
    rast, _ = rasterize(glctx, pos, faces, (H, W))
    ones = torch.ones((verts.shape[0], 1), dtype=torch.float32, device=verts.device)
    m, _ = interpolate(ones, rast, faces)
    return antialias(m, rast, pos, faces)[0]


def render_mesh(glctx, verts, faces, vtx_color, cam, resolution=None, whitebackground=False, rast=None):
    """R/utils/renderer.py:69-121: the antialiased vertex colour, background where the mask is 0, clamped to [0, 1], (3, H, W)."""
    return render_mask_and_mesh(glctx, verts, faces, vtx_color, cam, resolution, whitebackground, rast)[1]
