"""End-to-end GPU tests of the texture bake (dg-mesh_amd/mesh_texture.py) and the textured render (mesh_raster.render_mesh_textured).

An affine colour c = A x + b is baked into the atlas of a mesh; because the atlas holds the unclamped affine interpolation, the textured
render must reproduce render_mesh of the vertex colours on every pixel -- at cell 4 too, the smallest cell, where a chart is one texel
step wide.  Tolerance: 8 x the largest |ref32 - ref64| of the numpy restatement of interpolate-uv-then-sample (tests/_texture_ref.py)
on the device's own rast buffer and baked texture, the rule of tests/test_mesh_inside.py; nothing comes from the images compared.
The colour stays within [0.1, 0.9] on the mesh and within [0, 1] one edge length beyond it (the extrapolated texels of a chart), so
bake's clamp to [0, 1] touches nothing.  Meshes: icosphere(2), and _surface_ref.mc_sphere(1e-3) -- the tiny faces and slivers of a
marching-cubes surface -- moved to the origin and scaled to unit radius so that it fills the 96 x 96 view of the synthetic camera."""
import functools
import os

import numpy as np
import pytest
import torch

import _edges_ref as E
import _surface_ref as S
import _texture_ref as R
from conftest import pkg
from test_visualize import _record_psr, scene  # noqa: F401  (the tiny mesh-phase scene of the visualize tests, as a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_FACTOR = 8.0
SIDE = 96
A = np.array([[0.2, 0.0, 0.1], [0.0, 0.22, -0.1], [-0.15, 0.1, 0.18]], np.float32)  # rows of length <= 0.27: 0.5 +- 0.27 on the unit sphere
B = np.float32(0.5)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == "icosphere":
        verts, faces = E.icosphere(2)
    else:
        verts, faces = S.mc_sphere(1e-3)
        centre = (verts.max(0) + verts.min(0)) / 2
        verts = ((verts - centre) / np.abs(verts - centre).max()).astype(np.float32)
    for a in (verts, faces):
        a.setflags(write=False)
    return verts, faces


def color_fn(points):
    """points @ A + B, written out elementwise: the same bits for a point whatever batch it comes in."""
    a = dev(A)
    return ((points[:, 0:1] * a[0] + points[:, 1:2] * a[1]) + points[:, 2:3] * a[2]) + float(B)


def camera():
    syn, SC = pkg("synthetic"), pkg("scene")
    return SC.TorchCamera(syn.make_camera(SIDE, SIDE), DEV)


@pytest.mark.parametrize("cell", [4, 8])
@pytest.mark.parametrize("name", ["icosphere", "mc_sphere"])
def test_textured_render_equals_vertex_colour_render(name, cell):
    MT, MR = pkg("mesh_texture"), pkg("mesh_raster")
    verts, faces = mesh(name)
    edge = np.linalg.norm(verts[faces] - verts[np.roll(faces, 1, 1)], axis=-1).max()
    reach = (np.abs(verts).max() + edge) * np.linalg.norm(A, axis=0).max()
    assert 0.1 <= B - np.abs(verts @ A).max() and B + np.abs(verts @ A).max() <= 0.9 and reach <= 0.5  # the docstring's condition on the colour
    v, f = dev(verts), dev(faces)
    calls = []
    tex, uv, atlas = MT.bake(v, f, lambda p: (calls.append(int(p.shape[0])), color_fn(p))[1], cell=cell, chunk=1000)
    F = len(faces)
    assert atlas == MT.build_atlas(F, cell=cell) and tex.shape == (atlas.size, atlas.size, 3) and uv.shape == (F, 3, 2)
    pos, face_id = MT.atlas_interpolate(atlas, v, f)
    owned = face_id >= 0
    assert sum(calls) == int(owned.sum()) and max(calls) <= 1000 and len(calls) == -(-int(owned.sum()) // 1000)  # owned texels only, in chunks
    assert not bool(tex[~owned].any()) and 0.0 < float(tex[owned].min()) and float(tex[owned].max()) < 1.0
    assert bool((tex[owned] == color_fn(pos[owned])).all())
    cam = camera()
    rast, _ = MR.rasterize(None, MR.clip_positions(cam, v), f, (SIDE, SIDE))
    vtx_color = color_fn(v)
    want = MR.render_mesh(None, v, f, vtx_color, cam, rast=rast)
    got = MR.render_mesh_textured(None, v, f, uv, tex, cam, rast=rast)
    assert got.shape == want.shape == (3, SIDE, SIDE)
    # the tolerance: the restatement of interpolate-uv-then-sample on the device's rast and texture, fp32 in the device's order against fp64
    rast_h, tex_h, uv_h = rast[0].cpu().numpy(), tex.cpu().numpy(), uv.cpu().numpy()
    uv64, covered = R.interp_uv(rast_h, uv_h, np.float64)
    uv32, _ = R.interp_uv(rast_h, uv_h, np.float32)
    ref64 = R.sample(tex_h, uv64, "linear", "clamp", np.float64)[covered]
    ref32 = R.sample(tex_h, uv32, "linear", "clamp", np.float32)[covered]
    ref_err = float(np.abs(ref32.astype(np.float64) - ref64).max())
    tol = TOL_FACTOR * ref_err
    corner = torch.arange(3 * F, dtype=torch.int32, device=DEV).reshape(F, 3)
    uv_px, _ = MR.interpolate(uv.reshape(3 * F, 2).contiguous(), rast, corner)
    sampled = MR.texture(tex[None], uv_px, boundary_mode="clamp")[0].reshape(-1, 3).cpu().numpy()[covered]
    err_sample = float(np.abs(sampled.astype(np.float64) - ref64).max())
    err_image = float((got - want).abs().max())
    exact = (verts.astype(np.float64) @ A.astype(np.float64) + float(B))
    print(f"{name} F {F} cell {cell} size {atlas.size}: covered pixels {int(covered.sum())}; numpy fp32 statement {ref_err:.3e}, factor "
          f"{TOL_FACTOR:g}, tolerance {tol:.3e}; device sample against ref64 {err_sample:.3e}; textured image against render_mesh "
          f"{err_image:.3e}; vertex colours in [{exact.min():.3f}, {exact.max():.3f}]")
    assert covered.sum() > 1500
    assert err_sample <= tol, f"sample: {err_sample:.3e} > {tol:.3e}"
    assert err_image <= tol, f"image: {err_image:.3e} > {tol:.3e}"
    white = MR.render_mesh_textured(None, v, f, uv, tex, cam, whitebackground=True)  # (rasterizes by itself)
    assert float((white - MR.render_mesh(None, v, f, vtx_color, cam, whitebackground=True)).abs().max()) <= tol
    assert float(white[:, 0, 0].min()) == 1.0 and float(got[:, 0, 0].max()) == 0.0


def test_bake_vertex_colors_gradients_and_errors():
    """bake_vertex_colors is atlas_interpolate of the colours; render_mesh_textured passes gradients to the texture and the vertices."""
    MT, MR = pkg("mesh_texture"), pkg("mesh_raster")
    verts, faces = mesh("icosphere")
    v, f = dev(verts), dev(faces)
    colours = color_fn(v)
    tex, uv, atlas = MT.bake_vertex_colors(v, f, colours, size=128)
    assert atlas == MT.build_atlas(len(faces), size=128) and bool((tex == MT.atlas_interpolate(atlas, colours, f)[0]).all())
    baked = MT.bake(v, f, color_fn, size=128)
    assert float((baked[0] - tex).abs().max()) < 1e-6 and bool((baked[1] == uv).all())
    cam = camera()
    tex_g, v_g = tex.clone().requires_grad_(True), v.clone().requires_grad_(True)
    image = MR.render_mesh_textured(None, v_g, f, uv, tex_g, cam)
    image.square().sum().backward()
    assert bool(torch.isfinite(tex_g.grad).all()) and float(tex_g.grad.abs().max()) > 0 and tex_g.grad.shape == tex.shape
    assert bool(torch.isfinite(v_g.grad).all()) and float(v_g.grad.abs().max()) > 0
    # no pixel reads an unowned texel with a weight beyond the rounding of its barycentrics (1e-7 of a texel)
    assert float(tex_g.grad[MT.atlas_interpolate(atlas, v, f)[1] < 0].abs().max()) <= 1e-5 * float(tex_g.grad.abs().max())
    with pytest.raises(ValueError, match="simplify="):
        MT.bake(v, f, color_fn, size=40)
    with pytest.raises(ValueError, match=r"must return \(n, 3\)"):
        MT.bake(v, f, lambda p: p[:, :2], cell=4)
    with pytest.raises(RuntimeError, match=r"uv must be \(320, 3, 2\)"):
        MR.render_mesh_textured(None, v, f, uv[:5], tex, cam)


def test_export_dynamic_mesh_with_texture(scene, tmp_path):  # noqa: F811
    """texture= adds dynamic_mesh_textured/frame_{i}.obj|.glb, baked from the network after simplify; the PLY files are byte-identical
    to a run without it (on the same DPSR fields: its splat sums with float atomics, so the second run replays the first one's)."""
    V, O, G, PLY, MS = pkg("visualize"), pkg("obj_io"), pkg("glb_io"), pkg("ply_io"), pkg("mesh_simplify")
    args = (scene["g"], scene["deform"], scene["deform_back"], scene["mesh"])
    m = scene["mesh"]
    fields, orig = _record_psr(m)
    try:
        plain = V.export_dynamic_mesh(*args, str(tmp_path / "plain"), frames=2, simplify=MS.SimplifySpec(grid=12))
        replay = iter(list(fields))
        m.psr = lambda *a, **k: next(replay)
        obj = V.export_dynamic_mesh(*args, str(tmp_path / "obj"), frames=2, simplify=MS.SimplifySpec(grid=12), texture={"cell": 6})
        replay = iter(list(fields[:2]))
        glb = V.export_dynamic_mesh(*args, str(tmp_path / "glb"), frames=2, simplify=MS.SimplifySpec(grid=12),
                                    texture=pkg("mesh_texture").TextureSpec(size=512, format="glb"))
    finally:
        m.psr = orig
    assert not os.path.exists(tmp_path / "plain" / "dynamic_mesh_textured")
    for i in range(2):
        ply = open(plain[i], "rb").read()
        assert open(obj[i], "rb").read() == ply and open(glb[i], "rb").read() == ply
        verts, faces, colours = PLY.read_mesh_ply(plain[i], return_colors=True)
        stem = tmp_path / "obj" / "dynamic_mesh_textured" / f"frame_{i}"
        assert all(os.path.exists(f"{stem}.{ext}") for ext in ("obj", "mtl", "png"))
        v2, f2, uv, tex = O.read_mesh_obj(f"{stem}.obj")
        size = 6 * R.per_row(len(faces))
        assert np.array_equal(v2, verts) and np.array_equal(f2, faces) and uv.shape == (len(faces), 3, 2) and tex.shape == (size, size, 3)
        assert np.abs(uv - R.atlas_uv(len(faces), size, 6)).max() <= 1e-7
        # the texture is the network's colour at the written mesh (not the decimated vertex colours of the PLY, which are those of the
        # clusters' representatives): the texel under a face's corner holds the network at that vertex, up to one step of the bytes
        fid = torch.tensor([i / 2], dtype=torch.float32, device=DEV)
        net = pkg("mesh_texture").appearance_color_fn(m, scene["deform_back"], fid)(dev(verts)).detach().clamp(0, 1).cpu().numpy()
        corner = R.sample(tex.astype(np.float64), uv.reshape(-1, 2), "nearest", "clamp").reshape(-1, 3, 3)
        step = np.abs(corner - np.floor(net.astype(np.float64) * 255)[faces]).max()
        print(f"frame {i}: V {len(verts)} F {len(faces)} atlas {size}; texture against the network at the corners: {step:.0f} of 255; "
              f"PLY colours against the network {np.abs(colours[:, :3] - np.floor(net.astype(np.float64) * 255)).max():.0f} of 255")
        assert step <= 1.0 and tex.max() > 1
        back = G.read_mesh_glb(str(tmp_path / "glb" / "dynamic_mesh_textured" / f"frame_{i}.glb"))
        assert np.array_equal(back["verts"], verts[faces.reshape(-1)]) and back["tex"].shape == (512, 512, 3) and back["colors"] is None
        assert np.abs(back["uv"] - R.atlas_uv(len(faces), 512, 512 // R.per_row(len(faces)))).max() == 0


def test_testing_saves_the_reference_glb_files(scene, tmp_path):  # noqa: F811
    """save_glb writes test_results/dynamic_glb/frame_{idx}.glb: the mesh and the colour bytes of the PLY that save_meshes writes."""
    E, G, PLY, SC = pkg("evaluate"), pkg("glb_io"), pkg("ply_io"), pkg("scene")
    cams = scene["cameras"][:2]
    kw = dict(pipe=SC.PipelineParams(), background=torch.ones(3, device=DEV), mesh=scene["mesh"])
    res = E.testing(scene["g"], scene["deform"], scene["deform_back"], cams, out_dir=str(tmp_path), save_meshes=True, save_glb=True, **kw)
    assert res["views"].shape == (2, 2, 4) and np.isfinite(res["views"][..., :3]).all()
    for idx in range(2):
        verts, faces, colours = PLY.read_mesh_ply(str(tmp_path / "test_results" / "dynamic_mesh" / f"frame_{idx}.ply"), return_colors=True)
        back = G.read_mesh_glb(str(tmp_path / "test_results" / "dynamic_glb" / f"frame_{idx}.glb"))
        assert np.array_equal(back["verts"], verts) and np.array_equal(back["faces"], faces) and np.array_equal(back["colors"], colours)
        assert back["uv"] is None and back["tex"] is None and len(faces) > 0
    plain = tmp_path / "plain"
    E.testing(scene["g"], scene["deform"], scene["deform_back"], cams, out_dir=str(plain), save_meshes=True, **kw)
    assert not os.path.exists(plain / "test_results" / "dynamic_glb") and os.path.exists(plain / "test_results" / "dynamic_mesh" / "frame_1.ply")
    with pytest.raises(ValueError, match="save_glb needs mesh and out_dir"):
        E.testing(scene["g"], scene["deform"], scene["deform_back"], cams, save_glb=True, **kw)


@pytest.mark.parametrize("ext", ["obj", "glb"])
def test_command_line_bakes_a_ply(ext, tmp_path, capsys):
    MT, O, G, PLY = pkg("mesh_texture"), pkg("obj_io"), pkg("glb_io"), pkg("ply_io")
    verts, faces = mesh("icosphere")
    colours = color_fn(dev(verts)).cpu().numpy()
    src, out = str(tmp_path / "in.ply"), str(tmp_path / "baked" / f"ball.{ext}")
    PLY.write_mesh_ply(src, verts, faces, vertex_colors=colours)
    assert MT.main([src, out, "--cell", "6"]) == 0
    assert "F 320  size 78 cell 6" in capsys.readouterr().out
    if ext == "obj":
        v2, f2, uv, tex = O.read_mesh_obj(out)
    else:
        back = G.read_mesh_glb(out)
        v2, f2, uv, tex = verts, faces, back["uv"], back["tex"]
        assert np.array_equal(back["verts"], verts[faces.reshape(-1)])
    assert np.array_equal(v2, verts) and np.array_equal(f2, faces) and tex.shape == (78, 78, 3)
    assert np.abs(uv - R.atlas_uv(320, 78, 6)).max() <= 1e-7
    # the texel under every corner holds the PLY's colour byte of that vertex
    corner = R.sample(tex.astype(np.float64), uv.reshape(-1, 2), "nearest", "clamp").reshape(-1, 3, 3)
    assert np.array_equal(corner, np.clip(colours * 255, 0, 255).astype(np.uint8)[faces].astype(np.float64))
    with pytest.raises(SystemExit):
        MT.main([src, str(tmp_path / "x.stl"), "--cell", "6"])
    with pytest.raises(SystemExit):
        MT.main([src, out])  # neither --size nor --cell
