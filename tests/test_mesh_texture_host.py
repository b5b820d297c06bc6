"""Host-side tests of the texture feature: the numpy restatement (tests/_texture_ref.py) against torch's grid_sample, the atlas layout's
no-bleed property, build_atlas, and the OBJ / GLB writers.  No GPU."""
import json
import struct

import numpy as np
import pytest
import torch

import _edges_ref as E
import _texture_ref as R
from conftest import pkg


def random_case(Ht, Wt, C, n, seed, lo=-1.5, hi=2.5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((Ht, Wt, C)), rng.uniform(lo, hi, (n, 2))


def grid_sample(tex, uv, padding):
    t = torch.from_numpy(tex).permute(2, 0, 1)[None]
    grid = torch.from_numpy(2 * uv - 1).reshape(1, 1, -1, 2)
    out = torch.nn.functional.grid_sample(t, grid, mode="bilinear", padding_mode=padding, align_corners=False)
    return out[0, :, 0].T.numpy()


@pytest.mark.parametrize("Ht,Wt,C", [(1, 1, 1), (2, 3, 1), (5, 7, 3), (33, 130, 3)])
@pytest.mark.parametrize("boundary,padding", [("clamp", "border"), ("zero", "zeros")])
def test_reference_equals_grid_sample(Ht, Wt, C, boundary, padding):
    tex, uv = random_case(Ht, Wt, C, 4000, Ht * 131 + Wt)
    ref = R.sample(tex, uv, "linear", boundary, np.float64)
    err = np.abs(ref - grid_sample(tex, uv, padding)).max()
    print(f"{(Ht, Wt, C)} {boundary}: max |ref64 - grid_sample| {err:.3e}")
    assert err <= 1e-13  # (fp64 on values of order 1: a few 1e-16 measured)


@pytest.mark.parametrize("Ht,Wt,C", [(1, 1, 1), (2, 3, 1), (5, 7, 3), (33, 130, 3)])
@pytest.mark.parametrize("filter_mode", R.FILTERS)
def test_wrap_is_periodic(Ht, Wt, C, filter_mode):
    """wrap at uv equals clamp on the 3 x 3 tiling of the texture at the shifted (uv + 1) / 3, for uv in (-1, 2) less the outermost
    half texel (where clamp on the tiling meets its own border)."""
    tex, uv = random_case(Ht, Wt, C, 4000, Ht * 17 + Wt, lo=-0.9, hi=1.9)
    uv = uv[((uv > -1 + 0.6 / np.array([Wt, Ht])) & (uv < 2 - 0.6 / np.array([Wt, Ht]))).all(1)]
    tiled = np.tile(tex, (3, 3, 1))
    a = R.sample(tex, uv, filter_mode, "wrap", np.float64)
    b = R.sample(tiled, (uv + 1) / 3, filter_mode, "clamp", np.float64)
    if filter_mode == "nearest":  # (an index, not a blend: leave out the samples within rounding of a texel boundary)
        x = uv * np.array([Wt, Ht])
        keep = (np.abs(x - np.round(x)) > 1e-9).all(1)
        a, b = a[keep], b[keep]
    err = np.abs(a - b).max()
    print(f"{(Ht, Wt, C)} {filter_mode}: max |wrap - tiled clamp| {err:.3e} over {len(a)} samples")
    assert len(a) > 1000 and err <= 1e-12  # (the 1 x 1 texture's margin is 0.6 of the texture on every side)


def test_reference_bad_inputs_and_nearest():
    tex = np.arange(12, dtype=np.float64).reshape(3, 4, 1)
    uv = np.array([[np.nan, 0.5], [0.5, np.inf], [-np.inf, 0.1], [1e30, -1e30], [0.0, 0.0], [1.0, 1.0], [0.125, 0.5]])
    for boundary in R.BOUNDARIES:
        for filter_mode in R.FILTERS:
            for dt in (np.float32, np.float64):
                out = R.sample(tex, uv, filter_mode, boundary, dt)
                assert out.dtype == dt and np.isfinite(out).all() and (out[:3] == 0).all()
    assert R.sample(tex, uv, "nearest", "clamp")[3:, 0].tolist() == [3.0, 0.0, 11.0, 4.0]   # (3, 0), (0, 0), (3, 2), (0, 1)
    assert R.sample(tex, uv, "nearest", "wrap")[3:, 0].tolist() == [0.0, 0.0, 0.0, 4.0]     # 1e30 and 1 reduce to 0
    assert R.sample(tex, uv, "nearest", "zero")[3:, 0].tolist() == [0.0, 0.0, 0.0, 4.0]     # u = 1 is outside
    assert R.sample(tex, uv, "linear", "clamp")[6, 0] == 4.0                                   # the centre of texel (0, 1)
    # the analytic gradients against a central difference of the fp64 statement
    rng = np.random.default_rng(5)
    tex, uv = rng.standard_normal((5, 7, 3)), rng.uniform(-0.4, 1.4, (200, 2))
    uv = uv[(R.lattice_distance(uv, 5, 7) > 1e-3).all(1)]
    dout = rng.standard_normal((len(uv), 3))
    for boundary in R.BOUNDARIES:
        dtex, duv = R.sample_grads(tex, uv, dout, "linear", boundary)
        h = 1e-7
        for k in range(2):
            e = np.zeros(2)
            e[k] = h
            num = ((R.sample(tex, uv + e, "linear", boundary) - R.sample(tex, uv - e, "linear", boundary)) * dout).sum(1) / (2 * h)
            assert np.abs(num - duv[:, k]).max() < 1e-5
        probe = rng.standard_normal(tex.shape)
        lin = ((R.sample(tex + probe, uv, "linear", boundary) - R.sample(tex, uv, "linear", boundary)) * dout).sum()
        assert abs(lin - (dtex * probe).sum()) < 1e-9


@pytest.mark.parametrize("s", [4, 5, 8, 13])
def test_chart_footprints_are_owned_and_disjoint(s):
    """Every point of a chart, corners and edges included, has its whole bilinear footprint (the texels with a non-zero weight) inside
    the cell and owned by its own face; so the two footprints of a cell are disjoint and no chart bleeds into another."""
    face, i, j = R.owner(s, s, 2)  # one cell
    owned = [{(int(a), int(b)) for a, b in zip(i[face == k], j[face == k])} for k in (0, 1)]
    assert owned[0] == {(a, b) for a in range(s) for b in range(s) if a + b <= s - 2}
    assert owned[1] == {(a, b) for a in range(s) for b in range(s) if a + b >= s}
    prints = [R.footprint(R.chart_points(s, odd)) for odd in (0, 1)]
    for k in (0, 1):
        assert prints[k] <= owned[k], sorted(prints[k] - owned[k])
        assert all(0 <= a < s and 0 <= b < s for a, b in prints[k])
        assert {tuple(c) for c in R.corner_local(s)[k]} <= prints[k]
    assert not prints[0] & prints[1]
    # the unclamped barycentrics make bilinear sampling exact for an affine attribute, at every point of both charts
    attr = np.array([[0.3, -1.0], [2.0, 0.5], [-0.7, 4.0], [1.1, 1.3]])
    faces = np.array([[0, 1, 2], [3, 2, 1]])
    tex, fid = R.atlas_interpolate(attr, faces, s, s, np.float64)
    assert (fid[::-1].diagonal() == -1).all() and set(np.unique(fid)) == {-1, 0, 1}
    for k in (0, 1):
        pts = R.chart_points(s, k)
        c = R.corner_local(s)[k].astype(np.float64)
        T = np.linalg.solve(np.c_[c, np.ones(3)], attr[faces[k]])  # the affine map (i, j, 1) -> attr
        want = np.c_[pts, np.ones(len(pts))] @ T
        got = R.sample(tex, (pts + 0.5) / s, "linear", "clamp", np.float64)
        assert np.abs(got - want).max() < 1e-12


def test_build_atlas():
    MT = pkg("mesh_texture")
    assert [R.per_row(F) for F in (0, 1, 2, 3, 8, 9, 18, 19, 320)] == [1, 1, 1, 2, 2, 3, 3, 4, 13]
    assert MT.build_atlas(320, size=2048) == MT.Atlas(2048, 157, 13, 320)
    assert MT.build_atlas(320, cell=4) == MT.Atlas(52, 4, 13, 320)
    assert MT.build_atlas(1, cell=16) == MT.Atlas(16, 16, 1, 1) and MT.build_atlas(2, size=21) == MT.Atlas(21, 21, 1, 2)
    assert MT.build_atlas(7, size=21) == MT.Atlas(21, 10, 2, 7)  # a size that is no multiple of the cell: a one-texel margin
    for F in (1, 2, 3, 7, 50, 321, 12345):
        a = MT.build_atlas(F, cell=5)
        assert a.cells_per_row == R.per_row(F) and a.cells_per_row ** 2 >= (F + 1) // 2 and a.size == 5 * a.cells_per_row
        b = MT.build_atlas(F, size=1000)
        assert b.cell == 1000 // R.per_row(F) and b.cells_per_row ** 2 >= (F + 1) // 2 and b.cells_per_row * b.cell <= 1000
    with pytest.raises(ValueError, match="exactly one"):
        MT.build_atlas(10)
    with pytest.raises(ValueError, match="exactly one"):
        MT.build_atlas(10, size=64, cell=4)
    with pytest.raises(ValueError, match=r"1000000 faces.*simplify=.*larger size"):
        MT.build_atlas(1000000, size=2048)
    with pytest.raises(ValueError, match="smallest cell 4"):
        MT.build_atlas(10, cell=3)
    with pytest.raises(ValueError, match="16384"):
        MT.build_atlas(10 ** 8, cell=4)
    assert MT.as_spec(None) is None and MT.as_spec({"cell": 6, "format": "glb"}) == MT.TextureSpec(size=2048, cell=6, format="glb")
    assert MT.TextureSpec().atlas_args() == {"size": 2048} and MT.TextureSpec(cell=6).atlas_args() == {"cell": 6}
    with pytest.raises(ValueError, match="format"):
        MT.as_spec({"format": "fbx"})
    with pytest.raises(TypeError):
        MT.as_spec(3)


def baked_icosphere(cell):
    """icosphere(2) with an affine colour baked by the numpy restatement: (verts, faces, colours, uv, tex float32, size)."""
    verts, faces = E.icosphere(2)
    colours = (0.5 + verts.astype(np.float64) @ np.array([[0.2, 0.0, 0.1], [0.0, 0.25, -0.1], [-0.15, 0.1, 0.2]])).astype(np.float32)
    size = cell * R.per_row(len(faces))
    tex, _ = R.atlas_interpolate(colours, faces, size, cell, np.float32)
    return verts, faces, colours, R.atlas_uv(len(faces), size, cell), tex, size


def centroid_colours(tex_u8, uv):
    """The colour the files give at every face's centroid: the uint8 texture sampled at the mean of the face's three uv rows."""
    return R.sample(tex_u8.astype(np.float64) / 255, uv.astype(np.float64).mean(1), "linear", "clamp", np.float64)


def test_obj_round_trip_and_v_flip(tmp_path):
    O, PNG = pkg("obj_io"), pkg("png_io")
    from PIL import Image
    verts, faces, colours, uv, tex, size = baked_icosphere(8)
    paths = O.write_mesh_obj(str(tmp_path / "out" / "ball.obj"), verts, faces, uv, tex)
    assert [p.rsplit(".", 1)[1] for p in paths] == ["obj", "mtl", "png"] and "map_Kd ball.png" in open(paths[1]).read()
    text = open(paths[0]).read().splitlines()
    assert sum(ln.startswith("v ") for ln in text) == len(verts) and sum(ln.startswith("vt ") for ln in text) == 3 * len(faces)
    assert text[2 + len(verts)] == f"vt {uv[0, 0, 0]:.9g} {1.0 - np.float64(uv[0, 0, 1]):.9g}"  # the file holds (u, 1 - v)
    assert text[-1] == f"f {faces[-1, 0] + 1}/{3 * len(faces) - 2} {faces[-1, 1] + 1}/{3 * len(faces) - 1} {faces[-1, 2] + 1}/{3 * len(faces)}"
    v2, f2, uv2, tex2 = O.read_mesh_obj(paths[0])
    assert np.array_equal(v2, verts) and np.array_equal(f2, faces) and np.abs(uv2 - uv).max() <= 1e-7
    want = np.clip(tex * 255, 0, 255).astype(np.uint8)
    assert tex2.dtype == np.uint8 and np.array_equal(tex2, want)
    assert np.array_equal(np.asarray(Image.open(paths[2]).convert("RGB")), want) and np.array_equal(PNG.read_png_host(paths[2]), want)
    # what a viewer does with OBJ's bottom-left origin: image row = (1 - vt_v) * H from the top.  Sampling the PIL image there gives the
    # baked colour at every centroid (the quantisation to bytes is the only difference: half a step plus the blend of four texels)
    vt = np.array([[float(x) for x in ln.split()[1:]] for ln in text if ln.startswith("vt ")]).reshape(-1, 3, 2)
    viewer_uv = np.stack([vt[..., 0], 1.0 - vt[..., 1]], -1)
    got = centroid_colours(np.asarray(Image.open(paths[2]).convert("RGB")), viewer_uv)
    baked = colours.astype(np.float64)[faces].mean(1)
    print(f"obj: max |colour through the files - baked| at the centroids {np.abs(got - baked).max():.3e}")
    assert np.abs(got - baked).max() <= 1.01 / 255
    flipped = centroid_colours(np.asarray(Image.open(paths[2]).convert("RGB")), vt)  # without the flip the colours are another face's
    assert np.abs(flipped - baked).max() > 0.05


def parse_glb(path):
    data = open(path, "rb").read()
    magic, version, total = struct.unpack_from("<III", data, 0)
    assert (magic, version, total) == (0x46546C67, 2, len(data)) and len(data) % 4 == 0
    n_json, kind = struct.unpack_from("<II", data, 12)
    assert kind == 0x4E4F534A and n_json % 4 == 0
    doc = json.loads(data[20:20 + n_json])
    n_bin, kind = struct.unpack_from("<II", data, 20 + n_json)
    assert kind == 0x004E4942 and n_bin % 4 == 0 and 28 + n_json + n_bin == len(data)
    blob = data[28 + n_json:]
    assert doc["asset"]["version"] == "2.0" and doc["buffers"] == [{"byteLength": n_bin}] and len(doc["meshes"]) == 1
    assert len(doc["meshes"][0]["primitives"]) == 1
    for bv in doc["bufferViews"]:
        assert bv["buffer"] == 0 and bv["byteOffset"] % 4 == 0 and bv["byteOffset"] + bv["byteLength"] <= n_bin
    return doc, blob


def accessor(doc, blob, index, dtype, width):
    acc = doc["accessors"][index]
    bv = doc["bufferViews"][acc["bufferView"]]
    assert bv["byteLength"] == acc["count"] * width * np.dtype(dtype).itemsize
    return np.frombuffer(blob, dtype, acc["count"] * width, bv["byteOffset"]).reshape(acc["count"], width), acc


def test_glb_round_trips(tmp_path):
    G = pkg("glb_io")
    import io

    from PIL import Image
    verts, faces, colours, uv, tex, size = baked_icosphere(5)
    V, F = len(verts), len(faces)
    # vertex colours: the reference's dynamic_glb files
    p = G.write_mesh_glb(str(tmp_path / "dynamic_glb" / "frame_0.glb"), verts, faces, vertex_colors=colours)
    doc, blob = parse_glb(p)
    prim = doc["meshes"][0]["primitives"][0]
    assert set(prim["attributes"]) == {"POSITION", "COLOR_0"} and prim["mode"] == 4 and "images" not in doc
    pos, acc = accessor(doc, blob, prim["attributes"]["POSITION"], "<f4", 3)
    assert acc["componentType"] == 5126 and acc["type"] == "VEC3" and acc["count"] == V and np.array_equal(pos, verts)
    assert acc["min"] == [float(x) for x in verts.min(0)] and acc["max"] == [float(x) for x in verts.max(0)]
    col, acc = accessor(doc, blob, prim["attributes"]["COLOR_0"], "u1", 4)
    assert acc["componentType"] == 5121 and acc["normalized"] is True and acc["count"] == V
    assert np.array_equal(col[:, :3], np.clip(colours * 255, 0, 255).astype(np.uint8)) and (col[:, 3] == 255).all()
    idx, acc = accessor(doc, blob, prim["indices"], "<u4", 1)
    assert acc["componentType"] == 5125 and acc["type"] == "SCALAR" and acc["count"] == 3 * F and np.array_equal(idx.reshape(-1, 3), faces)
    back = G.read_mesh_glb(p)
    assert np.array_equal(back["verts"], verts) and np.array_equal(back["faces"], faces) and np.array_equal(back["colors"], col)
    assert back["uv"] is None and back["tex"] is None
    # textured: un-indexed, the PNG embedded
    p = G.write_mesh_glb(str(tmp_path / "ball.glb"), verts, faces, uv=uv, tex=tex)
    doc, blob = parse_glb(p)
    prim = doc["meshes"][0]["primitives"][0]
    assert set(prim["attributes"]) == {"POSITION", "TEXCOORD_0"}
    pos, acc = accessor(doc, blob, prim["attributes"]["POSITION"], "<f4", 3)
    assert acc["count"] == 3 * F and np.array_equal(pos, verts[faces.reshape(-1)])
    assert acc["min"] == [float(x) for x in verts[faces.reshape(-1)].min(0)] and acc["max"] == [float(x) for x in verts[faces.reshape(-1)].max(0)]
    st, acc = accessor(doc, blob, prim["attributes"]["TEXCOORD_0"], "<f4", 2)
    assert acc["type"] == "VEC2" and acc["count"] == 3 * F and np.array_equal(st, uv.reshape(-1, 2))  # no flip: glTF's origin is top-left
    idx, acc = accessor(doc, blob, prim["indices"], "<u4", 1)
    assert acc["count"] == 3 * F and np.array_equal(idx[:, 0], np.arange(3 * F))
    mat = doc["materials"][prim["material"]]["pbrMetallicRoughness"]
    assert mat["baseColorTexture"] == {"index": 0} and doc["textures"] == [{"sampler": 0, "source": 0}]
    image = doc["images"][0]
    assert image["mimeType"] == "image/png"
    bv = doc["bufferViews"][image["bufferView"]]
    png = blob[bv["byteOffset"]:bv["byteOffset"] + bv["byteLength"]]
    want = np.clip(tex * 255, 0, 255).astype(np.uint8)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(png)).convert("RGB")), want)
    assert np.array_equal(pkg("png_io").read_png_host(png), want)
    back = G.read_mesh_glb(p)
    assert np.array_equal(back["uv"], uv) and np.array_equal(back["tex"], want) and back["colors"] is None
    got = centroid_colours(back["tex"], back["uv"])
    assert np.abs(got - colours.astype(np.float64)[faces].mean(1)).max() <= 1.01 / 255
    with pytest.raises(ValueError, match="go together"):
        G.write_mesh_glb(str(tmp_path / "x.glb"), verts, faces, uv=uv)
    with pytest.raises(ValueError, match="not both"):
        G.write_mesh_glb(str(tmp_path / "x.glb"), verts, faces, vertex_colors=colours, uv=uv, tex=tex)
    with pytest.raises(ValueError, match="out of range"):
        G.write_mesh_glb(str(tmp_path / "x.glb"), verts, faces + 1)
    (tmp_path / "bad.glb").write_bytes(b"glTF" + b"\0" * 30)
    with pytest.raises(ValueError, match="not a binary glTF"):
        G.read_mesh_glb(str(tmp_path / "bad.glb"))


def test_read_png_host_undoes_every_filter(tmp_path):
    """read_png_host on a file PIL wrote (PIL picks filters per row) equals PIL's own decoding."""
    from PIL import Image
    PNG = pkg("png_io")
    rng = np.random.default_rng(2)
    y, x = np.mgrid[0:23, 0:31]
    img = np.stack([(x * 8) % 256, (y * 11 + x) % 256, rng.integers(0, 256, (23, 31))], -1).astype(np.uint8)
    Image.fromarray(img).save(str(tmp_path / "pil.png"), optimize=True)
    assert np.array_equal(PNG.read_png_host(str(tmp_path / "pil.png")), img)
    PNG.write_png(str(tmp_path / "own.png"), img)
    assert np.array_equal(PNG.read_png_host(str(tmp_path / "own.png")), img)
    assert open(str(tmp_path / "own.png"), "rb").read() == PNG.encode_png(img)


def test_texture_argument_errors_need_no_gpu():
    MR = pkg("mesh_raster")
    tex, uv = torch.zeros(1, 4, 4, 3), torch.zeros(1, 2, 2, 2)
    for kw in ({"uv_da": uv}, {"mip_level_bias": uv}, {"mip": [tex]}, {"max_mip_level": 2}, {"filter_mode": "linear-mipmap-linear"},
               {"filter_mode": "linear-mipmap-nearest"}):
        with pytest.raises(RuntimeError, match=r"texture: mip-maps \(.*\) are not supported"):
            MR.texture(tex, uv, **kw)
    with pytest.raises(RuntimeError, match="texture: cube maps .* are not supported"):
        MR.texture(tex, uv, boundary_mode="cube")
    with pytest.raises(RuntimeError, match="filter_mode must be one of"):
        MR.texture(tex, uv, filter_mode="cubic")
    with pytest.raises(RuntimeError, match="boundary_mode must be one of"):
        MR.texture(tex, uv, boundary_mode="mirror")
    with pytest.raises(RuntimeError, match="no CPU path"):
        MR.texture(tex, uv)
    import inspect
    assert list(inspect.signature(MR.texture).parameters) == ["tex", "uv", "uv_da", "mip_level_bias", "mip", "filter_mode", "boundary_mode",
                                                              "max_mip_level"]
    assert list(inspect.signature(MR.render_mesh_textured).parameters) == ["glctx", "verts", "faces", "uv", "tex", "cam", "resolution",
                                                                           "whitebackground", "rast"]
    lib = pkg("_lib").lib()
    assert lib.dgm_tri_texture_forward(5, 0, 4, 3, 1, 0, None, None, None, None) != 0 and b"within [1, 16384]" in lib.dgm_last_error()
    assert lib.dgm_tri_texture_forward(5, 4, 4, 3, 2, 0, None, None, None, None) != 0 and b"filter" in lib.dgm_last_error()
    assert lib.dgm_tri_texture_forward(5, 4, 4, 3, 1, 3, None, None, None, None) != 0 and b"boundary" in lib.dgm_last_error()
    assert lib.dgm_tri_texture_forward(0, 4, 4, 3, 1, 0, None, None, None, None) == 0  # n == 0 is a no-op
    assert lib.dgm_tri_texture_forward(5, 4, 4, 3, 1, 0, None, None, None, None) != 0 and b"NULL" in lib.dgm_last_error()
    assert lib.dgm_atlas_uv(0, 64, 4, None, None) == 0
    assert lib.dgm_atlas_uv(10, 64, 3, None, None) != 0 and b"cell" in lib.dgm_last_error()
    assert lib.dgm_atlas_uv(10, 20000, 4, None, None) != 0 and b"size" in lib.dgm_last_error()
    assert lib.dgm_atlas_uv(33, 16, 4, None, None) != 0 and b"more face pairs than cells" in lib.dgm_last_error()  # 17 pairs, 16 cells
    assert lib.dgm_atlas_uv(32, 16, 4, None, None) != 0 and b"NULL" in lib.dgm_last_error()
    assert lib.dgm_atlas_interpolate(3, 33, 3, 16, 4, None, None, None, None, None) != 0 and b"more face pairs" in lib.dgm_last_error()
