"""GPU tests of the texture atlas (dg-mesh_amd/mesh_texture.py: atlas_uv, atlas_interpolate; csrc/mesh_texture.hip) against the numpy
restatement (tests/_texture_ref.py).  face_id and uv equal the fp32 restatement bit for bit (integer logic and one correctly rounded
division); the values are held to 8 x the largest |ref32 - ref64| of the case, the rule of tests/test_mesh_inside.py -- and, the
kernel being three products and two adds without contraction, also equal the fp32 restatement's bits."""
import functools

import numpy as np
import pytest
import torch

import _edges_ref as E
import _texture_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_FACTOR = 8.0
FACES = [1, 2, 7, 320]
CELLS = [4, 5, 16]


def MT():
    return pkg("mesh_texture")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


@functools.lru_cache(maxsize=None)
def mesh(F):
    """icosphere(2) for 320 faces, its first F faces otherwise; a 5-channel attribute."""
    verts, faces = E.icosphere(2)
    faces = faces[:F].copy()
    attr = np.random.default_rng(F).standard_normal((len(verts), 5)).astype(np.float32)
    for a in (verts, faces, attr):
        a.setflags(write=False)
    return verts, faces, attr


def same_bits(t, a):
    return t.shape == a.shape and np.array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(a).view(np.uint32))


def check(atlas, attr, faces, what):
    M = MT()
    uv = M.atlas_uv(atlas, DEV)
    out, face_id = M.atlas_interpolate(atlas, dev(attr), dev(faces))
    F, C = len(faces), attr.shape[1]
    assert uv.shape == (F, 3, 2) and uv.dtype == torch.float32
    assert out.shape == (atlas.size, atlas.size, C) and face_id.shape == (atlas.size, atlas.size) and face_id.dtype == torch.int32
    assert same_bits(uv, R.atlas_uv(F, atlas.size, atlas.cell, np.float32)), f"{what}: uv"
    ref32, id32 = R.atlas_interpolate(attr, faces, atlas.size, atlas.cell, np.float32)
    ref64, _ = R.atlas_interpolate(attr, faces, atlas.size, atlas.cell, np.float64)
    assert np.array_equal(face_id.cpu().numpy(), id32), f"{what}: face_id"
    got = out.cpu().numpy()
    nan = np.isnan(ref64)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs"
    ref_err = float(np.abs(np.where(nan, 0, ref32.astype(np.float64) - ref64)).max())
    err = float(np.abs(np.where(nan, 0, got.astype(np.float64) - ref64)).max())
    print(f"{what}: size {atlas.size} cell {atlas.cell}: device max |out - ref64| {err:.3e}; numpy fp32 statement {ref_err:.3e}, factor "
          f"{TOL_FACTOR:g}, tolerance {TOL_FACTOR * ref_err:.3e}; owned texels {(id32 >= 0).mean():.1%}")
    assert err <= TOL_FACTOR * ref_err
    assert np.array_equal(got.view(np.uint32)[~nan], ref32.view(np.uint32)[~nan]), f"{what}: values differ from the fp32 restatement's bits"
    again, again_id = M.atlas_interpolate(atlas, dev(attr), dev(faces))
    assert np.array_equal(again.cpu().numpy().view(np.uint32)[~nan], got.view(np.uint32)[~nan]) and np.array_equal(again_id.cpu().numpy(), id32)
    return got, id32, uv.cpu().numpy()


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("F", FACES)
def test_atlas_against_the_restatement(F, cell):
    verts, faces, attr = mesh(F)
    atlas = MT().build_atlas(F, cell=cell)
    got, ids, uv = check(atlas, attr, faces, f"F {F}")
    # every face owns texels, its corners' texels among them, holding the corners' attributes exactly (b = 1, 0, 0)
    assert set(np.unique(ids)) - {-1} == set(range(F))
    px = np.round(uv * atlas.size - 0.5).astype(np.int64)  # (F, 3, 2) texel indices of the corners
    assert np.array_equal(ids[px[..., 1], px[..., 0]], np.repeat(np.arange(F)[:, None], 3, 1))
    assert np.array_equal(got[px[..., 1], px[..., 0]], attr[faces])
    assert not got[ids < 0].any()


def test_a_size_that_is_no_multiple_of_the_cell():
    verts, faces, attr = mesh(320)
    atlas = MT().build_atlas(320, size=72)  # 72 // 13 = 5 texels a cell, 14 whole cells a row, a margin of 2 texels
    assert atlas == MT().Atlas(72, 5, 14, 320)
    got, ids, _ = check(atlas, attr, faces, "size 72")
    assert (ids[70:] == -1).all() and (ids[:, 70:] == -1).all() and not got[70:].any() and not got[:, 70:].any()
    verts, faces, attr = mesh(7)
    atlas = MT().build_atlas(7, size=23)  # 2 cells of 11: one texel of margin
    assert (atlas.cell, atlas.cells_per_row) == (11, 2)
    got, ids, _ = check(atlas, attr, faces, "size 23")
    assert (ids[22] == -1).all() and (ids[:, 22] == -1).all() and not got[22].any() and not got[:, 22].any()


def test_bad_faces_and_nan_vertices():
    verts, faces, attr = mesh(320)
    faces, attr = faces.copy(), attr.copy()
    V = len(verts)
    faces[3, 1], faces[10, 0], faces[11, 2] = -1, V, 2 ** 31 - 1   # indices outside [0, V): those faces own nothing
    attr[int(faces[40, 0])] = np.nan                               # a NaN vertex: NaN on the texels of its faces, nowhere else
    atlas = MT().build_atlas(320, cell=5)
    got, ids, _ = check(atlas, attr, faces, "bad faces")
    assert not np.isin(ids, [3, 10, 11]).any()
    uses = (faces == faces[40, 0]).any(1)
    uses[[3, 10, 11]] = False
    nan_texels = np.isnan(got).any(-1)
    assert nan_texels.any() and np.isin(ids[nan_texels], np.nonzero(uses)[0]).all()
    clean = mesh(320)
    ref, _ = R.atlas_interpolate(clean[2], clean[1], atlas.size, atlas.cell, np.float32)
    untouched = ~np.isin(ids, np.nonzero(uses)[0]) & (ids >= 0)
    assert np.array_equal(got[untouched], ref[untouched])


def test_empty_and_argument_errors():
    M = MT()
    verts, faces, attr = mesh(7)
    atlas = M.build_atlas(0, cell=4)
    out, ids = M.atlas_interpolate(atlas, dev(attr), dev(faces[:0]))
    assert out.shape == (4, 4, 5) and not out.any() and bool((ids == -1).all()) and M.atlas_uv(atlas, DEV).shape == (0, 3, 2)
    out, ids = M.atlas_interpolate(M.build_atlas(7, cell=4), dev(attr[:0]), dev(faces))  # no vertices: every index is outside
    assert not out.any() and bool((ids == -1).all())
    with pytest.raises(ValueError, match="built for 7 faces"):
        M.atlas_interpolate(M.build_atlas(7, cell=4), dev(attr), dev(faces[:3]))
    with pytest.raises(RuntimeError, match="float32 and faces int32"):
        M.atlas_interpolate(M.build_atlas(7, cell=4), dev(attr), dev(faces).long())
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.atlas_interpolate(M.build_atlas(7, cell=4), torch.from_numpy(attr.copy()), torch.from_numpy(faces.copy()))
    with pytest.raises(RuntimeError, match="more face pairs than cells"):
        M.atlas_uv(M.Atlas(8, 4, 2, 9), DEV)  # a hand-made atlas too small for its faces: the library refuses
