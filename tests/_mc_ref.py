"""Plain NumPy restatement of the marching-cubes conventions (include/dgmesh_hip.h, "marching cubes"): the comparison for the HIP
kernels and the mesh checks of the CPU tests.  Reads the case table from the committed header."""
import os
import re

import numpy as np

from conftest import ROOT

HEADER = os.path.join(ROOT, "dg-mesh_amd", "csrc", "mc_tables.hpp")


def _array(text, name):
    m = re.search(name + r"\[[^=]*=\s*\{(.*?)\};", text, re.S)
    return [int(x) for x in re.findall(r"-?\d+", m.group(1))]


def load_table():
    text = open(HEADER).read()
    max_tris = int(re.search(r"#define DGM_MC_MAX_TRIS (\d+)", text).group(1))
    corner_a = np.array(_array(text, "dgm_mc_edge_corner_a"), np.int64)
    count = np.array(_array(text, "dgm_mc_tri_count"), np.int64)
    tris = np.array(_array(text, "dgm_mc_tri_table"), np.int64).reshape(256, 3 * max_tris)
    return corner_a, count, tris, max_tris


def marching_cubes(grid, iso=0.0, deform=None, normalize=True, dtype=np.float32):
    """-> verts (V, 3) `dtype`, faces (F, 3) int32, and the edge records the backward needs."""
    corner_a, count, tris, max_tris = load_table()
    f = np.asarray(grid, dtype)
    X, Y, Z = f.shape
    iso = dtype(iso)
    inside = f < iso
    N = X * Y * Z
    stride = np.array([Y * Z, Z, 1], np.int64)
    cross = np.zeros((X, Y, Z, 3), bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    flat = cross.reshape(-1)
    V = int(flat.sum())
    vid = np.full(N * 3, -1, np.int64)
    vid[flat] = np.arange(V)
    e = np.nonzero(flat)[0]
    a, axis = e // 3, e % 3
    b = a + stride[axis]
    ff = f.reshape(-1)
    idx = np.stack(np.unravel_index(np.arange(N), (X, Y, Z)), 1).astype(dtype)
    pa, pb = idx[a], idx[b]
    if deform is not None:
        dfm = np.asarray(deform, dtype).reshape(N, 3)
        pa, pb = pa + dfm[a], pb + dfm[b]
    fa, fb = ff[a], ff[b]
    t = (iso - fa) / (fb - fa)
    v = pa + t[:, None] * (pb - pa)
    scale = np.array([X - 1, Y - 1, Z - 1], dtype) if normalize else np.ones(3, dtype)
    if normalize:
        v = v / scale
    # faces: cells in linear order, then table order
    ins = inside.astype(np.int64)
    case = np.zeros((X - 1, Y - 1, Z - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= ins[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz] << c
    case = case.reshape(-1)
    ci, cj, ck = np.unravel_index(np.arange(case.size), (X - 1, Y - 1, Z - 1))
    origin = (ci * Y + cj) * Z + ck
    valid = np.arange(max_tris)[None, :] < count[case][:, None]
    cell, slot = np.nonzero(valid)
    faces = np.zeros((cell.size, 3), np.int64)
    for r in range(3):
        edge = tris[case[cell], 3 * slot + r]
        ca = corner_a[edge]
        q = origin[cell] + (ca & 1) * Y * Z + ((ca >> 1) & 1) * Z + (ca >> 2)
        faces[:, r] = vid[q * 3 + edge // 4]
    assert (faces >= 0).all()
    rec = dict(a=a, b=b, axis=axis, t=t, pa=pa, pb=pb, fa=fa, fb=fb, scale=scale, iso=iso, shape=(X, Y, Z))
    return v, faces.astype(np.int32), rec


def backward(rec, dverts, with_deform=False):
    """Analytic adjoint (float64): dgrid (X, Y, Z) and ddeform (X, Y, Z, 3) of sum(dverts * verts)."""
    X, Y, Z = rec["shape"]
    N = X * Y * Z
    du = np.asarray(dverts, np.float64) / rec["scale"].astype(np.float64)
    fa, fb = rec["fa"].astype(np.float64), rec["fb"].astype(np.float64)
    iso = float(rec["iso"])
    t = (iso - fa) / (fb - fa)
    dt = (du * (rec["pb"].astype(np.float64) - rec["pa"].astype(np.float64))).sum(1)
    den2 = (fb - fa) ** 2
    dgrid = np.zeros(N)
    np.add.at(dgrid, rec["a"], dt * (iso - fb) / den2)
    np.add.at(dgrid, rec["b"], -dt * (iso - fa) / den2)
    ddef = np.zeros((N, 3))
    np.add.at(ddef, rec["a"], (1 - t)[:, None] * du)
    np.add.at(ddef, rec["b"], t[:, None] * du)
    return dgrid.reshape(X, Y, Z), (ddef.reshape(X, Y, Z, 3) if with_deform else None)


# ---- mesh checks ------------------------------------------------------------------------------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)


def is_closed_and_oriented(faces):
    """Every directed edge appears once and its reverse once: every undirected edge lies in exactly two faces, oppositely."""
    d = directed_edges(faces)
    if len(d) == 0:
        return True
    keys = d[:, 0] * (1 << 32) + d[:, 1]
    rev = d[:, 1] * (1 << 32) + d[:, 0]
    if len(np.unique(keys)) != len(keys):
        return False
    return bool(np.isin(rev, keys).all())


def euler_characteristic(verts, faces):
    d = directed_edges(faces)
    und = np.unique(np.sort(d, 1), axis=0)
    used = np.unique(np.asarray(faces).reshape(-1))
    return len(used) - len(und) + len(faces)


def area_and_normals(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return 0.5 * np.linalg.norm(n, axis=1).sum(), n
