"""PLY checkpoint format of the Gaussian set: same four elements, property names and order as the reference writes with
plyfile (R/scene/gaussian_model_dpsr_dynamic_anchor.py:238-289 save_ply, :296-362 load_ply):

    element vertex P            x y z nx ny nz f_dc_0..2 f_rest_0..44 opacity scale_0..2 rot_0..3       (float32)
    element density_thres 1     density_thres
    element gaussian_center 1   gaussian_center_x gaussian_center_y gaussian_center_z
    element gaussian_scale 1    gaussian_scale

binary_little_endian 1.0 (plyfile's default for PlyData.write).  f_dc / f_rest are stored channel-major, i.e. the
(P, coeffs, 3) parameter transposed to (P, 3, coeffs) and flattened.  plyfile is not a dependency: the format is a text
header followed by packed little-endian records, read / written here with numpy structured arrays (scalar properties only,
which is all this format uses).  Reader also accepts ascii PLY and float64 / integer scalar properties.
"""
import os

import numpy as np

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}
_NP_TO_PLY = {"f4": "float", "f8": "double", "i4": "int", "u1": "uchar", "i2": "short", "u2": "ushort", "u4": "uint", "i1": "char"}


def write_ply(path, elements):
    """elements: list of (name, structured ndarray).  binary_little_endian, plyfile-style header."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    head = ["ply", "format binary_little_endian 1.0"]
    for name, arr in elements:
        head.append(f"element {name} {len(arr)}")
        for field in arr.dtype.names:
            head.append(f"property {_NP_TO_PLY[arr.dtype[field].str[1:]]} {field}")
    head.append("end_header")
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        for _, arr in elements:
            fh.write(np.ascontiguousarray(arr.astype(arr.dtype.newbyteorder("<"))).tobytes())


def read_ply(path):
    """-> dict name -> structured ndarray (in file order: use list(result) for positional access like plydata.elements[i])."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header")
    end = data.index(b"\n", end) + 1
    lines = data[:end].decode("ascii").splitlines()
    if lines[0].strip() != "ply":
        raise ValueError(f"{path}: not a PLY file")
    fmt, elems = None, []
    for ln in lines[1:]:
        tok = ln.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elems.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if tok[1] == "list":
                raise ValueError(f"{path}: list properties are not part of this checkpoint format")
            elems[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
    out, off = {}, end
    if fmt == "ascii":
        toks = data[end:].split()
        pos = 0
        for name, n, props in elems:
            arr = np.empty(n, dtype=[(p, t) for p, t in props])
            for i in range(n):
                for p, t in props:
                    arr[p][i] = np.array(toks[pos].decode(), dtype=t)
                    pos += 1
            out[name] = arr
        return out
    bo = "<" if fmt == "binary_little_endian" else ">"
    for name, n, props in elems:
        dt = np.dtype([(p, bo + t) for p, t in props])
        out[name] = np.frombuffer(data, dtype=dt, count=n, offset=off).copy()
        off += n * dt.itemsize
    return out


def attribute_names(n_dc, n_rest, n_scale=3, n_rot=4):
    """construct_list_of_attributes (:238-251)."""
    return (["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(n_dc)] + [f"f_rest_{i}" for i in range(n_rest)]
            + ["opacity"] + [f"scale_{i}" for i in range(n_scale)] + [f"rot_{i}" for i in range(n_rot)])


def save_gaussians(path, xyz, normal, f_dc, f_rest, opacity, scaling, rotation, density_thres=0.0, gaussian_center=(0.0, 0.0, 0.0),
                   gaussian_scale=1.0):
    """All arrays numpy float32: f_dc (P, 1, 3), f_rest (P, 15, 3) as the model keeps them."""
    P = xyz.shape[0]
    dc = np.transpose(f_dc, (0, 2, 1)).reshape(P, -1)
    rest = np.transpose(f_rest, (0, 2, 1)).reshape(P, -1)
    names = attribute_names(dc.shape[1], rest.shape[1], scaling.shape[1], rotation.shape[1])
    table = np.concatenate((xyz, normal, dc, rest, opacity.reshape(P, 1), scaling, rotation), axis=1).astype(np.float32)
    vertex = np.empty(P, dtype=[(n, "<f4") for n in names])
    for i, n in enumerate(names):
        vertex[n] = table[:, i]
    one = lambda fields, vals: np.array([tuple(np.float32(v) for v in vals)], dtype=[(f, "<f4") for f in fields])
    write_ply(path, [("vertex", vertex), ("density_thres", one(["density_thres"], [density_thres])),
                     ("gaussian_center", one(["gaussian_center_x", "gaussian_center_y", "gaussian_center_z"], gaussian_center)),
                     ("gaussian_scale", one(["gaussian_scale"], [gaussian_scale]))])


def load_gaussians(path, max_sh_degree=3):
    """-> dict of float32 arrays in the model's layout (+ density_thres, gaussian_center, gaussian_scale).  A plain
    3D-GS PLY (vertex element only) loads too; the three extra elements then default like a fresh model."""
    ply = read_ply(path)
    v = ply["vertex"] if "vertex" in ply else ply[list(ply)[0]]
    col = lambda n: np.asarray(v[n], np.float32)
    P = len(v)
    xyz = np.stack((col("x"), col("y"), col("z")), 1)
    normal = np.stack((col("nx"), col("ny"), col("nz")), 1) if "nx" in v.dtype.names else np.zeros((P, 3), np.float32)
    f_dc = np.stack((col("f_dc_0"), col("f_dc_1"), col("f_dc_2")), 1).reshape(P, 3, 1)
    rest_names = sorted((n for n in v.dtype.names if n.startswith("f_rest_")), key=lambda n: int(n.split("_")[-1]))
    if len(rest_names) != 3 * (max_sh_degree + 1) ** 2 - 3:
        raise ValueError(f"{path}: {len(rest_names)} f_rest properties do not match sh degree {max_sh_degree}")
    f_rest = np.stack([col(n) for n in rest_names], 1).reshape(P, 3, (max_sh_degree + 1) ** 2 - 1)
    scale_names = sorted((n for n in v.dtype.names if n.startswith("scale_")), key=lambda n: int(n.split("_")[-1]))
    rot_names = sorted((n for n in v.dtype.names if n.startswith("rot")), key=lambda n: int(n.split("_")[-1]))
    out = dict(xyz=xyz, normal=normal, features_dc=np.ascontiguousarray(np.transpose(f_dc, (0, 2, 1))),
               features_rest=np.ascontiguousarray(np.transpose(f_rest, (0, 2, 1))), opacity=col("opacity").reshape(P, 1),
               scaling=np.stack([col(n) for n in scale_names], 1), rotation=np.stack([col(n) for n in rot_names], 1),
               density_thres=np.float32(0.0), gaussian_center=np.zeros(3, np.float32), gaussian_scale=np.float32(1.0))
    if "density_thres" in ply:
        out["density_thres"] = np.float32(ply["density_thres"]["density_thres"][0])
    if "gaussian_center" in ply:
        c = ply["gaussian_center"]
        out["gaussian_center"] = np.array([c["gaussian_center_x"][0], c["gaussian_center_y"][0], c["gaussian_center_z"][0]], np.float32)
    if "gaussian_scale" in ply:
        out["gaussian_scale"] = np.float32(ply["gaussian_scale"]["gaussian_scale"][0])
    return out


# ---- triangle meshes (export_mesh, R/scene/gaussian_model_dpsr_dynamic_anchor.py:831-856) ----------------------------------------
# binary_little_endian: `element vertex V` with float x y z, `element face F` with `property list uchar int vertex_indices`, the
# layout MeshLab, trimesh and Open3D read.  (A separate pair from write_ply / read_ply: the checkpoint format has no list
# properties and read_ply keeps refusing them.)
def write_mesh_ply(path, verts, faces, vertex_colors=None):
    """verts (V, 3) float, faces (F, 3) int (numpy arrays or tensors on any device).  vertex_colors: (V, 3) floats in [0, 1]; the
    vertex element then gains `uchar red green blue alpha`, the layout trimesh writes, quantised as testing() does
    (R/train.py:730-731: clip(c * 255, 0, 255) truncated) with alpha 255."""
    as_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    v = np.ascontiguousarray(as_np(verts), dtype="<f4").reshape(-1, 3)
    f = np.asarray(as_np(faces)).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("write_mesh_ply: face index out of range")
    rec = np.empty(len(f), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    rec["n"], rec["idx"] = 3, f
    colour_props = []
    if vertex_colors is not None:
        c = np.asarray(as_np(vertex_colors)).reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError(f"write_mesh_ply: {len(v)} vertices but {len(c)} colours")
        vc = np.empty(len(v), dtype=[("xyz", "<f4", (3,)), ("rgba", "u1", (4,))])
        vc["xyz"] = v
        vc["rgba"][:, :3] = np.clip(c * 255, 0, 255).astype(np.uint8)
        vc["rgba"][:, 3] = 255
        v = vc
        colour_props = [f"property uchar {k}" for k in ("red", "green", "blue", "alpha")]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y",
            "property float z"] + colour_props + [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(v.tobytes())
        fh.write(rec.tobytes())


def read_mesh_ply(path, return_colors=False):
    """-> verts (V, 3) float32, faces (F, 3) int32 of a binary little-endian triangle-mesh PLY as write_mesh_ply writes it; with
    return_colors also the (V, 4) uint8 red green blue alpha of the vertices, or None when the file has none."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"\n", data.index(b"end_header")) + 1
    lines = [ln.split() for ln in data[:end].decode("ascii").splitlines()]
    if lines[0] != ["ply"] or ["format", "binary_little_endian", "1.0"] not in lines:
        raise ValueError(f"{path}: not a binary little-endian PLY")
    elems = []
    for tok in lines:
        if tok and tok[0] == "element":
            elems.append((tok[1], int(tok[2]), []))
        elif tok and tok[0] == "property":
            elems[-1][2].append(tok[1:])
    by = {name: (n, props) for name, n, props in elems}
    nv, vprops = by["vertex"]
    if [p[-1] for p in vprops][:3] != ["x", "y", "z"] or any(p[0] == "list" for p in vprops):
        raise ValueError(f"{path}: vertex element must start with x y z scalars")
    vdt = np.dtype([(p[1], "<" + _PLY_TYPES[p[0]]) for p in vprops])
    off = end
    v = np.frombuffer(data, dtype=vdt, count=nv, offset=off)
    off += nv * vdt.itemsize
    verts = np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32)
    nf, fprops = by.get("face", (0, []))
    if nf and fprops != [["list", "uchar", "int", "vertex_indices"]] and fprops != [["list", "uchar", "int", "vertex_index"]]:
        raise ValueError(f"{path}: face element must be `property list uchar int vertex_indices`")
    f = np.frombuffer(data, dtype=[("n", "u1"), ("idx", "<i4", (3,))], count=nf, offset=off)
    if nf and (f["n"] != 3).any():
        raise ValueError(f"{path}: only triangles are supported")
    faces = f["idx"].astype(np.int32).reshape(-1, 3)
    if not return_colors:
        return verts, faces
    rgba = ("red", "green", "blue", "alpha")
    colors = np.stack([v[k] for k in rgba], 1).astype(np.uint8) if all(k in vdt.names for k in rgba) else None
    return verts, faces, colors


def read_mesh_ply_on_device(path, device):
    """read_mesh_ply for the command lines of the mesh tools: verts (V, 3) float32, faces (F, 3) int32 and colours (V, 3) float32,
    tensors on `device`; colours None when the file has none.  The byte k is read as (k + 0.5) / 255: write_mesh_ply and the
    texture writers quantise floats in [0, 1] as clip(c * 255) truncated, which gives k back for every byte k, so a tool that does
    not touch a colour writes the byte it read."""
    import torch
    verts, faces, colors = read_mesh_ply(path, return_colors=True)
    if colors is not None:
        colors = torch.from_numpy((colors[:, :3].astype(np.float32) + np.float32(0.5)) / np.float32(255.0)).to(device)
    return torch.from_numpy(verts).to(device), torch.from_numpy(faces).to(device), colors


# ---- point clouds with normals (pointcloud_init.ply of normal_initialization, R/scene/gaussian_model_dpsr_dynamic_anchor.py:722-729) --
def write_pointcloud_ply(path, points, normals):
    """points (N, 3), normals (N, 3) (numpy arrays or tensors on any device) as `element vertex N` with float x y z nx ny nz,
    binary_little_endian -- the layout Open3D's write_point_cloud produces for a cloud with normals, up to its double precision."""
    as_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    p = np.asarray(as_np(points), np.float32).reshape(-1, 3)
    n = np.asarray(as_np(normals), np.float32).reshape(-1, 3)
    if len(p) != len(n):
        raise ValueError(f"write_pointcloud_ply: {len(p)} points but {len(n)} normals")
    vertex = np.empty(len(p), dtype=[(k, "<f4") for k in ("x", "y", "z", "nx", "ny", "nz")])
    for i, k in enumerate(("x", "y", "z")):
        vertex[k], vertex["n" + k] = p[:, i], n[:, i]
    write_ply(path, [("vertex", vertex)])


def read_pointcloud_ply(path):
    """-> points (N, 3) float32, normals (N, 3) float32 of a PLY as write_pointcloud_ply writes it."""
    v = read_ply(path)["vertex"]
    col = lambda k: np.asarray(v[k], np.float32)
    return np.stack([col("x"), col("y"), col("z")], 1), np.stack([col("nx"), col("ny"), col("nz")], 1)
