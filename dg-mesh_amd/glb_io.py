"""Binary glTF 2.0 (.glb) writer and reader for one triangle mesh: the dynamic_glb/frame_{idx}.glb files of the reference's testing()
(R/train.py:740, trimesh's exporter there) and the textured export of mesh_texture.py.  Standard library + numpy only; trimesh and
pygltflib are neither vendored nor dependencies, and the files have not been checked against an external loader.

What a file holds: one scene, one node, one mesh with ONE primitive (mode 4, triangles) over ONE buffer, the GLB's BIN chunk:
  POSITION    float32 VEC3 with min / max (the specification requires them);
  indices     uint32 SCALAR;
  and either  COLOR_0 uint8 VEC4 normalised -- the bytes ply_io.write_mesh_ply stores: clamp(c, 0, 1) * 255 truncated, alpha 255 --
  or          TEXCOORD_0 float32 VEC2 with the PNG (png_io.write_png's bytes) embedded as a buffer view behind the material's
              baseColorTexture, sampled LINEAR with CLAMP_TO_EDGE.  glTF's uv origin is the top-left corner of the image, which is
              this project's (mesh_raster.texture), so uv is stored as it is.  A texture coordinate belongs to a vertex in glTF, so the
              textured form is un-indexed: 3F vertices, indices 0 .. 3F - 1.
The material is unlit-looking PBR: base colour 1, metallic 0, roughness 1.  Every buffer view starts on a 4-byte boundary and both
chunks are padded to 4 bytes (JSON with spaces, BIN with zeros).  Nothing else of glTF -- normals, animation, several meshes, sparse
accessors, extensions, external buffers -- is written or read."""
import json
import os
import struct

import numpy as np

from .obj_io import _np, texture_bytes
from .png_io import encode_png, read_png_host

MAGIC, JSON_CHUNK, BIN_CHUNK = 0x46546C67, 0x4E4F534A, 0x004E4942
FLOAT, UBYTE, UINT = 5126, 5121, 5125
ARRAY_BUFFER, ELEMENT_ARRAY_BUFFER = 34962, 34963


def write_mesh_glb(path, verts, faces, *, vertex_colors=None, uv=None, tex=None):
    """verts (V, 3), faces (F, 3) (numpy arrays or tensors on any device) and either vertex_colors (V, 3) floats in [0, 1], or uv
    (F, 3, 2) per face corner together with tex (H, W, 3) uint8 or floats in [0, 1], or neither (a bare mesh).  Module docstring for
    the layout."""
    v = np.ascontiguousarray(_np(verts), dtype="<f4").reshape(-1, 3)
    f = np.asarray(_np(faces)).reshape(-1, 3).astype(np.int64)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("write_mesh_glb: face index out of range")
    if (uv is None) != (tex is None):
        raise ValueError("write_mesh_glb: uv and tex go together")
    if uv is not None and vertex_colors is not None:
        raise ValueError("write_mesh_glb: either vertex_colors or uv + tex, not both")
    views, accessors, blob = [], [], bytearray()

    def view(data, target=None):
        blob.extend(b"\0" * (-len(blob) % 4))
        views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": len(data)})
        if target is not None:
            views[-1]["target"] = target
        blob.extend(data)
        return len(views) - 1

    def accessor(array, ctype, kind, target, **extra):
        accessors.append(dict({"bufferView": view(array.tobytes(), target), "componentType": ctype, "count": int(array.shape[0]), "type": kind},
                              **extra))
        return len(accessors) - 1

    attributes, material = {}, {"pbrMetallicRoughness": {"baseColorFactor": [1.0, 1.0, 1.0, 1.0], "metallicFactor": 0.0, "roughnessFactor": 1.0}}
    doc = {"asset": {"version": "2.0", "generator": "dgmesh_amd.glb_io"}, "scene": 0, "scenes": [{"nodes": [0]}], "nodes": [{"mesh": 0}]}
    if uv is not None:
        t = np.asarray(_np(uv), dtype="<f4")
        if t.shape != (len(f), 3, 2):
            raise ValueError(f"write_mesh_glb: uv must be ({len(f)}, 3, 2), one row per face corner, got {t.shape}")
        v = np.ascontiguousarray(v[f.reshape(-1)])
        f = np.arange(len(v), dtype=np.int64).reshape(-1, 3)
    bounds = {"min": [float(x) for x in v.min(0)], "max": [float(x) for x in v.max(0)]} if len(v) else {}
    attributes["POSITION"] = accessor(v, FLOAT, "VEC3", ARRAY_BUFFER, **bounds)
    if uv is not None:
        attributes["TEXCOORD_0"] = accessor(np.ascontiguousarray(t.reshape(-1, 2)), FLOAT, "VEC2", ARRAY_BUFFER)
    if vertex_colors is not None:
        c = np.asarray(_np(vertex_colors)).reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError(f"write_mesh_glb: {len(v)} vertices but {len(c)} colours")
        rgba = np.full((len(v), 4), 255, np.uint8)
        rgba[:, :3] = np.clip(c * 255, 0, 255).astype(np.uint8)
        attributes["COLOR_0"] = accessor(rgba, UBYTE, "VEC4", ARRAY_BUFFER, normalized=True)
    indices = accessor(np.ascontiguousarray(f.reshape(-1), dtype="<u4"), UINT, "SCALAR", ELEMENT_ARRAY_BUFFER)
    if uv is not None:
        doc["images"] = [{"bufferView": view(encode_png(texture_bytes(tex))), "mimeType": "image/png"}]
        doc["samplers"] = [{"magFilter": 9729, "minFilter": 9729, "wrapS": 33071, "wrapT": 33071}]
        doc["textures"] = [{"sampler": 0, "source": 0}]
        material["pbrMetallicRoughness"]["baseColorTexture"] = {"index": 0}
    blob.extend(b"\0" * (-len(blob) % 4))
    doc.update({"meshes": [{"primitives": [{"attributes": attributes, "indices": indices, "material": 0, "mode": 4}]}], "materials": [material],
                "accessors": accessors, "bufferViews": views, "buffers": [{"byteLength": len(blob)}]})
    text = json.dumps(doc, separators=(",", ":")).encode("utf-8")
    text += b" " * (-len(text) % 4)
    total = 12 + 8 + len(text) + 8 + len(blob)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<III", MAGIC, 2, total) + struct.pack("<II", len(text), JSON_CHUNK) + text
                 + struct.pack("<II", len(blob), BIN_CHUNK) + bytes(blob))
    return path


_KIND = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4}
_CTYPE = {FLOAT: "<f4", UBYTE: "u1", UINT: "<u4", 5123: "<u2"}


def read_mesh_glb(path):
    """A file of write_mesh_glb back: {"verts" (n, 3) float32, "faces" (F, 3) int32, "colors" (n, 4) uint8 or None, "uv" (F, 3, 2)
    float32 or None (the vertices' TEXCOORD_0 gathered per face corner), "tex" (H, W, 3) uint8 or None, "json": the document}.
    ValueError for anything that is not a GLB of version 2 with a JSON and a BIN chunk and tightly packed accessors."""
    with open(path, "rb") as fh:
        data = fh.read()
    if len(data) < 20 or struct.unpack_from("<III", data, 0)[:2] != (MAGIC, 2) or struct.unpack_from("<I", data, 8)[0] != len(data):
        raise ValueError(f"{path}: not a binary glTF 2.0 file")
    n_json, kind = struct.unpack_from("<II", data, 12)
    if kind != JSON_CHUNK:
        raise ValueError(f"{path}: the first chunk is not JSON")
    doc = json.loads(data[20:20 + n_json].decode("utf-8"))
    n_bin, kind = struct.unpack_from("<II", data, 20 + n_json)
    if kind != BIN_CHUNK:
        raise ValueError(f"{path}: the second chunk is not BIN")
    blob = data[28 + n_json:28 + n_json + n_bin]

    def view(i):
        bv = doc["bufferViews"][i]
        if "byteStride" in bv:
            raise ValueError(f"{path}: interleaved buffer views are not supported")
        return blob[bv.get("byteOffset", 0):bv.get("byteOffset", 0) + bv["byteLength"]]

    def array(i):
        acc = doc["accessors"][i]
        a = np.frombuffer(view(acc["bufferView"]), dtype=_CTYPE[acc["componentType"]], count=acc["count"] * _KIND[acc["type"]],
                          offset=acc.get("byteOffset", 0))
        return a.reshape(acc["count"], _KIND[acc["type"]])

    prim = doc["meshes"][0]["primitives"][0]
    att = prim["attributes"]
    verts = array(att["POSITION"]).astype(np.float32)
    faces = array(prim["indices"]).astype(np.int32).reshape(-1, 3)
    colors = array(att["COLOR_0"]).astype(np.uint8) if "COLOR_0" in att else None
    uv = array(att["TEXCOORD_0"]).astype(np.float32)[faces] if "TEXCOORD_0" in att else None
    tex = None
    if doc.get("images"):
        tex = read_png_host(bytes(view(doc["images"][0]["bufferView"])))[..., :3]
    return {"verts": verts, "faces": faces, "colors": colors, "uv": uv, "tex": tex, "json": doc}
