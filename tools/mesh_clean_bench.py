"""Timer of mesh cleaning (mesh_clean.connected_components / clean_mesh; informational) on a mesh of the mesh phase's size: DiffMC of
a synthetic two-body field on the 288^3 grid with 500 small blobs around the bodies.

    timeout 600 python tools/mesh_clean_bench.py [--res 288] [--blobs 500] [--iters 7]

Reports the median of `iters` runs after a warm-up, in HIP events on the stream and as wall time with a synchronisation (both
entry points read a few bytes back, so the wall time is what a caller sees): connected_components, clean_mesh(largest=True), and
the kernels' stages alone (label, stats, select, compaction).  The hooking is the single-pass lock-free form: one hooking launch
and one labelling launch whatever the mesh, so `hook_launches` is 1 by construction.  For orientation, the host route the
reference takes -- mesh to the host, labelling there (scipy.sparse.csgraph when present, else a vectorised numpy min-label
propagation), mask, compaction, mesh back to the device -- is timed on the same mesh with a wall clock; its labels must equal the
device's.  Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _times(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    wall = []
    fn()
    torch.cuda.synchronize()
    for a, b in ev:
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2], sorted(wall)[len(wall) // 2]


def two_body_field(res, blobs, dev, seed=0):
    """Signed distance (negative inside) to a sphere and an ellipsoid-like second body, with `blobs` balls of radius 1.3 to 2.2
    voxels stamped into the free space around them."""
    ax = torch.arange(res, dtype=torch.float32, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    c1, r1 = (0.36 * res, 0.40 * res, 0.45 * res), 0.22 * res
    c2, r2 = (0.70 * res, 0.62 * res, 0.55 * res), 0.13 * res
    d1 = torch.sqrt((x - c1[0]) ** 2 + (y - c1[1]) ** 2 + (z - c1[2]) ** 2) - r1
    d2 = torch.sqrt(((x - c2[0]) / 1.3) ** 2 + (y - c2[1]) ** 2 + ((z - c2[2]) / 0.8) ** 2) - r2
    field = torch.minimum(d1, d2)
    del x, y, z, d1, d2
    rng = np.random.RandomState(seed)
    placed, w = 0, 4
    probe = field.cpu().numpy()
    while placed < blobs:
        c = rng.uniform(w + 2, res - w - 3, 3)
        i, j, k = (int(v) for v in c)
        if probe[i - w:i + w + 1, j - w:j + w + 1, k - w:k + w + 1].min() < 3.0:  # too close to a body or to another blob
            continue
        r = rng.uniform(1.3, 2.2)
        g = np.stack(np.meshgrid(*(np.arange(v - w, v + w + 1, dtype=np.float32) for v in (i, j, k)), indexing="ij"), -1)
        ball = np.linalg.norm(g - c.astype(np.float32), axis=-1) - np.float32(r)
        sl = (slice(i - w, i + w + 1), slice(j - w, j + w + 1), slice(k - w, k + w + 1))
        probe[sl] = np.minimum(probe[sl], ball)
        placed += 1
    return torch.from_numpy(probe).to(dev)


def numpy_labels(faces, V):
    """Min-label propagation with pointer jumping, vectorised (the route without scipy)."""
    lab = np.arange(V, dtype=np.int64)
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]]]).astype(np.int64)
    while True:
        a, b = lab[e[:, 0]], lab[e[:, 1]]
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        if (lo == hi).all():
            return lab.astype(np.int32)
        np.minimum.at(lab, hi, lo)
        while True:
            nxt = lab[lab]
            if (nxt == lab).all():
                break
            lab = nxt


def host_route(verts, faces):
    """verts_on_largest_mesh the reference's way: to the host, label, keep the component with the most faces, compact, back."""
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    V = len(v)
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import connected_components
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]]])
        _, comp = connected_components(sp.coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(V, V)), directed=False)
        first = np.full(comp.max() + 1, V, np.int64)
        np.minimum.at(first, comp, np.arange(V))
        lab, how = first[comp].astype(np.int32), "scipy"
    except ImportError:
        lab, how = numpy_labels(f, V), "numpy"
    per_face = lab[f[:, 0]]
    counts = np.bincount(per_face, minlength=V)
    keep = per_face == np.argmax(counts)
    used = np.zeros(V, bool)
    used[f[keep].reshape(-1)] = True
    new = np.cumsum(used) - 1
    out = (torch.from_numpy(v[used]).to(verts.device), torch.from_numpy(new[f[keep]].astype(np.int32)).to(verts.device))
    return out, lab, how


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=288)
    ap.add_argument("--blobs", type=int, default=500)
    ap.add_argument("--iters", type=int, default=7)
    args = ap.parse_args()
    M = importlib.import_module("dg-mesh_amd.mesh_clean")
    MC = importlib.import_module("dg-mesh_amd.marching_cubes")
    dev = torch.device("cuda:0")
    with torch.no_grad():
        verts, faces = MC.marching_cubes(two_body_field(args.res, args.blobs, dev), isovalue=0.0, normalize=False)
        verts, faces = verts.contiguous(), faces.contiguous()
        V, F = verts.shape[0], faces.shape[0]
        labels = M.connected_components(faces, V)
        table = M.component_table(verts, faces, labels)
        res = dict(res=args.res, V=V, F=F, components=int(table["label"].numel()), largest_faces=int(table["faces"].max()),
                   hook_launches=1)
        res["connected_components_ms"], res["connected_components_wall_ms"] = _times(lambda: M.connected_components(faces, V), args.iters)
        res["clean_mesh_largest_ms"], res["clean_mesh_largest_wall_ms"] = _times(lambda: M.clean_mesh(verts, faces, largest=True), args.iters)
        res["stats_ms"], _ = _times(lambda: M._stats(verts, faces, labels), args.iters)
        keep = M.keep_mask(verts, faces, labels, largest=True)
        res["stats_select_ms"], _ = _times(lambda: M.keep_mask(verts, faces, labels, largest=True), args.iters)
        res["compact_ms"], res["compact_wall_ms"] = _times(lambda: M.compact(verts, faces, keep), args.iters)
        cv, cf = M.clean_mesh(verts, faces, largest=True)
        res["V_clean"], res["F_clean"] = cv.shape[0], cf.shape[0]
        torch.cuda.synchronize()
        wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            (hv, hf), hlab, how = host_route(verts, faces)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        res["host_route"] = how
        res["host_route_wall_ms"] = sorted(wall)[1]
        res["host_route_over_clean_mesh"] = res["host_route_wall_ms"] / res["clean_mesh_largest_wall_ms"]
        res["labels_equal_host"] = bool(np.array_equal(hlab, labels.cpu().numpy()))
        res["clean_equal_host"] = bool(torch.equal(hv, cv) and torch.equal(hf, cf))
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
