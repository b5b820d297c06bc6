"""The fields and the reference chain of tests/test_mesh_postprocess_chain.py: numpy only, no torch, nothing from the reference
project.  chain_field is a noisy signed field of five bodies chosen so that the post-processing chain of the exports (marching cubes,
clean, smooth, simplify, repair -- visualize.export_dynamic_mesh, MeshPhase.extract_mesh) produces the meshes the hand-built inputs
of the per-stage tests never are: vertex clustering welds the two nearly touching blobs and the two skins of the thin sheet into edges
that three or more faces share, misorients a few, and opens the surface into rims that touch (open chains), next to the one clean rim
the grid box cuts.  reference_chain runs the numpy references of every stage (tests/_mc_ref.py, _meshclean_ref.py, _edges_ref.py,
_simplify_ref.py, _repair_ref.py) in the production order and records, per stage, the mesh, the edge table's counts and what repair
reports on it."""
import functools

import numpy as np

import _edges_ref as E
import _mc_ref as MC
import _meshclean_ref as RC
import _repair_ref as RR
import _simplify_ref as RS

N, SEED = 24, 1
CLEAN = {"min_faces": 30}
SMOOTH = {"iterations": 3}  # Taubin, lam 0.5, mu -0.53, boundary "fixed": the defaults
CASES = {"grid10": {"grid": 10}, "grid16": {"grid": 16}, "target1200": {"target_faces": 1200}}
STAGES = ("mc", "clean", "smooth", "simplify", "repair")


def chain_field(n, seed):
    """(n, n, n) float32, negative inside: the minimum of five bodies plus 0.25 x standard normal noise.  With c = (n - 1) / 2: two
    spheres of radius 0.2 n at x = c - 0.22 n and x = c + 0.2 n (0.02 n apart: nearly touching), a floater of radius 0.07 n at
    y = c + 0.33 n, a sphere of radius 0.25 n centred on the face z = n - 1 (the box cuts it into an open rim) and a sheet 1.2 voxels
    thick at z = c - 0.3 n with half-width 0.3 n."""
    c = (n - 1) / 2.0
    i = np.arange(n, dtype=np.float64)
    x, y, z = np.meshgrid(i, i, i, indexing="ij")
    ball = lambda cx, cy, cz, r: np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - r
    bodies = [ball(c - 0.22 * n, c, c, 0.2 * n), ball(c + 0.2 * n, c, c, 0.2 * n), ball(c, c + 0.33 * n, c, 0.07 * n),
              ball(c, c, n - 1.0, 0.25 * n),
              np.maximum(np.maximum(np.abs(x - c), np.abs(y - c)) - 0.3 * n, np.abs(z - (c - 0.3 * n)) - 0.6)]
    field = np.minimum.reduce(bodies) + 0.25 * np.random.default_rng(seed).standard_normal((n, n, n))
    return field.astype(np.float32)


def to_unit_box(verts, n):
    """Marching-cubes vertices in lattice units -> [-1, 1]: (v - c) / (n / 2) in fp64, rounded to fp32 once."""
    return ((np.asarray(verts, np.float64) - (n - 1) / 2.0) / (n / 2.0)).astype(np.float32)


def stage(name, verts, faces, repair=None, **more):
    """One stage's record: the mesh, the edge table's counts on it, and what repair reports when it runs on it (`repaired` is then
    that repair's mesh)."""
    verts, faces = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32)
    rv, rf, info = RR.repair(verts, faces) if repair is None else repair
    out = dict(name=name, verts=verts, faces=faces, edges=E.edge_table(faces, len(verts))["info"], repair=info, repaired=(rv, rf), **more)
    for a in (verts, faces, rv, rf):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_head(n=N, seed=SEED):
    """The stages every case shares: marching cubes on chain_field, clean, smooth.  -> (field, [mc, clean, smooth])."""
    field = chain_field(n, seed)
    field.setflags(write=False)
    v, f, _ = MC.marching_cubes(field, 0.0, None, False)
    out = [stage("mc", to_unit_box(v, n), f)]
    cv, cf, vi, fi = RC.clean(out[0]["verts"], out[0]["faces"], **CLEAN)
    out.append(stage("clean", cv, cf, vert_index=vi))
    out.append(stage("smooth", E.smooth(cv, cf, **SMOOTH), cf))
    return field, out


@functools.lru_cache(maxsize=None)
def reference_chain(case, n=N, seed=SEED):
    """-> the five stage records of a case, in STAGES' order (read-only arrays, computed once)."""
    _, head = reference_head(n, seed)
    s = RS.simplify(head[-1]["verts"], head[-1]["faces"], **CASES[case])
    simplified = stage("simplify", s["verts"], s["faces"], vert_index=s["vert_index"], grid=s["grid"], grids_tried=tuple(s["grids_tried"]))
    rv, rf = simplified["repaired"]
    return head + [simplified, stage("repair", rv, rf)]


def describe(st):
    e, r = st["edges"], st["repair"]
    return (f"{st['name']:8s} V {len(st['verts'])} F {len(st['faces'])}: boundary {e['boundary_edges']} non-manifold {e['nonmanifold_edges']} "
            f"misoriented {e['misoriented_edges']}; repair on it: components {r['components']} (closed {r['closed_components']}, unorientable "
            f"{r['unorientable_components']}) flipped {r['faces_flipped']} holes filled {r['holes_filled']} too long {r['holes_too_long']} "
            f"edges on open chains {r['edges_on_open_chains']} verts added {r['verts_added']} faces added {r['faces_added']}")
