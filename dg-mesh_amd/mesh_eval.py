"""Mesh evaluation on the device: the Chamfer distance and the approximate earth mover's distance of exported dynamic meshes
against ground truth -- mesh_evaluation.py of the reference (R/mesh_evaluation.py, R/ = dgmesh/) with emd_cd
(R/metrics/evaluation_metrics.py:18-62) and its CUDA extension (R/metrics/pytorch_structural_losses/src/approxmatch.cu).

  * EMD: csrc/emd.hip (dgm_emd_approx): the reference's iteration, nine levels, spread over the chip, without the n x m `match`
    matrix.  emd_approx mirrors match_cost.
  * nearest distances: anchor.nearest with max_d2 = +inf, the exact, bit-reproducible knn_points(K=1); no second search kernel.
  * surface samples: normal_init.sample_surface, trimesh.sample.sample_surface on the device, with this project's sampling stream
    (torch.rand of a device generator) -- the reference draws from numpy's global stream, unseeded.
  * predicted meshes: ply_io.read_mesh_ply; ground truth: read_mesh_obj below.

chamferdist, the external emd module, trimesh and wis3d are neither vendored nor dependencies.  chamfer_distance is this project's
reading of chamferdist.ChamferDistance()(source, target, point_reduction="mean") with one batch element: the mean over the source
points of the SQUARED distance to the nearest target point.  wis3d (the reference's debug viewer) is not built.
No CPU fallback: every function that computes raises on host tensors.

  python -m dgmesh_amd.mesh_eval --path <scene folder> --eval_type dgmesh
follows the reference's folders: <path>/gt/*.obj against <path>/DGMesh/dynamic_mesh/*.ply, results in
<path>/DGMesh/results/<scene>_<time>/eval_results.txt."""
import argparse
import ctypes
import glob
import json
import os
import time

import numpy as np
import torch

from . import _lib

# R/utils/pose_utils.py:102-139: the matrix applied to the predicted points of each eval_model_type (rotate_mtx_dgmesh is stated
# there as the inverse of [[1, 0, 0], [0, 0, -1], [0, 1, 0]], which is its transpose).  All are orthonormal; the dnerf one has determinant
# -1 (it mirrors) in the reference and is restated as it is.
_Y_TO_Z = ((1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, -1.0, 0.0))
ROTATIONS = {
    "dgmesh": _Y_TO_Z,
    "hexplane": _Y_TO_Z,
    "tineuvox": _Y_TO_Z,
    "dnerf": ((0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (-1.0, 0.0, 0.0)),
    "kplane": _Y_TO_Z,
    "deformable_gaussian": _Y_TO_Z,
}
# R/mesh_evaluation.py:205-214 (deformable_gaussian has no folder there; evaluation() takes any pair of folders)
FOLDERS = {"dgmesh": "DGMesh", "hexplane": "HexPlane", "tineuvox": "TiNeuVox", "dnerf": "D-NeRF", "kplane": "K-Plane"}
# the camera-origin shift of R/mesh_evaluation.py:46-51: inverse(rotate_mtx_dgmesh) @ (blender2opencv @ (origin, 1))[:3], whatever
# the eval_model_type; blender2opencv = diag(1, -1, -1, 1) (R/nvdiffrast_utils/util.py:470-473)
_CAM_ORIGIN_MATRIX = np.array(((1.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0))) @ np.diag((1.0, -1.0, -1.0))


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _cloud(name, t, dims):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"mesh_eval.{name} needs CUDA/HIP tensors (dg-mesh_amd has no CPU path)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"mesh_eval.{name} needs float32 tensors, got {t.dtype}")
    if t.dim() != dims or t.shape[-1] != 3 or min(t.shape) < 1:
        raise ValueError(f"mesh_eval.{name}: expected a non-empty {'(B, N, 3)' if dims == 3 else '(N, 3)'} tensor, got {tuple(t.shape)}")
    return t.detach().contiguous()


def emd_tiles():
    """The launch constants of csrc/emd.hip: {"rows", "cols", "target_blocks", "levels"} (dgm_emd_tile)."""
    L = _lib.lib()
    return {k: int(L.dgm_emd_tile(i)) for i, k in enumerate(("rows", "cols", "target_blocks", "levels"))}


def emd_parts(rows, cols):
    """Column parts of a sweep with `rows` rows against `cols` columns (dgm_emd_parts)."""
    return int(_lib.lib().dgm_emd_parts(int(rows), int(cols)))


def emd_approx(sample, ref, return_residual=False, *, scratch=None):
    """match_cost (R/metrics/pytorch_structural_losses/match_cost.py) without its gradient: sample (B, N, 3), ref (B, M, 3) fp32
    device tensors -> cost (B,) fp32, not divided by N.  return_residual: also (B, 2) = (sum remainL, sum remainR) after the last
    level, the mass that was not transported.  `scratch`: a float32 device tensor of at least dgm_emd_scratch_floats(B, N, M)
    elements to use instead of a fresh one (its contents do not matter).  Bit-reproducible; nothing is read back."""
    a, b = _cloud("emd_approx", sample, 3), _cloud("emd_approx", ref, 3)
    if a.shape[0] != b.shape[0] or a.device != b.device:
        raise ValueError(f"mesh_eval.emd_approx: batch sizes / devices differ: {tuple(a.shape)} on {a.device}, {tuple(b.shape)} on {b.device}")
    B, N, M = a.shape[0], a.shape[1], b.shape[1]
    L = _lib.lib()
    need = int(L.dgm_emd_scratch_floats(B, N, M))
    if need == 0:
        raise ValueError(f"mesh_eval.emd_approx: sizes out of range: B = {B}, N = {N}, M = {M}")
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.float32, device=a.device)
    elif not (scratch.is_cuda and scratch.dtype == torch.float32 and scratch.is_contiguous() and scratch.numel() >= need
              and scratch.device == a.device):
        raise ValueError(f"mesh_eval.emd_approx: scratch must be a contiguous float32 tensor of >= {need} elements on {a.device}")
    cost = torch.empty(B, dtype=torch.float32, device=a.device)
    residual = torch.empty((B, 2), dtype=torch.float32, device=a.device) if return_residual else None
    with _lib.device_guard(a.device):
        _lib.check(L.dgm_emd_approx(B, N, M, _vp(a), _vp(b), _vp(scratch), _vp(cost), _vp(residual) if return_residual else None,
                                    _lib.stream_ptr()))
    return (cost, residual) if return_residual else cost


def _mean_nearest_d2(a, b):
    """Mean over the rows of a of the squared distance to the nearest row of b: the fp32 distances of anchor.nearest (max_d2 = +inf:
    knn_points(K=1)), averaged in fp64."""
    from . import anchor as _A
    return _A.nearest(a, b)[1].double().mean()


def emd_cd(sample_pcs, ref_pcs, reduced=True):
    """emd_cd of R/metrics/evaluation_metrics.py:42-62 (its batch_size chunking changes nothing and is not reproduced): (B, N, 3)
    against (B, N, 3) -> {"CD": mean(dl) + mean(dr) of the squared nearest distances (float64), "EMD": match cost / N (float32)}, each
    the mean over the batch, or (B,) tensors with reduced=False.  N == M is required, as emd_approx_cuda asserts."""
    a, b = _cloud("emd_cd", sample_pcs, 3), _cloud("emd_cd", ref_pcs, 3)
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"mesh_eval.emd_cd: REF:{b.shape[0]} SMP:{a.shape[0]}")
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"mesh_eval.emd_cd: the EMD needs clouds of one size, got {a.shape[1]} and {b.shape[1]} points")
    cd = torch.stack([_mean_nearest_d2(a[i], b[i]) + _mean_nearest_d2(b[i], a[i]) for i in range(a.shape[0])])
    emd = emd_approx(a, b) / float(a.shape[1])
    if reduced:
        cd, emd = cd.mean(), emd.mean()
    return {"CD": cd, "EMD": emd}


def chamfer_distance(a, b):
    """The evaluation's symmetric Chamfer distance (R/mesh_evaluation.py:67-70) of a (Na, 3) and b (Nb, 3):
    (mean over a of min d2 + mean over b of min d2) / 2 with SQUARED distances -- this project's reading of
    (ChamferDistance()(a, b, point_reduction="mean") + ChamferDistance()(b, a, point_reduction="mean")) / 2; chamferdist itself
    is not available to compare against.  A float64 device scalar."""
    a, b = _cloud("chamfer_distance", a, 2), _cloud("chamfer_distance", b, 2)
    return (_mean_nearest_d2(a, b) + _mean_nearest_d2(b, a)) / 2


def read_mesh_obj(path):
    """-> verts (V, 3) float32, faces (F, 3) int32 of a Wavefront OBJ.  `v x y z [w]` and `f` lines are read; face entries may be
    `a`, `a/b`, `a//c` or `a/b/c` (only a, the vertex index, is used), 1-based or negative (relative to the vertices read so far);
    a polygon is fan-triangulated around its first vertex.  Every other line is ignored.  A malformed or out-of-range entry raises
    ValueError with the line number."""
    verts, faces = [], []
    with open(path, "r", errors="replace") as fh:
        for no, line in enumerate(fh, 1):
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                try:
                    verts.append((float(tok[1]), float(tok[2]), float(tok[3])))
                except (IndexError, ValueError):
                    raise ValueError(f"{path}:{no}: malformed vertex line {line.strip()!r}") from None
            elif tok[0] == "f":
                idx = []
                for entry in tok[1:]:
                    try:
                        i = int(entry.split("/")[0])
                    except ValueError:
                        raise ValueError(f"{path}:{no}: malformed face entry {entry!r}") from None
                    j = i - 1 if i > 0 else len(verts) + i
                    if i == 0 or not 0 <= j < len(verts):
                        raise ValueError(f"{path}:{no}: face index {i} out of range ({len(verts)} vertices so far)")
                    idx.append(j)
                if len(idx) < 3:
                    raise ValueError(f"{path}:{no}: a face needs at least three vertices")
                faces.extend((idx[0], idx[k], idx[k + 1]) for k in range(1, len(idx) - 1))
    return np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)


def eval_distance(gt_verts, gt_faces, eval_verts, eval_faces, rotate=None, cam_origin=None, emd_sample=8192, generator=None):
    """eval_distance of R/mesh_evaluation.py:31-95 on device tensors: (chamfer, emd), two device scalars, nothing read back.
    The Chamfer distance is taken on the VERTICES, the EMD on `emd_sample` surface samples of each mesh (sample_surface, the
    ground truth first, then the prediction, both from `generator`).  rotate: a 3 x 3 matrix applied to the predicted points
    (a ROTATIONS entry); cam_origin: the dataset's Blender-space camera origin, whose image under the reference's fixed matrix
    is subtracted from the ground-truth points.  A mesh without area gives a NaN EMD (no read-back checks it)."""
    from . import normal_init as _N
    gv, ev = _cloud("eval_distance", gt_verts, 2), _cloud("eval_distance", eval_verts, 2)
    dev = gv.device
    shift = None
    if cam_origin is not None:
        shift = torch.tensor(_CAM_ORIGIN_MATRIX @ np.asarray(cam_origin, np.float64).reshape(3), dtype=torch.float32, device=dev)
        gv = gv - shift
    rot = None if rotate is None else torch.as_tensor(np.asarray(rotate, np.float32), device=dev)
    if rot is not None:
        ev = (rot @ ev.T).T.contiguous()
    chamfer = chamfer_distance(gv, ev)
    gs, _ = _N.sample_surface(gt_verts, gt_faces, emd_sample, generator=generator, check=False)
    es, _ = _N.sample_surface(eval_verts, eval_faces, emd_sample, generator=generator, check=False)
    if shift is not None:
        gs = gs - shift
    if rot is not None:
        es = (rot @ es.T).T.contiguous()
    return chamfer, emd_cd(gs[None], es[None])["EMD"]


def _mesh_pairs(who, gt_mesh_path, eval_mesh_path, eval_model_type):
    """What evaluation and evaluation_iou share before the device is touched: -> ([(gt file, predicted file)], camera_origin or
    None, the current device); the ValueErrors are those evaluation documents."""
    if eval_model_type not in ROTATIONS:
        raise ValueError(f"mesh_eval.{who}: eval_model_type {eval_model_type!r} not supported (one of {sorted(ROTATIONS)})")
    gt_list = sorted(glob.glob(os.path.join(gt_mesh_path, "*.obj")))
    eval_list = sorted(glob.glob(os.path.join(eval_mesh_path, "*.ply")))
    if len(gt_list) != len(eval_list):
        raise ValueError(f"mesh_eval.{who}: {len(gt_list)} ground-truth meshes in {gt_mesh_path} but {len(eval_list)} predicted "
                         f"meshes in {eval_mesh_path}")
    if not gt_list:
        raise ValueError(f"mesh_eval.{who}: no *.obj in {gt_mesh_path}")
    cam_origin = None
    json_path = os.path.join(os.path.dirname(os.path.abspath(gt_mesh_path)), "transforms_train.json")
    if os.path.exists(json_path):
        with open(json_path, "r") as fh:
            cam_origin = json.load(fh).get("camera_origin")
    return list(zip(gt_list, eval_list)), cam_origin, torch.device("cuda", torch.cuda.current_device())


def _load_pair(who, gt_file, eval_file, clean, dev):
    """-> (gt verts, gt faces, predicted verts, predicted faces) on the device, the prediction cleaned when `clean` says so."""
    from . import mesh_clean
    from .ply_io import read_mesh_ply
    gv, gf = read_mesh_obj(gt_file)
    ev, ef = read_mesh_ply(eval_file)
    to = lambda a: torch.from_numpy(a).to(dev)
    ev, ef = to(ev), to(ef)
    if clean is not None:
        ev, ef = mesh_clean.apply(clean, ev, ef)
        if ev.shape[0] == 0:
            raise ValueError(f"mesh_eval.{who}: nothing of {eval_file} is left after cleaning ({clean.describe()})")
    return to(gv), to(gf), ev, ef


def evaluation(gt_mesh_path, eval_mesh_path, eval_model_type, emd_sample=8192, seed=0, clean=None):
    """evaluation of R/mesh_evaluation.py:98-178: the sorted *.obj of gt_mesh_path against the sorted *.ply of eval_mesh_path,
    -> (avg_cd, cd_list, avg_emd, emd_list) as Python floats.  camera_origin is read from ../transforms_train.json of the ground
    truth when that file exists and has the key.  Runs on the current device; the samples come from one generator seeded with `seed`.  The results stay
    on the device until one read-back after the last mesh.  ValueError: an unknown eval_model_type, no meshes, or folders of
    different sizes (raised before the device is touched).  clean: None, or a mesh_clean.CleanSpec (or a dict of its fields): each
    PREDICTED mesh loses the components that fail it before it is scored (mesh_clean.clean_mesh, which reads the output sizes back
    per mesh); a prediction of which nothing is left raises ValueError."""
    from . import mesh_clean
    clean = mesh_clean.as_spec(clean)
    pairs, cam_origin, dev = _mesh_pairs("evaluation", gt_mesh_path, eval_mesh_path, eval_model_type)
    generator = torch.Generator(device=dev).manual_seed(int(seed))
    table = torch.empty((len(pairs), 2), dtype=torch.float64, device=dev)
    for i, (gt_file, eval_file) in enumerate(pairs):
        gv, gf, ev, ef = _load_pair("evaluation", gt_file, eval_file, clean, dev)
        cd, emd = eval_distance(gv, gf, ev, ef, rotate=ROTATIONS[eval_model_type], cam_origin=cam_origin,
                                emd_sample=emd_sample, generator=generator)
        table[i, 0], table[i, 1] = cd, emd
    host = table.cpu().numpy()  # the one read-back
    cd_list, emd_list = [float(v) for v in host[:, 0]], [float(v) for v in host[:, 1]]
    return float(np.mean(cd_list)), cd_list, float(np.mean(emd_list)), emd_list


def evaluation_iou(gt_mesh_path, eval_mesh_path, eval_model_type, n_points=100000, seed=0, clean=None):
    """The volumetric IoU (mesh_inside.volume_iou, absolute=True: either winding counts as inside) of every predicted mesh against
    its ground truth, -> (avg_iou, iou_list) as Python floats.  The folders, the rotation of the predicted vertices, the
    camera_origin shift of the ground truth, `clean` and the ValueErrors are evaluation()'s; the n_points samples of every pair come
    from one generator seeded with `seed`.  Cost: n_points x (faces of both meshes) pairs per item.  The results stay on the device
    until one read-back after the last mesh.  A pair neither of whose meshes encloses a sample gives NaN."""
    from . import mesh_clean, mesh_inside
    clean = mesh_clean.as_spec(clean)
    pairs, cam_origin, dev = _mesh_pairs("evaluation_iou", gt_mesh_path, eval_mesh_path, eval_model_type)
    generator = torch.Generator(device=dev).manual_seed(int(seed))
    rot = torch.as_tensor(np.asarray(ROTATIONS[eval_model_type], np.float32), device=dev)
    table = torch.empty(len(pairs), dtype=torch.float64, device=dev)
    for i, (gt_file, eval_file) in enumerate(pairs):
        gv, gf, ev, ef = _load_pair("evaluation_iou", gt_file, eval_file, clean, dev)
        if cam_origin is not None:
            gv = gv - torch.tensor(_CAM_ORIGIN_MATRIX @ np.asarray(cam_origin, np.float64).reshape(3), dtype=torch.float32, device=dev)
        ev = (rot @ ev.T).T.contiguous()
        table[i] = mesh_inside.volume_iou(gv, gf, ev, ef, n_points=n_points, generator=generator, absolute=True)["iou"]
    iou_list = [float(v) for v in table.cpu().numpy()]  # the one read-back
    return float(np.mean(iou_list)), iou_list


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m dgmesh_amd.mesh_eval", description=__doc__.split("\n\n")[0])
    ap.add_argument("--path", required=True, help="scene folder holding gt/ and the method's folder")
    ap.add_argument("--eval_type", required=True, choices=sorted(ROTATIONS))
    ap.add_argument("--emd_sample", type=int, default=8192)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--iou", type=int, nargs="?", const=100000, default=None, metavar="N",
                    help="also score the volumetric IoU of every pair, on N uniform samples of the union bounding box (default 100000)")
    ap.add_argument("--largest_component", action="store_true", help="score only the largest component of each predicted mesh")
    ap.add_argument("--min_component_faces", type=int, default=0, metavar="N", help="drop predicted components with fewer faces")
    ap.add_argument("--min_component_diameter", type=float, default=0.0, metavar="FRAC",
                    help="drop predicted components whose box diagonal is below FRAC of the whole mesh's")
    return ap


def clean_from_args(args):
    """The mesh_clean.CleanSpec of the three component flags, or None when none is set."""
    from .mesh_clean import CleanSpec
    spec = CleanSpec(largest=args.largest_component, min_faces=args.min_component_faces, min_diameter_frac=args.min_component_diameter)
    if spec.min_faces < 0 or not spec.min_diameter_frac >= 0.0:
        raise ValueError("--min_component_faces and --min_component_diameter must be >= 0")
    return spec if spec.any() else None


def main(argv=None):
    """The command line of R/mesh_evaluation.py:181-248; returns the path of the eval_results.txt it wrote."""
    ap = build_parser()
    args = ap.parse_args(argv)
    clean = clean_from_args(args)
    folder = FOLDERS.get(args.eval_type)
    if folder is None:
        ap.error(f"--eval_type {args.eval_type} has no folder in the reference's command line: call evaluation() with the two folders")
    gt_path = os.path.join(args.path, "gt")
    pred_root = os.path.join(args.path, folder)
    if not os.path.exists(pred_root):
        raise FileNotFoundError(f"Predicted results path not found: {pred_root}")
    pred_path = os.path.join(pred_root, "dynamic_mesh")
    item_name = os.path.basename(os.path.dirname(os.path.abspath(gt_path)))
    log_folder = os.path.join(pred_root, "results", item_name + time.strftime("_%Y-%m-%d_%H-%M-%S", time.localtime()))
    print(f"GT path: {gt_path} \nPred path: {pred_path} \nLog folder: {log_folder}")
    avg_cd, cd_list, avg_emd, emd_list = evaluation(gt_path, pred_path, args.eval_type, emd_sample=args.emd_sample, seed=args.seed,
                                                    clean=clean)
    for i, (cd, emd) in enumerate(zip(cd_list, emd_list)):
        print(f"Item {i}: CD {cd:.10f}, EMD {emd:.4f}")
    print(f"Average Chamfer distance: {avg_cd:.4f}")
    print(f"Average EMD: {avg_emd:.4f}")
    if args.iou is not None:
        avg_iou, iou_list = evaluation_iou(gt_path, pred_path, args.eval_type, n_points=args.iou, seed=args.seed, clean=clean)
        for i, iou in enumerate(iou_list):
            print(f"Item {i}: IoU {iou:.6f}")
        print(f"Average volume IoU: {avg_iou:.6f}")
    os.makedirs(log_folder, exist_ok=True)
    out = os.path.join(log_folder, "eval_results.txt")
    with open(out, "w") as fh:
        fh.write(f"GT source: {gt_path}\n")
        fh.write(f"Pred source: {pred_path}\n")
        fh.write(f"Average Chamfer distance: {avg_cd:.10f}\n")
        fh.write(f"Average EMD: {avg_emd:.4f}\n")
        if args.iou is not None:
            for i, iou in enumerate(iou_list):
                fh.write(f"Item {i}: IoU {iou:.6f}\n")
            fh.write(f"Average volume IoU: {avg_iou:.6f}\n")
        if clean is not None:
            fh.write(f"Predicted meshes cleaned: {clean.describe()}\n")
    return out


if __name__ == "__main__":
    main()
