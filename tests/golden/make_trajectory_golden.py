"""Writes tests/golden/trajectory_poses.npz: the REFERENCE's get_camera_trajectory_pose and compute_pose_matrix
(R/utils/camera_utils.py:121-148, R/ = dgmesh/) executed from their source text.

Run from the repository root:  python tests/golden/make_trajectory_golden.py   (needs the reference tree at REF below).

Two orbits, each stored as the (n, 4, 4) float64 OpenGL camera-to-world matrices the reference returns, with their arguments:
  a: radius 4, elevation 1, 8 frames, look_at (0, 0, 0)          -- render_trajectory.py's defaults, fewer frames;
  b: radius 2.5, elevation -0.5, 5 frames, look_at (0.1, 0, 0.2)."""
import ast
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/dgmesh"
CASES = {"a": dict(radius=4.0, elevation=1.0, total_frames=8, look_at=[0.0, 0.0, 0.0]),
         "b": dict(radius=2.5, elevation=-0.5, total_frames=5, look_at=[0.1, 0.0, 0.2])}


def function(path, name, ns):
    """Compile one function of the file at `path` from its source text, wherever in the module it is defined."""
    node = next(n for n in ast.walk(ast.parse(open(path).read())) if isinstance(n, ast.FunctionDef) and n.name == name)
    exec(compile(ast.Module([node], []), os.path.basename(path), "exec"), ns)
    return ns[name]


def main():
    ns = {"np": np}
    path = os.path.join(REF, "utils/camera_utils.py")
    function(path, "compute_pose_matrix", ns)
    poses_of = function(path, "get_camera_trajectory_pose", ns)
    rec = {}
    for key, c in CASES.items():
        poses = np.stack(poses_of(c["radius"], c["elevation"], c["total_frames"], look_at=list(c["look_at"]))).astype(np.float64)
        assert poses.shape == (c["total_frames"], 4, 4)
        rec[key + "/poses"] = poses
        rec[key + "/radius"], rec[key + "/elevation"] = np.float64(c["radius"]), np.float64(c["elevation"])
        rec[key + "/total_frames"], rec[key + "/look_at"] = np.int64(c["total_frames"]), np.array(c["look_at"], np.float64)
        print(key, c, "\n", poses[1])
    out = os.path.join(HERE, "trajectory_poses.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
