"""CPU checks of entering the mesh phase: the float64 restatement (tests/_ninit_ref.py) reproduces the reference's own
update_scale_center / normal_initialization (tests/golden/normal_init_small.npz, written by make_normal_init_golden.py from the
reference's source text); the library exports the dgm_ninit_* entry points and validates their arguments without a GPU; the
point-cloud PLY pair round-trips; MeshPhase validates normal_init."""
import ctypes
import os
import re

import numpy as np
import pytest

import _mc_ref
import _ninit_ref as NR
from _anchor_ref import PolyField
from conftest import ROOT, pkg

GOLD = os.path.join(os.path.dirname(__file__), "golden", "normal_init_small.npz")


def gold_deform(gold):
    return PolyField(*[gold[f"deform/{i}"] for i in range(4)])


def poly_d_xyz(gold):
    """PolyField's d_xyz in float64 from the golden's constants: (xyz (N, 3), t) -> (N, 3)."""
    W = gold["deform/0"].astype(np.float64)
    return lambda x, t: ((x[:, 0:1] * W[0] + x[:, 1:2] * W[1]) + x[:, 2:3] * W[2]) + t * W[3]


def test_fixture_holds_arrays_only():
    gold = np.load(GOLD, allow_pickle=False)
    for k in gold.files:
        assert gold[k].dtype.kind in "fiu", k
    assert os.path.getsize(GOLD) < 1 << 20
    assert 0.0 <= float(gold["flip_share_ref"]) <= 0.02


def test_scale_center_restatement_matches_the_reference():
    gold = np.load(GOLD)
    table = NR.bbox_table(gold["xyz"], poly_d_xyz(gold), 50)
    center, scale = NR.scale_center(table, float(gold["gaussian_ratio"]))
    assert np.abs(center - gold["center"]).max() <= 1e-6 * np.abs(gold["center"]).max()
    assert abs(scale - float(gold["scale"][0])) <= 1e-6 * float(gold["scale"][0])
    assert float(gold["threshold"][0]) == pytest.approx(0.05, rel=1e-6)


def test_sampling_restatement_matches_the_reference():
    gold = np.load(GOLD)
    pts, fidx, margin = NR.sample_surface(gold["verts"], gold["faces"], gold["u"])
    assert np.array_equal(fidx, gold["face_index"])
    box = float(np.ptp(gold["verts"], axis=0).max())
    assert np.abs(pts - gold["samples"]).max() <= 1e-6 * box
    # the committed seed: no draw of the golden lies within 2^-40 * total of a cumulative boundary (the GPU test's exclusion rule
    # excludes nothing here), for float64 areas and for the device's fp32 areas alike, and both pick the same faces
    total = NR.face_areas(gold["verts"], gold["faces"]).sum()
    assert margin.min() > 2.0 ** -40 * total
    pts32, fidx32, margin32 = NR.sample_surface(gold["verts"], gold["faces"], gold["u"], areas=NR.face_areas32(gold["verts"], gold["faces"]))
    assert np.array_equal(fidx32, fidx) and margin32.min() > 2.0 ** -40 * total


def test_chain_restatement_matches_the_reference():
    gold = np.load(GOLD)
    d_xyz = gold_deform(gold).step(__import__("torch").tensor(gold["xyz"]), float(gold["t0"]))[0].numpy()
    xyz_d = gold["xyz"] + d_xyz
    out = NR.chain_from_occ(gold["occ"], xyz_d, gold["u"], lambda grid, iso: _mc_ref.marching_cubes(grid, iso=iso)[:2])
    assert (len(out["verts"]), len(out["faces"])) == (int(gold["V"]), int(gold["F"]))
    assert np.array_equal(out["faces"], gold["faces"]) and np.array_equal(out["verts"], gold["verts"])
    assert np.array_equal(out["face_index"], gold["face_index"])
    assert np.array_equal(out["nearest"], gold["nearest"])
    box = float(np.ptp(gold["verts"], axis=0).max())
    assert np.abs(out["samples"] - gold["samples"]).max() <= 1e-6 * box
    assert np.abs(out["normals"] - gold["normals"]).max() <= 1e-6
    assert out["gap"].min() > 5e-8


def test_library_exports_the_ninit_entry_points():
    L = pkg("_lib")
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "dgmesh_hip.h")).read()
    declared = {n for n in re.findall(r"\b(dgm_[a-z0-9_]+)\s*\(", header) if n.startswith("dgm_ninit_")}
    assert declared == {"dgm_ninit_bbox_scratch_bytes", "dgm_ninit_bbox", "dgm_ninit_face_areas", "dgm_ninit_scan_scratch_bytes",
                        "dgm_ninit_area_scan", "dgm_ninit_sample"}
    for name in declared:
        assert name in L.SYMBOLS and hasattr(lib, name), name
    assert lib.dgm_abi_version() == 5
    # argument validation happens before any HIP call
    assert lib.dgm_ninit_bbox(0, None, None, None, None, None) != 0 and b"ninit_bbox" in lib.dgm_last_error()
    assert lib.dgm_ninit_bbox(5, None, None, None, None, None) != 0
    assert lib.dgm_ninit_face_areas(-1, 0, None, None, None, None) != 0
    assert lib.dgm_ninit_face_areas(3, 0, None, None, None, None) == 0   # F == 0 is a no-op
    assert lib.dgm_ninit_area_scan(0, None, None, None, None) == 0 and lib.dgm_ninit_area_scan(4, None, None, None, None) != 0
    assert lib.dgm_ninit_sample(3, 0, 4, None, None, None, None, None, None, None) != 0
    assert lib.dgm_ninit_bbox_scratch_bytes() >= 256 * 6 * 4
    assert lib.dgm_ninit_scan_scratch_bytes(4_700_000) >= 2 * 8 * (4_700_000 // 4096)


def test_cpu_tensors_are_refused():
    import torch
    N = pkg("normal_init")
    with pytest.raises(RuntimeError, match="no CPU path"):
        N.bbox(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        N.sample_surface(torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32), 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        N.face_areas(torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32))


def test_pointcloud_ply_round_trip(tmp_path):
    io = pkg("ply_io")
    rng = np.random.RandomState(0)
    p, n = rng.randn(257, 3).astype(np.float32), rng.randn(257, 3).astype(np.float32)
    path = str(tmp_path / "sub" / "pointcloud_init.ply")
    io.write_pointcloud_ply(path, p, n)
    p2, n2 = io.read_pointcloud_ply(path)
    assert np.array_equal(p, p2) and np.array_equal(n, n2)
    head = open(path, "rb").read(200).decode("ascii", "ignore")
    assert "element vertex 257" in head and "property float nx" in head
    import torch
    io.write_pointcloud_ply(path, torch.tensor(p), torch.tensor(n))
    assert np.array_equal(io.read_pointcloud_ply(path)[1], n)
    with pytest.raises(ValueError):
        io.write_pointcloud_ply(path, p, n[:5])


def test_mesh_phase_validates_normal_init():
    T = pkg("trainer")
    assert T.MeshPhase(None, None, None, mesh_source="diffmc", device="cpu").normal_init is False
    with pytest.raises(ValueError):
        T.MeshPhase(None, None, None, mesh_source="diffmc", normal_init=True, device="cpu")            # no DPSR module
    with pytest.raises(ValueError):
        T.MeshPhase(None, None, None, dpsr=object(), mesh_source="probes", normal_init=True, device="cpu")
    ms = T.MeshPhase(None, None, None, dpsr=object(), mesh_source="diffmc", normal_init=True, gaussian_ratio=1.2, real=True, device="cpu")
    assert ms.normal_init and ms.gaussian_ratio == 1.2 and ms.real
    assert pkg("scene").OptimizationParams().init_density_threshold == 0.05
