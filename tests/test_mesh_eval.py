"""The mesh evaluation (dg-mesh_amd/mesh_eval.py) on the GPU: the Chamfer distances against an fp64 brute force, eval_distance on
two icospheres (vertices for the Chamfer distance, surface samples for the EMD, the rotation on the predicted side, the
camera-origin shift on the ground-truth side) and evaluation() / the command line on a folder of three OBJ / PLY pairs."""
import json
import os

import numpy as np
import pytest
import torch

import _emd_ref as ER
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ME():
    return pkg("mesh_eval")


def dt(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def icosphere(radius=1.0, subdivisions=2):
    """-> verts (V, 3) float32 on the sphere, faces (F, 3) int32, outward winding (162 vertices, 320 faces at 2 subdivisions)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius).astype(np.float32), np.asarray(f, np.int32)


def brute_chamfer(a, b):
    dl, dr = ER.chamfer_sides(a, b)
    return dl.mean(), dr.mean()


@pytest.mark.parametrize("na, nb", [(1, 1), (257, 1000), (1000, 257)])
def test_chamfer_against_fp64_brute_force(na, nb):
    rng = np.random.default_rng(na * 31 + nb)
    a = rng.standard_normal((na, 3)).astype(np.float32)
    b = (rng.standard_normal((nb, 3)) * 1.1 + 0.1).astype(np.float32)
    if na > 1:
        b[nb // 2] = a[na // 3]  # one exact duplicate point: a distance of exactly 0
    dl, dr = brute_chamfer(a, b)
    want = (dl + dr) / 2
    got = float(ME().chamfer_distance(dt(a), dt(b)))
    print(f"CD_FIG chamfer_distance na={na} nb={nb} want={want:.12g} got={got:.12g} rel={abs(got - want) / want:.3e}")
    assert abs(got - want) <= 1e-6 * want
    # emd_cd needs clouds of one size: its CD is checked on the clouds cut to the smaller size, with the duplicate point put back
    k = min(na, nb)
    x, y = a[:k].copy(), b[:k].copy()
    if k > 1:
        y[k // 2] = x[k // 3]
    for x, y in [(x, y)]:
        dl, dr = brute_chamfer(x, y)
        out = ME().emd_cd(dt(x)[None], dt(y)[None])
        got = float(out["CD"])
        print(f"CD_FIG emd_cd n={len(x)} want={dl + dr:.12g} got={got:.12g} rel={abs(got - (dl + dr)) / (dl + dr):.3e}")
        assert abs(got - (dl + dr)) <= 1e-6 * (dl + dr)
        assert out["EMD"].shape == () and float(out["EMD"]) > 0


def test_emd_cd_batch_and_reduction():
    a = np.stack([ER.sphere_cloud(300, 1.0, seed=i) for i in range(2)])
    b = np.stack([ER.sphere_cloud(300, 1.1, seed=5 + i) for i in range(2)])
    full = ME().emd_cd(dt(a), dt(b), reduced=False)
    red = ME().emd_cd(dt(a), dt(b))
    assert full["CD"].shape == (2,) and full["EMD"].shape == (2,)
    for i in range(2):
        dl, dr = brute_chamfer(a[i], b[i])
        assert abs(float(full["CD"][i]) - (dl + dr)) <= 1e-6 * (dl + dr)
    cost = ME().emd_approx(dt(a), dt(b))
    assert torch.equal(full["EMD"], cost / 300.0)
    assert float(red["CD"]) == pytest.approx(float(full["CD"].mean()), rel=1e-12)
    assert float(red["EMD"]) == pytest.approx(float(full["EMD"].mean()), rel=1e-6)


def test_eval_distance_on_icospheres():
    N = pkg("normal_init")
    gv, gf = icosphere(1.0)
    ev, ef = icosphere(1.05)
    assert gv.shape == (162, 3) and gf.shape == (320, 3)
    tg, tgf, te, tef = dt(gv), dt(gf, torch.int32), dt(ev), dt(ef, torch.int32)
    gen = torch.Generator(device=DEV).manual_seed(11)
    cd, emd = ME().eval_distance(tg, tgf, te, tef, emd_sample=1024, generator=gen)
    dl, dr = brute_chamfer(gv, ev)
    want = (dl + dr) / 2
    print(f"CD_FIG eval_distance want={want:.12g} got={float(cd):.12g}")
    assert abs(float(cd) - want) <= 1e-6 * want
    assert want == pytest.approx(0.05 ** 2, rel=1e-4)  # same directions, radii 0.05 apart
    # the EMD is the match cost of the surface samples, drawn ground truth first, over their number
    gen = torch.Generator(device=DEV).manual_seed(11)
    gs, _ = N.sample_surface(tg, tgf, 1024, generator=gen)
    es, _ = N.sample_surface(te, tef, 1024, generator=gen)
    cost = ME().emd_approx(gs[None], es[None])
    assert torch.equal(emd.reshape(1), cost / 1024.0)
    assert 0.04 < float(emd) < 0.5  # at least the gap between the two surfaces


def test_eval_distance_rotates_the_prediction_and_shifts_the_ground_truth():
    M = ME()
    sv, sf = icosphere(1.0)
    gv = (sv * np.array([1.0, 0.5, 0.25], np.float32) + np.array([0.3, 0.1, -0.2], np.float32)).astype(np.float32)  # no symmetry left
    tgf = dt(sf, torch.int32)
    for name in ("dgmesh", "dnerf"):
        R = np.asarray(M.ROTATIONS[name], np.float32)
        ev = gv @ R  # rows R^T g: the preset maps them back onto the ground truth (R R^T = 1, exact for these matrices)
        gen = torch.Generator(device=DEV).manual_seed(3)
        cd_rot, emd_rot = M.eval_distance(dt(gv), tgf, dt(ev), tgf, rotate=M.ROTATIONS[name], emd_sample=512, generator=gen)
        gen = torch.Generator(device=DEV).manual_seed(3)
        cd_raw, emd_raw = M.eval_distance(dt(gv), tgf, dt(ev), tgf, emd_sample=512, generator=gen)
        assert float(cd_rot) == 0.0
        dl, dr = brute_chamfer(gv, ev)
        assert abs(float(cd_raw) - (dl + dr) / 2) <= 1e-6 * (dl + dr) / 2 and float(cd_raw) > 1e-3
        assert float(emd_rot) < float(emd_raw)
        # the rotation belongs to the predicted side: rotating the ground truth instead does not give 0
        gen = torch.Generator(device=DEV).manual_seed(3)
        cd_swapped, _ = M.eval_distance(dt(ev), tgf, dt(gv), tgf, rotate=M.ROTATIONS[name], emd_sample=512, generator=gen)
        assert float(cd_swapped) > 1e-3
    # camera origin: subtracted from the ground truth after the reference's fixed matrix (x, y, z) -> (x, z, -y)
    origin = np.array([0.25, -0.5, 0.75])
    shift = np.array([origin[0], origin[2], -origin[1]], np.float32)
    ev = (gv - shift).astype(np.float32)
    gen = torch.Generator(device=DEV).manual_seed(3)
    cd_shift, emd_shift = M.eval_distance(dt(gv), tgf, dt(ev), tgf, cam_origin=origin, emd_sample=512, generator=gen)
    assert float(cd_shift) <= 1e-12
    gen = torch.Generator(device=DEV).manual_seed(3)
    cd_none, _ = M.eval_distance(dt(gv), tgf, dt(ev), tgf, emd_sample=512, generator=gen)
    assert float(cd_none) > 0.1


def _write_obj(path, v, f):
    with open(path, "w") as fh:
        fh.write("# test mesh\n")
        for p in v:
            fh.write(f"v {p[0]:.9g} {p[1]:.9g} {p[2]:.9g}\n")
        for t in f:
            fh.write(f"f {t[0] + 1}//{t[0] + 1} {t[1] + 1}//{t[1] + 1} {t[2] + 1}//{t[2] + 1}\n")


def test_evaluation_end_to_end_and_cli(tmp_path):
    M = ME()
    P = pkg("ply_io")
    scene = tmp_path / "scene"
    gt, pred = scene / "gt", scene / "DGMesh" / "dynamic_mesh"
    gt.mkdir(parents=True)
    pred.mkdir(parents=True)
    R = np.asarray(M.ROTATIONS["dgmesh"], np.float32)
    origin = [0.1, -0.2, 0.3]
    shift = np.array([origin[0], origin[2], -origin[1]], np.float32)
    meshes = []
    for i, radius in enumerate((0.5, 0.8, 1.0)):
        gv, gf = icosphere(radius, 1 + i % 2)
        ev, ef = icosphere(radius * (1.02 + 0.02 * i), 2)
        _write_obj(str(gt / f"frame_{i:03d}.obj"), gv + shift, gf)      # stored with the camera origin still in
        P.write_mesh_ply(str(pred / f"frame_{i:03d}.ply"), ev @ R, ef)  # stored in the method's frame
        meshes.append((gv, gf, ev, ef))
    (scene / "transforms_train.json").write_text(json.dumps({"camera_origin": origin, "frames": []}))
    avg_cd, cd_list, avg_emd, emd_list = M.evaluation(str(gt), str(pred), "dgmesh", emd_sample=512, seed=4)
    assert len(cd_list) == 3 and len(emd_list) == 3
    assert all(isinstance(x, float) and np.isfinite(x) and x > 0 for x in cd_list + emd_list)
    assert avg_cd == pytest.approx(np.mean(cd_list), rel=1e-12) and avg_emd == pytest.approx(np.mean(emd_list), rel=1e-12)
    for (gv, gf, ev, ef), cd in zip(meshes, cd_list):  # shift and rotation undone: the Chamfer distance of the meshes as built
        dl, dr = brute_chamfer(gv, ev)
        assert cd == pytest.approx((dl + dr) / 2, rel=1e-4)
    again = M.evaluation(str(gt), str(pred), "dgmesh", emd_sample=512, seed=4)
    assert again[1] == cd_list and again[3] == emd_list  # same seed, same samples, same bits
    # a count mismatch raises
    (pred / "frame_999.ply").write_bytes((pred / "frame_000.ply").read_bytes())
    with pytest.raises(ValueError, match="3 ground-truth meshes .* 4 predicted"):
        M.evaluation(str(gt), str(pred), "dgmesh")
    os.remove(str(pred / "frame_999.ply"))
    # the command line writes the reference's four lines
    out = M.main(["--path", str(scene), "--eval_type", "dgmesh", "--emd_sample", "512", "--seed", "4"])
    assert os.path.basename(out) == "eval_results.txt" and os.path.dirname(os.path.dirname(out)) == str(scene / "DGMesh" / "results")
    assert os.path.basename(os.path.dirname(out)).startswith("scene_")
    lines = open(out).read().splitlines()
    assert len(lines) == 4
    assert lines[0] == f"GT source: {gt}" and lines[1] == f"Pred source: {pred}"
    assert lines[2] == f"Average Chamfer distance: {avg_cd:.10f}" and lines[3] == f"Average EMD: {avg_emd:.4f}"
