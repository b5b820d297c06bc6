"""GPU tests of the inside / outside queries (dg-mesh_amd/mesh_inside.py, csrc/mesh_inside.hip, mesh_eval.evaluation_iou) against the
numpy restatement of the definition (tests/_inside_ref.py).

Values: |w_dev - w64| <= tol on every query, w64 the fp64 statement.  tol is not chosen: per case it is 8 x the largest |w32 - w64|
of the numpy fp32 statement in the device's summation order -- what the number format gives on that case -- and the factor 8 covers
the device's atan2f, which differs from numpy's by a few ulp per term.  The device's largest error is printed per case.
Classification: contains() equals w64 >= 0.5 on every query at least 0.05 away from the threshold; the share of closer ones is
asserted to be small.  Every case runs twice and in parts: the same bytes.

Queries: uniform in the mesh's bounding box scaled by 1.1 about its centre, seeded."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import _edges_ref as E
import _inside_ref as R
import _surface_ref as S
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_FACTOR = 8.0
MARGIN = 0.05


def MI():
    return pkg("mesh_inside")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)  # (a copy: the shared cases are read-only)


def build(name):
    verts, faces = E.icosphere(2)
    if name == "sphere":
        return verts, faces
    if name == "torus":  # 17266 = 67 * 256 + 114 faces: ragged against the chunk, across the 16384-face slice boundary
        return E.torus(97, 89)
    if name == "open":
        return R.open_icosphere(2, 0.3)
    if name == "disjoint":
        return R.join((verts, faces), (verts * np.float32(0.7) + np.float32([2.5, 0.3, -0.2]), faces))
    if name == "nested_reversed":
        return R.join((verts, faces), (verts * np.float32(0.5), R.reversed_faces(faces)))
    if name == "soup":
        return E.random_soup()
    if name == "salted":
        return R.salted_icosphere(2)[:2]
    if name == "mc_sphere":  # what DiffMC produces: watertight, with the tiny faces and slivers of an isosurface grazing lattice nodes
        return S.mc_sphere(1e-3)
    raise KeyError(name)


CASES = {"sphere": 4000, "torus": 520, "open": 4000, "disjoint": 4000, "nested_reversed": 4000, "soup": 4000, "salted": 4000,
         "mc_sphere": 4000}  # name -> N


@functools.lru_cache(maxsize=None)
def case(name):
    """The mesh, the queries and both numpy statements, computed once and shared (read-only)."""
    verts, faces = build(name)
    queries = R.box_queries(verts, CASES[name], seed=len(name))
    w64 = R.winding(queries, verts, faces, np.float64)
    w32 = R.winding(queries, verts, faces, np.float32)
    for a in (verts, faces, queries, w64, w32):
        a.setflags(write=False)
    return verts, faces, queries, w64, w32


def test_cases_are_what_they_claim():
    assert build("sphere")[1].shape == (320, 3) and build("open")[1].shape == (210, 3)
    verts, faces = build("torus")
    assert verts.shape == (8633, 3) and faces.shape == (17266, 3)
    w64 = case("soup")[3]
    assert w64.min() < -8 and w64.max() > 8  # many overlapping sheets
    verts, faces = build("salted")
    assert (faces < 0).any() and (faces >= len(verts)).any() and np.isnan(verts).any()


@pytest.mark.parametrize("name", list(CASES))
def test_values_classification_and_reproducibility(name):
    M = MI()
    verts, faces, queries, w64, w32 = case(name)
    p, v, f = dev(queries), dev(verts), dev(faces)
    keep = [t.clone() for t in (p, v, f)]
    w = M.winding_number(p, v, f)
    assert w.shape == (len(queries),) and w.dtype == torch.float32 and w.device.type == "cuda"
    got = w.cpu().numpy()
    # values
    ref_err = float(np.abs(w32.astype(np.float64) - w64).max())
    tol = TOL_FACTOR * ref_err
    err = float(np.abs(got.astype(np.float64) - w64).max())
    print(f"{name}: F {len(faces)}, N {len(queries)}: device max |w - w64| {err:.3e}; numpy fp32 statement {ref_err:.3e}, tolerance {tol:.3e}; "
          f"w64 in [{w64.min():.2f}, {w64.max():.2f}]")
    assert np.isfinite(got).all()
    assert err <= tol, f"{name}: {err:.3e} > {tol:.3e}"
    # classification
    far = np.abs(w64 - 0.5) >= MARGIN
    print(f"{name}: {1 - far.mean():.3%} of the queries within {MARGIN} of the threshold")
    assert 1 - far.mean() <= 0.05
    inside = M.contains(p, v, f).cpu().numpy()
    assert inside.dtype == np.bool_ and (inside[far] == (w64 >= 0.5)[far]).all()
    assert (inside == (got >= 0.5)).all()
    lax = M.contains(p, v, f, threshold=0.25, absolute=True).cpu().numpy()
    assert (lax == (np.abs(got) >= 0.25)).all()
    # the same bytes: a second run, the first 65 queries alone, one query alone
    same = lambda a, b: bool((a.view(torch.int32) == b.view(torch.int32)).all())
    assert same(M.winding_number(p, v, f), w)
    assert same(M.winding_number(p[:65].contiguous(), v, f), w[:65])
    assert same(M.winding_number(p[64:65].contiguous(), v, f), w[64:65])
    for t, k in zip((p, v, f), keep):  # inputs unmodified (NaN vertices compared as bytes)
        assert bool((t.view(torch.int32) == k.view(torch.int32)).all())


def test_batches_change_no_bit(monkeypatch):
    M = MI()
    verts, faces, queries, _, _ = case("torus")
    p, v, f = dev(queries), dev(verts), dev(faces)
    whole = M.winding_number(p, v, f)
    monkeypatch.setattr(M, "batch_rows", lambda F: 256)  # 520 queries in batches of 256, 256 and 8
    parts = M.winding_number(p, v, f)
    assert bool((parts.view(torch.int32) == whole.view(torch.int32)).all())


def test_reversed_mesh_and_absolute():
    M = MI()
    verts, faces, queries, w64, _ = case("sphere")
    p, v = dev(queries), dev(verts)
    fwd, rev = dev(faces), dev(R.reversed_faces(faces))
    w_rev = M.winding_number(p, v, rev).cpu().numpy()
    assert np.abs(w_rev + w64).max() < 1e-5
    assert not bool(M.contains(p, v, rev).any())
    assert bool((M.contains(p, v, rev, absolute=True) == M.contains(p, v, fwd)).all())


def test_edge_cases():
    M = MI()
    verts, faces, queries, _, _ = case("sphere")
    p, v, f = dev(queries[:300]), dev(verts), dev(faces)
    none_f = torch.zeros((0, 3), dtype=torch.int32, device=DEV)
    none_v = torch.zeros((0, 3), dtype=torch.float32, device=DEV)
    for w in (M.winding_number(p, v, none_f), M.winding_number(p, none_v, f), M.winding_number(p, none_v, none_f),
              M.winding_number(p, v, torch.full((500, 3), -1, dtype=torch.int32, device=DEV)),
              M.winding_number(p, v, f + len(verts))):
        assert w.shape == (300,) and bool((w.view(torch.int32) == 0).all())  # +0.0
    empty = M.winding_number(p[:0], v, f)
    assert empty.shape == (0,) and empty.dtype == torch.float32
    assert M.contains(p[:0], v, f).shape == (0,) and M.signed_distance(p[:0], v, f).shape == (0,)
    # a query with a non-finite coordinate gets NaN, its neighbours what they get without it
    bad = p.clone()
    bad[5, 0], bad[70, 1], bad[299, 2] = float("nan"), float("inf"), float("-inf")
    w, w_bad = M.winding_number(p, v, f), M.winding_number(bad, v, f)
    rows = torch.tensor([5, 70, 299], device=DEV)
    assert bool(torch.isnan(w_bad[rows]).all()) and bool(torch.isnan(M.winding_number(bad, v, none_f)[rows]).all())
    rest = torch.ones(300, dtype=torch.bool, device=DEV)
    rest[rows] = False
    assert bool((w_bad[rest].view(torch.int32) == w[rest].view(torch.int32)).all())
    assert not bool(M.contains(bad, v, f)[rows].any())
    # on the surface itself: unspecified but finite (vertices, edge midpoints, face centroids)
    tri = verts[faces]
    on = np.concatenate([verts, (tri[:, 0] + tri[:, 1]) / 2, tri.mean(1)]).astype(np.float32)
    assert bool(torch.isfinite(M.winding_number(dev(on), v, f)).all())
    with pytest.raises(RuntimeError, match="must be torch.int32"):
        M.winding_number(p, v, f.long())
    with pytest.raises(RuntimeError, match="must be torch.float32"):
        M.winding_number(p.double(), v, f)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        M.winding_number(p.reshape(-1), v, f)


@pytest.mark.parametrize("name", ["sphere", "open"])
def test_signed_distance(name):
    M, C = MI(), pkg("correspondence")
    verts, faces, queries, w64, _ = case(name)
    p, v, f = dev(queries), dev(verts), dev(faces)
    same = lambda a, b: bool((a.view(torch.int32) == b.view(torch.int32)).all())
    inside = M.contains(p, v, f)
    sd = M.signed_distance(p, v, f)
    assert sd.dtype == torch.float32 and same(sd.abs(), C.closest_on_mesh(p, v, f)[1].sqrt())
    assert (sd.abs().cpu().numpy().view(np.uint32) == np.sqrt(S.closest32(queries, verts, faces)[1]).view(np.uint32)).all()  # numpy's statement of it
    assert bool(((sd < 0) == inside).all()) and bool(torch.isfinite(sd).all())
    if name == "sphere":  # |p| - 1 up to the faceting of the icosphere (its faces lie up to 1 - cos(edge / 2) ~ 0.02 inside the sphere)
        r = np.linalg.norm(queries.astype(np.float64), axis=1)
        assert np.abs(sd.cpu().numpy() - (r - 1)).max() < 0.03
    face, d2, _ = C.closest_on_mesh(p, v, f, max_dist=0.2)
    near = M.signed_distance(p, v, f, max_dist=0.2)
    lost = face < 0
    assert 0 < int(lost.sum()) < len(queries)
    assert bool((torch.isinf(near) == lost).all()) and same(near.abs(), d2.sqrt())
    assert bool(((near < 0) == inside).all())  # -inf inside, +inf outside
    assert same(near[~lost], sd[~lost])
    flipped = M.signed_distance(p, v, dev(R.reversed_faces(faces)))
    assert bool((flipped >= 0).all())  # wound inwards: nothing counts as inside ...
    if name == "sphere":  # ... unless |w| is asked for (the corners arrive in another order: the same distance up to rounding)
        unflipped = M.signed_distance(p, v, dev(R.reversed_faces(faces)), absolute=True)
        assert bool(((unflipped < 0) == inside).all()) and float((unflipped - sd).abs().max()) < 1e-6


def test_occupancy_grid():
    M = MI()
    verts, faces, _, _, _ = case("sphere")
    v, f = dev(verts), dev(faces)
    res = 8

    def centres(lo, hi):  # lo + (i + 0.5) / res * (hi - lo) per axis in fp32, x slowest
        t = ((np.arange(res, dtype=np.float32) + np.float32(0.5)) / np.float32(res)).astype(np.float32)
        ax = [np.float32(lo[a]) + t * np.float32(hi[a] - lo[a]) for a in range(3)]
        return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)

    grid = M.occupancy_grid(v, f, res)
    assert grid.shape == (res, res, res) and grid.dtype == torch.bool
    lo, hi = verts.min(0), verts.max(0)
    c = centres(lo, hi)
    assert bool((grid.reshape(-1) == M.contains(dev(c), v, f)).all())
    w64 = R.winding(c, verts, faces, np.float64)
    far = np.abs(w64 - 0.5) >= MARGIN
    assert far.mean() > 0.95 and (grid.reshape(-1).cpu().numpy()[far] == (w64 >= 0.5)[far]).all()
    assert 0 < int(grid.sum()) < res ** 3 and bool(grid[res // 2, res // 2, res // 2]) and not bool(grid[0, 0, 0])
    # an explicit box, not a cube: the axes are (x, y, z)
    lo, hi = np.float32([-0.25, -1.5, 0.0]), np.float32([1.75, 1.5, 0.5])
    grid = M.occupancy_grid(v, f, res, lo=tuple(lo), hi=torch.from_numpy(hi).to(DEV))
    assert bool((grid.reshape(-1) == M.contains(dev(centres(lo, hi)), v, f)).all())
    assert not bool(grid[:, 0, :].any()) and not bool(grid[-1].any()) and bool(grid[0, res // 2, 0])
    flipped = M.occupancy_grid(v, dev(R.reversed_faces(faces)), res, absolute=True)
    assert bool((flipped == M.occupancy_grid(v, f, res)).all())
    with pytest.raises(ValueError, match="res"):
        M.occupancy_grid(v, f, 0)
    with pytest.raises(ValueError, match="both lo and hi"):
        M.occupancy_grid(v, f, 4, lo=(0, 0, 0))


def test_volume_iou():
    M = MI()
    verts, faces = E.icosphere(3)
    shifted = (verts + np.float32([0.5, 0, 0])).astype(np.float32)
    va, vb, f = dev(verts), dev(shifted), dev(faces)
    n = 65536
    gen = torch.Generator(device=DEV).manual_seed(11)
    out = M.volume_iou(va, f, vb, f, n_points=n, generator=gen, return_points=True)
    assert set(out) == {"iou", "n_a", "n_b", "n_inter", "n_union", "volume_a", "volume_b", "points"}
    assert all(out[k].dtype == torch.int64 and out[k].is_cuda and out[k].dim() == 0 for k in ("n_a", "n_b", "n_inter", "n_union"))
    assert all(out[k].dtype == torch.float64 and out[k].is_cuda and out[k].dim() == 0 for k in ("iou", "volume_a", "volume_b"))
    points = out["points"]
    assert points.shape == (n, 3) and points.dtype == torch.float32
    pts = points.cpu().numpy()
    lo, hi = np.minimum(verts.min(0), shifted.min(0)), np.maximum(verts.max(0), shifted.max(0))
    assert (pts >= lo).all() and (pts <= hi).all() and (pts.min(0) < lo + 0.01).all() and (pts.max(0) > hi - 0.01).all()
    # the counts against numpy fp64 at the returned points, without the samples the reference puts within MARGIN of the threshold
    wa, wb = R.winding(pts, verts, faces, np.float64), R.winding(pts, shifted, faces, np.float64)
    near = (np.abs(np.abs(wa) - 0.5) < MARGIN) | (np.abs(np.abs(wb) - 0.5) < MARGIN)
    print(f"volume_iou: {near.mean():.4%} of {n} samples within {MARGIN} of the threshold")
    assert near.mean() <= 0.001
    in_a, in_b = M.contains(points, va, f, absolute=True), M.contains(points, vb, f, absolute=True)  # the same bits as inside volume_iou
    count = lambda t: int(t.sum())
    assert (count(in_a), count(in_b), count(in_a & in_b), count(in_a | in_b)) == tuple(int(out[k]) for k in ("n_a", "n_b", "n_inter", "n_union"))
    ra, rb, far = np.abs(wa) >= 0.5, np.abs(wb) >= 0.5, ~near
    da, db = in_a.cpu().numpy(), in_b.cpu().numpy()
    assert (da[far] == ra[far]).all() and (db[far] == rb[far]).all()
    for dev_mask, ref_mask in ((da, ra), (db, rb), (da & db, ra & rb), (da | db, ra | rb)):
        assert int(dev_mask[far].sum()) == int(ref_mask[far].sum())
    assert float(out["iou"]) == int(out["n_inter"]) / int(out["n_union"])
    # the volumes: box volume x share, within four binomial standard deviations of the polyhedron's volume
    box = float(np.prod((hi - lo).astype(np.float64)))
    vol = E.enclosed_volume(verts, faces)
    share = vol / box
    bound = 4 * box * (share * (1 - share) / n) ** 0.5
    print(f"volume_iou: volume_a {float(out['volume_a']):.5f}, volume_b {float(out['volume_b']):.5f}, polyhedron {vol:.5f}, bound {bound:.5f}; "
          f"iou {float(out['iou']):.5f}")
    assert abs(float(out["volume_a"]) - vol) <= bound and abs(float(out["volume_b"]) - vol) <= bound
    assert float(out["volume_a"]) == pytest.approx(box * int(out["n_a"]) / n, rel=1e-6)  # (the device's box is the fp32 one)
    # two unit spheres 0.5 apart: the lens is 1 - 3 d / 4 + d^3 / 16 of a sphere, so IoU = 0.6328 / 1.3672 = 0.463 for exact spheres
    assert abs(float(out["iou"]) - 0.463) < 0.02
    # the same generator state, the same samples; a mesh against itself; disjoint meshes; padding; nothing inside
    again = M.volume_iou(va, f, vb, f, n_points=n, generator=torch.Generator(device=DEV).manual_seed(11))
    assert "points" not in again and all(bool(again[k] == out[k]) for k in again)
    itself = M.volume_iou(va, f, va.clone(), f.clone(), n_points=4096, generator=gen)
    assert float(itself["iou"]) == 1.0 and int(itself["n_a"]) == int(itself["n_inter"]) == int(itself["n_union"]) > 0
    apart = M.volume_iou(va, f, dev(verts + np.float32([2.5, 0, 0])), f, n_points=4096, generator=gen)
    assert float(apart["iou"]) == 0.0 and int(apart["n_inter"]) == 0 and int(apart["n_union"]) == int(apart["n_a"]) + int(apart["n_b"]) > 0
    padded = M.volume_iou(va, f, va, f, n_points=4096, generator=gen, padding=0.5, return_points=True)
    diag = float(np.linalg.norm((verts.max(0) - verts.min(0)).astype(np.float64)))
    assert float(padded["points"].min()) < -1.3 and float(padded["points"].min()) >= float(verts.min()) - 0.5 * diag - 1e-5
    reversed_ = dev(R.reversed_faces(faces))
    assert float(M.volume_iou(va, reversed_, vb, f, n_points=4096, generator=gen)["iou"]) > 0.4  # absolute=True by default
    nothing = M.volume_iou(va, reversed_, vb, reversed_, n_points=4096, generator=gen, absolute=False)
    assert np.isnan(float(nothing["iou"])) and int(nothing["n_union"]) == 0 and float(nothing["volume_a"]) == 0.0


def _write_obj(path, verts, faces):
    with open(path, "w") as fh:
        for p in verts:
            fh.write(f"v {p[0]:.9g} {p[1]:.9g} {p[2]:.9g}\n")
        for t in faces:
            fh.write(f"f {t[0] + 1} {t[1] + 1} {t[2] + 1}\n")


def test_evaluation_iou_and_command_lines(tmp_path, capsys):
    M, ME, P = MI(), pkg("mesh_eval"), pkg("ply_io")
    scene = tmp_path / "scene"
    gt, pred = scene / "gt", scene / "DGMesh" / "dynamic_mesh"
    gt.mkdir(parents=True)
    pred.mkdir(parents=True)
    rot = np.asarray(ME.ROTATIONS["dgmesh"], np.float32)
    origin = [0.1, -0.2, 0.3]
    shift = np.array([origin[0], origin[2], -origin[1]], np.float32)
    verts, faces = E.icosphere(2)
    meshes = []
    for i, (scale, offset) in enumerate(((1.0, 0.0), (0.9, 0.0), (1.0, 0.4))):  # the same, a smaller one, a shifted one
        gv = verts
        ev = (verts * np.float32(scale) + np.float32([offset, 0, 0])).astype(np.float32)
        _write_obj(str(gt / f"frame_{i:03d}.obj"), gv + shift, faces)      # stored with the camera origin still in
        P.write_mesh_ply(str(pred / f"frame_{i:03d}.ply"), ev @ rot, faces)  # stored in the method's frame
        meshes.append((gv, ev))
    (scene / "transforms_train.json").write_text(json.dumps({"camera_origin": origin, "frames": []}))
    n = 8192
    avg, ious = ME.evaluation_iou(str(gt), str(pred), "dgmesh", n_points=n, seed=4)
    assert len(ious) == 3 and all(isinstance(x, float) for x in ious) and avg == pytest.approx(np.mean(ious), rel=1e-12)
    # by hand: the files as evaluation_iou reads them, the shift and the rotation applied, one generator through the three pairs
    gen = torch.Generator(device=DEV).manual_seed(4)
    by_hand = []
    for i in range(3):
        gv, gf = ME.read_mesh_obj(str(gt / f"frame_{i:03d}.obj"))
        ev, ef = P.read_mesh_ply(str(pred / f"frame_{i:03d}.ply"))
        gv_d = dev(gv) - torch.tensor(shift, device=DEV)
        ev_d = (torch.tensor(rot, device=DEV) @ dev(ev).T).T.contiguous()
        by_hand.append(float(M.volume_iou(gv_d, dev(gf), ev_d, dev(ef), n_points=n, generator=gen, absolute=True)["iou"]))
    assert ious == by_hand
    print("evaluation_iou:", ious)
    assert ious[0] > 0.99 and abs(ious[1] - 0.9 ** 3) < 0.03 and 0.3 < ious[2] < 0.7  # nested spheres: the ratio of the volumes
    assert ME.evaluation_iou(str(gt), str(pred), "dgmesh", n_points=n, seed=4)[1] == ious
    # mesh_eval's command line: byte-identical without the flag, the new lines with it
    avg_cd, _, avg_emd, _ = ME.evaluation(str(gt), str(pred), "dgmesh", emd_sample=512, seed=4)
    four = (f"GT source: {gt}\nPred source: {pred}\nAverage Chamfer distance: {avg_cd:.10f}\nAverage EMD: {avg_emd:.4f}\n")
    capsys.readouterr()
    plain = ME.main(["--path", str(scene), "--eval_type", "dgmesh", "--emd_sample", "512", "--seed", "4"])
    assert open(plain).read() == four
    printed = capsys.readouterr().out
    assert "IoU" not in printed and printed.count("Item ") == 3
    with_iou = ME.main(["--path", str(scene), "--eval_type", "dgmesh", "--emd_sample", "512", "--seed", "4", "--iou", str(n)])
    text = open(with_iou).read()
    extra = "".join(f"Item {i}: IoU {x:.6f}\n" for i, x in enumerate(ious)) + f"Average volume IoU: {avg:.6f}\n"
    assert text == four + extra
    printed = capsys.readouterr().out
    assert extra in printed and printed.count("Item ") == 6
    # mesh_inside's command line: one JSON line
    a, b = str(pred / "frame_000.ply"), str(pred / "frame_002.ply")
    assert M.main([a, b, "--points", "4096", "--seed", "3"]) == 0
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1
    rep = json.loads(line[0])
    ev0, ev2 = P.read_mesh_ply(a), P.read_mesh_ply(b)
    want = M.volume_iou(dev(ev0[0]), dev(ev0[1]), dev(ev2[0]), dev(ev2[1]), n_points=4096, generator=torch.Generator(device=DEV).manual_seed(3))
    assert (rep["mesh_a"], rep["mesh_b"], rep["points"], rep["seed"]) == (a, b, 4096, 3)
    assert rep["iou"] == float(want["iou"]) and rep["n_inter"] == int(want["n_inter"]) and rep["n_union"] == int(want["n_union"])
    assert rep["volume_a"] == float(want["volume_a"]) and os.path.exists(a)
