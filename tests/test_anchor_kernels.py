"""The anchoring kernels (csrc/anchor.hip through dg-mesh_amd/anchor.py) against float64 / brute-force restatements:
face geometry, the exact bounded nearest neighbour (grid for a finite bound, tiled brute force for +inf) and the per-face
classification.  Every test prints its error."""
import math

import numpy as np
import pytest
import torch

from conftest import pkg
from _anchor_ref import nearest32

DEV = "cuda:0"


def A():
    return pkg("anchor")


def _fp64_geometry(v, f):
    v = v.double()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = torch.cross(b - a, c - a, dim=1)
    ln = n.norm(dim=1, keepdim=True)
    return (a + b + c) / 3, torch.where(ln > 0, n / ln.clamp_min(1e-300), torch.zeros_like(n))


@pytest.mark.gpu
def test_face_geometry_against_fp64_degenerate_empty_and_out_of_range():
    g = torch.Generator().manual_seed(0)
    V, F = 500, 4000
    v = torch.randn(V, 3, generator=g)
    f = torch.randint(0, V, (F, 3), generator=g, dtype=torch.int32)
    f[:50, 1] = f[:50, 0]                                  # two equal indices: zero area
    v[10] = v[11] = v[12]                                  # three equal positions
    f[50] = torch.tensor([10, 11, 12])
    f[60, 2] = V                                           # out of range
    f[61, 0] = -1
    cent, nrm = A().face_geometry(v.to(DEV), f.to(DEV))
    c64, n64 = _fp64_geometry(v, f.long().clamp(0, V - 1))
    ok = torch.ones(F, dtype=torch.bool)
    ok[60] = ok[61] = False
    ec = float((cent.cpu().double()[ok] - c64[ok]).abs().max())
    en = float((nrm.cpu().double()[ok] - n64[ok]).abs().max())
    print(f"centroid err {ec:.3e}, normal err {en:.3e}")
    assert ec <= 4e-7 * float(v.abs().max()) and en <= 1e-5
    assert torch.all(nrm[:51] == 0)
    assert torch.isnan(cent[60]).all() and torch.isnan(cent[61]).all() and torch.all(nrm[60:62] == 0)
    c0, n0 = A().face_geometry(v.to(DEV), torch.zeros((0, 3), dtype=torch.int32, device=DEV))
    assert c0.shape == (0, 3) and n0.shape == (0, 3)


def _check_nn(q, t, max_d2, tag):
    idx, d2 = A().nearest(q, t, max_d2)
    ridx, rd2 = nearest32(q, t, max_d2, chunk=256)
    bad = int((idx != ridx).sum())
    same_d2 = bool(torch.equal(d2, rd2))
    # fp64 distance of the chosen target
    ok = idx >= 0
    err = 0.0
    if ok.any():
        d64 = ((q[ok].double() - t[idx[ok]].double()) ** 2).sum(1)
        err = float(((d2[ok].double() - d64).abs() / d64.clamp_min(1e-30)).max())
    print(f"{tag}: Nq={q.shape[0]} Nt={t.shape[0]} found={int(ok.sum())} idx mismatches={bad} d2 bit-equal={same_d2} "
          f"d2 rel err vs fp64={err:.2e}")
    assert bad == 0 and same_d2 and err <= 1e-6
    idx2, d22 = A().nearest(q, t, max_d2)
    assert torch.equal(idx, idx2) and torch.equal(d2, d22)
    return idx, d2


@pytest.mark.gpu
@pytest.mark.parametrize("max_d2", [1e-3, 2e-2, 0.3, math.inf])
def test_nearest_uniform_and_clustered(max_d2):
    g = torch.Generator().manual_seed(1)
    q = torch.rand(3000, 3, generator=g).to(DEV)
    t = torch.rand(7000, 3, generator=g).to(DEV)
    _check_nn(q, t, max_d2, "uniform")
    centers = torch.rand(12, 3, generator=g)
    tc = (centers[torch.randint(0, 12, (9000,), generator=g)] + 0.01 * torch.randn(9000, 3, generator=g)).to(DEV)
    _check_nn(q, tc, max_d2, "clustered")
    # a permuted target order gives the same (mapped) answer
    perm = torch.randperm(7000, generator=g).to(DEV)
    idx, d2 = A().nearest(q, t, max_d2)
    idp, d2p = A().nearest(q, t[perm], max_d2)
    assert torch.equal(d2, d2p) and torch.equal(torch.where(idp >= 0, perm[idp.clamp_min(0)], idp), idx)


@pytest.mark.gpu
@pytest.mark.parametrize("max_d2", [0.05, math.inf])
def test_nearest_ties_exact_hits_strict_bound_and_sizes(max_d2):
    g = torch.Generator().manual_seed(2)
    base = torch.rand(500, 3, generator=g)
    t = torch.cat([base, base, base[:100]]).to(DEV)           # every target three or two times: ties -> smallest index
    q = torch.cat([base[:200] + 0.001 * torch.randn(200, 3, generator=g), base[200:300]]).to(DEV)  # (the last 100 ON a target)
    idx, d2 = _check_nn(q, t, max_d2, "duplicates")
    assert torch.all(idx[idx >= 0] < 500)
    assert torch.all(d2[200:] == 0) and torch.equal(idx[200:].cpu(), torch.arange(200, 300))
    # targets exactly at d2 == max_d2 are not reported (strict)
    qq = torch.zeros(1, 3, device=DEV)
    tt = torch.tensor([[0.25, 0.0, 0.0], [0.0, 0.5, 0.0]], device=DEV)
    i0, e0 = A().nearest(qq, tt, 0.0625)
    i1, e1 = A().nearest(qq, tt, float(np.nextafter(np.float32(0.0625), np.float32(1))))
    print("strict bound:", i0.tolist(), e0.tolist(), i1.tolist(), e1.tolist())
    assert i0.tolist() == [-1] and math.isinf(float(e0)) and i1.tolist() == [0] and float(e1) == 0.0625
    # Nt = 0, Nt = 1, Nq = 0
    ie, de = A().nearest(q, t[:0], max_d2)
    assert torch.all(ie == -1) and torch.all(torch.isinf(de))
    _check_nn(q, t[:1], max_d2, "Nt=1")
    i_, d_ = A().nearest(q[:0], t, max_d2)
    assert i_.shape == (0,) and d_.shape == (0,)


@pytest.mark.gpu
def test_nearest_unbounded_20k_x_200k():
    g = torch.Generator().manual_seed(3)
    q = torch.randn(20000, 3, generator=g).to(DEV)
    t = torch.randn(200000, 3, generator=g).to(DEV)
    _check_nn(q, t, math.inf, "unbounded 20k x 200k")


def _classify_ref(face_of, F):
    fo = face_of.long().cpu()
    valid = fo >= 0
    fi = fo[valid]
    uniq, cnt = torch.unique(fi, return_counts=True)
    counts = torch.zeros(F, dtype=torch.long)
    counts[uniq] = cnt
    allf = torch.arange(F)
    f11, fn1 = uniq[cnt == 1], uniq[cnt > 1]
    f01 = allf[~(torch.isin(allf, f11) | torch.isin(allf, fn1))]
    rank = torch.full((fo.shape[0],), -1, dtype=torch.long)
    for f in torch.unique(fi).tolist() if fi.numel() < 5000 else []:
        m = torch.nonzero(fo == f).squeeze(1)
        rank[m] = torch.arange(m.numel())
    return counts, torch.cat([f11, fn1, f01]), rank, (f11.numel(), fn1.numel(), f01.numel(), int(valid.sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["random", "one_face", "every_face", "none_valid", "no_faces", "large"])
def test_classify_against_unique_isin_cumsum(case):
    g = torch.Generator().manual_seed(4)
    P, F = 3000, 2000
    if case == "random":
        fo = torch.randint(-1, F, (P,), generator=g)
    elif case == "one_face":
        fo = torch.full((P,), 777)
    elif case == "every_face":
        fo = torch.cat([torch.randperm(F, generator=g), torch.randint(0, F, (P - F,), generator=g)])
    elif case == "none_valid":
        fo = torch.full((P,), -1)
    elif case == "no_faces":
        F, fo = 0, torch.full((P,), -1)
    else:
        P, F = 200000, 4_720_000
        fo = torch.randint(-1, 60000, (P,), generator=g) * 71
        fo[fo < 0] = -1
    c = A().classify(fo.to(torch.int32).to(DEV), F)
    counts, lists, rank, totals = _classify_ref(fo, F)
    print(case, "totals", c["totals"], "ref", totals)
    assert c["totals"] == totals
    assert torch.equal(c["counts"].cpu().long(), counts) and torch.equal(c["lists"].cpu().long(), lists)
    off = torch.cumsum(counts, 0) - counts
    assert torch.equal(c["offsets"].cpu().long(), off)
    if P < 5000:
        assert torch.equal(c["rank"].cpu().long(), rank)
    # members: valid Gaussians by (face, index)
    fo_ = fo.clone()
    v = torch.nonzero(fo_ >= 0).squeeze(1)
    order = v[torch.argsort(fo_[v] * (P + 1) + v)]
    mem = c["members"].cpu().long()
    assert torch.equal(mem[:order.numel()], order) and torch.all(mem[order.numel():] == -1)
    r = c["rank"].cpu().long()
    assert torch.equal(r[order], torch.arange(order.numel()) - off[fo_[order]]) and torch.all(r[fo_ < 0] == -1)


@pytest.mark.gpu
def test_nearest_at_scale_on_the_bench_mesh():
    """bench.py's mesh-phase scene (P = 100 k Gaussians, DPSR 288^3 -> DiffMC, ~4.7 M faces): 4096 of its deformed Gaussians against
    every face centroid, at the bounds of search_radius 0.0005 and 0.0015 (gaussian_scale * radius), against the chunked fp32
    brute force: exact."""
    import bench
    dev = torch.device(DEV)
    tr, _ = bench.build_scene(dev, 0, 1, "hip", n_frames=2, phase="mesh", dpsr_res=288)
    ms, g = tr.mesh, tr.g
    with torch.no_grad():
        verts, faces = ms.surface(g, ms.psr(g, None, None).contiguous())
        P = g._xyz.shape[0]
        x = g.get_xyz + tr.deform.step(g.get_xyz, tr.cameras[0].fid.reshape(1, 1).expand(P, -1))[0]
    cent, _ = A().face_geometry(verts, faces)
    F = cent.shape[0]
    assert P == 100_000 and F > 4_500_000, (P, F)
    gen = torch.Generator(device=DEV).manual_seed(5)
    q = x[torch.randperm(P, device=DEV, generator=gen)[:4096]].contiguous()
    scale = float(g.gaussian_scale.reshape(-1)[0])
    for r in (0.0005, 0.0015):
        bound = float(torch.tensor(scale, dtype=torch.float32) * r)
        idx, _ = _check_nn(q, cent, bound, f"bench mesh F={F} radius {r}")
        assert int((idx >= 0).sum()) > 1000
