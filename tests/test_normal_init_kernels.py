"""The dgm_ninit_* kernels (dg-mesh_amd/normal_init.py, csrc/normal_init.hip) on the GPU: the one-launch bounding box against
torch.aminmax (bit-exact, NaN propagation), centre / scale against the float64 restatement, face areas against float64, surface
sampling against the reference's golden and on bench.py's 4.7 M-face mesh, and the stage chain samples -> nearest -> normals
against the golden."""
import math
import os
import types

import numpy as np
import pytest
import torch

import _ninit_ref as NR
from _anchor_ref import PolyField
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "normal_init_small.npz")
CHI2_63_1E6 = 131.37  # upper 1e-6 quantile of chi-square with 63 degrees of freedom (131.3697)


def N():
    return pkg("normal_init")


def dt(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def bits_equal_or_both_nan(a, b):
    nan = torch.isnan(a)
    return bool(torch.equal(nan, torch.isnan(b))) and bool(torch.equal(a[~nan].view(torch.int32), b[~nan].view(torch.int32)))


@pytest.mark.parametrize("P", [1, 63, 64, 65, 100_003])
@pytest.mark.parametrize("nan_row", [False, True])
@pytest.mark.parametrize("with_delta", [True, False])
def test_bbox_is_bit_exact(P, nan_row, with_delta):
    gen = torch.Generator(device=DEV).manual_seed(P)
    xyz = torch.randn((P, 3), device=DEV, generator=gen) * 3.0
    d = torch.randn((P, 3), device=DEV, generator=gen) * 0.1 if with_delta else None
    if nan_row:
        xyz[P // 2, 1] = float("nan")
    pts = xyz + d if with_delta else xyz
    mn, mx = torch.aminmax(pts, dim=0)
    want = torch.cat([mn, mx])
    scratch = N().bbox_scratch(xyz.device)
    for _ in range(2):  # (the scratch serves the next launch)
        got = N().bbox(xyz, d, scratch=scratch)
        assert bits_equal_or_both_nan(got, want), (got, want)
    if nan_row:  # NaN propagates, like torch.max / torch.min: both extrema of that axis, no other
        assert torch.isnan(got).tolist() == [False, True, False, False, True, False]
    # rows that do not start on a 16-byte boundary take the scalar path
    if P > 1:
        sub = xyz[1:]
        mn, mx = torch.aminmax(sub, dim=0)
        assert sub.data_ptr() % 16 != 0
        assert bits_equal_or_both_nan(N().bbox(sub), torch.cat([mn, mx]))


def test_bbox_orders_the_two_zeros():
    """-0 counts as less than +0, so the sign of a zero extremum does not depend on where the zeros sit (torch.aminmax makes no such
    promise, which is why this case is not compared with it)."""
    for P in (5, 3000):
        for first, second in ((0.0, -0.0), (-0.0, 0.0)):
            x = torch.zeros((P, 3), device=DEV)
            x[:, 0] = -1.0 - torch.arange(P, device=DEV)   # axis 0: max is -1
            x[0, 1], x[P - 1, 1] = first, second           # axis 1: both zeros, min -0, max +0
            x[1:P - 1, 1] = first
            x[:, 2] = 1.0 + torch.arange(P, device=DEV)
            got = N().bbox(x)
            assert torch.signbit(got[1]) and not torch.signbit(got[4]) and float(got[1]) == 0.0 == float(got[4])
            assert float(got[3]) == -1.0 and float(got[2]) == 1.0


def test_scale_center_of_fifty_frames():
    gold = np.load(GOLD)
    deform = PolyField(*[gold[f"deform/{i}"] for i in range(4)])
    g = types.SimpleNamespace(get_xyz=dt(gold["xyz"]))
    table = N().update_scale_center(g, deform, total_frames=50, gaussian_ratio=float(gold["gaussian_ratio"]))
    assert g.gaussian_center.shape == (3,) and g.gaussian_scale.shape == (1,) and g.gaussian_center.is_cuda
    W = gold["deform/0"].astype(np.float64)
    ref_table = NR.bbox_table(gold["xyz"], lambda x, t: ((x[:, 0:1] * W[0] + x[:, 1:2] * W[1]) + x[:, 2:3] * W[2]) + t * W[3], 50)
    center, scale = NR.scale_center(ref_table, float(gold["gaussian_ratio"]))
    c, s = g.gaussian_center.cpu().numpy().astype(np.float64), float(g.gaussian_scale[0])
    assert np.abs(table.cpu().numpy() - ref_table).max() <= 1e-6 * np.abs(ref_table).max()
    assert np.abs(c - center).max() <= 1e-6 * np.abs(center).max() and abs(s - scale) <= 1e-6 * scale
    assert np.abs(c - gold["center"]).max() <= 1e-6 * np.abs(gold["center"]).max() and abs(s - float(gold["scale"][0])) <= 1e-6 * scale
    # real=True: the caller's centre and ratio / 2
    N().update_scale_center(g, deform, gaussian_ratio=1.3, gaussian_center=(0.1, -0.2, 0.3), real=True)
    assert g.gaussian_scale.tolist() == [float(np.float32(1.3) / np.float32(2))]
    assert g.gaussian_center.tolist() == [float(np.float32(v)) for v in (0.1, -0.2, 0.3)]


def test_face_areas_against_float64():
    """Bound: with u = 2^-24 and L the face's largest edge, the three subtractions leave each edge component within u |e_k|; a product
    of two such components within 3u |p|; a cross-product component p - q within 3u (|p| + |q|) + u |n_k|, and over the three
    components sum (|p| + |q|)^2 <= 2 L^4 (Cauchy-Schwarz with |e1|, |e2| <= L), so the normal vector is within (3 sqrt 2 + 1) u L^2;
    the sum of squares and the correctly rounded root add 2.5u |n| <= 2.5u L^2; halved: |area32 - area64| <= 3.9 u L^2 <
    4 * 2^-24 L^2 <= 4 ulp(L^2)."""
    rng = np.random.RandomState(3)
    V, F = 5000, 20000
    verts = (rng.randn(V, 3) * np.array([1.0, 0.3, 2.0])).astype(np.float32)
    faces = rng.randint(0, V, (F, 3)).astype(np.int32)
    faces[:50, 2] = faces[:50, 1]                        # degenerate: two equal indices
    sliver = np.arange(60, 200)                          # slivers: the third vertex almost on the edge
    verts[faces[sliver, 2]] = (verts[faces[sliver, 0]] * 0.5 + verts[faces[sliver, 1]] * 0.5 + 1e-6 * rng.randn(len(sliver), 3)).astype(np.float32)
    faces[50:60, 1] = np.arange(V - 30, V - 20)          # degenerate: equal positions (vertices that no other face uses)
    faces[50:60, 0] = np.arange(V - 20, V - 10)
    faces[faces >= V - 30] -= 40
    faces[50:60, 1], faces[50:60, 0] = np.arange(V - 30, V - 20), np.arange(V - 20, V - 10)
    verts[V - 30:V - 20] = verts[V - 20:V - 10]
    faces[200:210, 0] = V                                # out of range
    faces[210:220, 1] = -1
    verts[4999] = np.array([np.nan, 0, 0], np.float32)   # non-finite vertices
    verts[4998] = np.array([np.inf, 0, 0], np.float32)
    faces[220:230, 2], faces[230:240, 0] = 4999, 4998
    assert (NR.face_areas(verts, faces)[:60] == 0).all()
    got = N().face_areas(dt(verts), dt(faces, torch.int32)).cpu().numpy()
    want = NR.face_areas(verts, faces)
    assert got.dtype == np.float32 and (got[200:240] == 0).all() and (got[:60] == 0).all()
    v64 = verts.astype(np.float64)
    ok = ((faces >= 0) & (faces < V)).all(1)
    fs = np.where(ok[:, None], faces, 0)
    with np.errstate(invalid="ignore"):
        tri = v64[fs]
        L2 = np.max([((tri[:, i] - tri[:, j]) ** 2).sum(1) for i, j in ((0, 1), (1, 2), (2, 0))], axis=0)
    fin = ok & np.isfinite(L2)
    err = np.abs(got.astype(np.float64) - want)[fin]
    print("area error / (2^-24 L^2): max", float((err / (2.0 ** -24 * L2[fin] + 1e-300)).max()))
    assert (err <= 4 * 2.0 ** -24 * L2[fin]).all()
    assert (got[~fin] == 0).all()


def test_cumulative_areas_are_monotone_and_reproducible():
    rng = np.random.RandomState(4)
    for F in (1, 15, 16, 17, 4095, 4096, 4097, 300_001):
        a = rng.rand(F).astype(np.float32) ** 4
        a[rng.rand(F) < 0.2] = 0.0
        cum = N().cumulative_areas(dt(a))
        c = cum.cpu().numpy()
        assert c.dtype == np.float64 and (np.diff(c) >= 0).all()
        ref = np.cumsum(a.astype(np.float64))
        assert np.abs(c - ref).max() <= F * 2.0 ** -52 * ref[-1] + 1e-300  # (two fp64 summation orders of F terms)
        assert torch.equal(cum, N().cumulative_areas(dt(a)))


def test_sampling_matches_the_reference_golden():
    gold = np.load(GOLD)
    verts, faces, u = dt(gold["verts"]), dt(gold["faces"], torch.int32), dt(gold["u"])
    P = u.shape[0]
    pts, fidx = N().sample_surface(verts, faces, P, draws=u)
    assert fidx.dtype == torch.int32 and pts.shape == (P, 3)
    # draws whose pick lies within 2^-40 * total of a cumulative boundary are excluded (fp64 sums in another order)
    _, _, margin = NR.sample_surface(gold["verts"], gold["faces"], gold["u"])
    total = NR.face_areas(gold["verts"], gold["faces"]).sum()
    keep = margin > 2.0 ** -40 * total
    print("excluded share on the golden mesh:", float((~keep).mean()))
    assert (~keep).mean() <= 1e-4
    assert np.array_equal(fidx.cpu().numpy()[keep], gold["face_index"][keep])
    box = float(np.ptp(gold["verts"], axis=0).max())
    err = np.abs(pts.cpu().numpy().astype(np.float64) - gold["samples"])[keep].max()
    print("sample error / box:", err / box)
    assert err <= 1e-6 * box
    # the generator path draws exactly torch.rand((count, 3))
    gen = torch.Generator(device=DEV).manual_seed(11)
    a = N().sample_surface(verts, faces, P, generator=gen)
    gen.manual_seed(11)
    ug = torch.rand((P, 3), generator=gen, device=DEV)
    b = N().sample_surface(verts, faces, P, draws=ug)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_sampling_never_chooses_a_face_without_area():
    verts = dt([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 2, 2]])
    faces = dt([[0, 0, 1], [0, 1, 2], [4, 4, 4], [0, 1, 3], [1, 2, 9], [3, 3, 3]], torch.int32)   # areas 0, .5, 0, .5, 0 (bad index), 0
    u = torch.rand((4096, 3), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    u[0, 0], u[1, 0] = 0.0, 1.0 - 2.0 ** -24
    pts, fidx = N().sample_surface(verts, faces, 4096, draws=u)
    assert set(fidx.tolist()) == {1, 3} and int(fidx[0]) == 1 and int(fidx[1]) == 3 and torch.isfinite(pts).all()
    with pytest.raises(RuntimeError, match="no faces"):
        N().sample_surface(verts, faces[:0], 8, draws=u[:8])
    with pytest.raises(RuntimeError, match="total area"):
        N().sample_surface(verts, faces[[0, 2, 4, 5]], 8, draws=u[:8])
    p, f = N().sample_surface(verts, faces[[0, 2, 4, 5]], 8, draws=u[:8], check=False)
    assert (f == -1).all() and torch.isnan(p).all()


def test_chain_from_the_golden_mesh_stage_by_stage():
    """Golden verts -> samples -> anchor.nearest -> normals.  The nearest indices are the golden's exactly.  The golden's normals
    are trimesh's float64 face normals rounded to fp32; the device's are anchor.face_geometry's fp32 ones, so `exactly` is asserted
    for what the chain decides -- every Gaussian gets the normal of exactly the golden's face -- and the values agree to fp32
    rounding (1e-6)."""
    gold = np.load(GOLD)
    A = pkg("anchor")
    verts, faces, u = dt(gold["verts"]), dt(gold["faces"], torch.int32), dt(gold["u"])
    deform = PolyField(*[gold[f"deform/{i}"] for i in range(4)])
    xyz = dt(gold["xyz"])
    xyz_d = xyz + deform.step(xyz, float(gold["t0"]))[0]
    normals, samples, fidx, idx, total = N().normals_from_surface(xyz_d, verts, faces, xyz.shape[0], draws=u)
    assert abs(float(total) - NR.face_areas(gold["verts"], gold["faces"]).sum()) <= 1e-6 * float(total)
    assert np.array_equal(idx.cpu().numpy(), gold["nearest"])
    assert np.array_equal(fidx.cpu().numpy(), gold["face_index"])
    _, fn = A.face_geometry(verts, faces)
    want = fn[dt(gold["face_index"], torch.long)][dt(gold["nearest"], torch.long)]
    assert torch.equal(normals, want)
    assert np.abs(normals.cpu().numpy() - gold["normals"]).max() <= 1e-6


def test_sampling_on_the_bench_mesh():
    """bench.py's mesh-phase surface (DiffMC of the 288^3 field, ~4.7 M faces): every sample lies in the plane of its reported
    triangle and inside it; the face counts follow the area shares (chi-square over 64 area-sorted bins of equal area share, 1e-6
    significance, fixed seed); equal generators give bit-identical runs."""
    import bench
    dev = torch.device(DEV)
    tr, _ = bench.build_scene(dev, 0, 1, "hip", n_frames=2, phase="mesh", dpsr_res=288)
    ms, g = tr.mesh, tr.g
    with torch.no_grad():
        verts, faces = ms.surface(g, ms.psr(g, None, None).contiguous())
    verts = verts.detach().contiguous()
    F = faces.shape[0]
    assert F > 4_500_000
    count = 1_000_000
    gen = torch.Generator(device=DEV).manual_seed(2024)
    pts, fidx = N().sample_surface(verts, faces, count, generator=gen)
    gen.manual_seed(2024)
    pts2, fidx2 = N().sample_surface(verts, faces, count, generator=gen)
    assert torch.equal(pts, pts2) and torch.equal(fidx, fidx2)
    assert int(fidx.min()) >= 0 and int(fidx.max()) < F
    # barycentrics in float64
    tri = verts.double()[faces.long()[fidx.long()]]
    e1, e2, w = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], pts.double() - tri[:, 0]
    d11, d12, d22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    w1, w2 = (w * e1).sum(1), (w * e2).sum(1)
    den = d11 * d22 - d12 * d12
    assert bool((den > 0).all()), "a face without area was chosen"
    b1, b2 = (d22 * w1 - d12 * w2) / den, (d11 * w2 - d12 * w1) / den
    bmin = float(torch.stack([b1, b2, 1 - b1 - b2]).min())
    n = torch.linalg.cross(e1, e2)
    off_plane = ((w * n).sum(1).abs() / n.norm(dim=1))
    edge = torch.sqrt(torch.maximum(d11, d22))
    print("min barycentric", bmin, "max |distance to plane| / edge", float((off_plane / edge).max()))
    assert bmin >= -1e-5
    assert bool((off_plane <= 1e-5 * edge + 1e-6 * verts.abs().max()).all())
    # chi-square: faces sorted by area, 64 bins of (nearly) equal area share
    area = N().face_areas(verts, faces).double()
    order = torch.argsort(area)
    cs = torch.cumsum(area[order], 0)
    total = float(cs[-1])
    bin_of_sorted = torch.clamp((cs / total * 64).long(), max=63)
    share = torch.zeros(64, dtype=torch.float64, device=dev).index_add_(0, bin_of_sorted, area[order]) / total
    bin_of_face = torch.empty(F, dtype=torch.long, device=dev)
    bin_of_face[order] = bin_of_sorted
    obs = torch.bincount(bin_of_face[fidx.long()], minlength=64).double()
    exp = share * count
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    print("chi-square (63 dof):", chi2, "critical", CHI2_63_1E6)
    assert float(exp.min()) > 1000 and chi2 < CHI2_63_1E6
    # share of these draws within 2^-40 * total of a cumulative boundary
    cum = N().cumulative_areas(area.float())
    gen.manual_seed(2024)
    pick = torch.rand((count, 3), generator=gen, device=DEV)[:, 0].double() * cum[-1]
    j = torch.searchsorted(cum, pick).clamp(max=F - 1)
    margin = torch.minimum((cum[j] - pick).abs(), (pick - cum[(j - 1).clamp(min=0)]).abs())
    excluded = float((margin <= 2.0 ** -40 * cum[-1]).double().mean())
    print("excluded-draw share on the bench mesh:", excluded)
    assert excluded <= 1e-4
