"""dgm_emd_approx (csrc/emd.hip) on the GPU against the dense fp64 restatement of the reference's approxmatch / matchcost kernels
(tests/_emd_ref.py), at every size where the launch structure changes: around the wave, the row tile R, the column tile C and the
smallest size S with a second column part -- all read from the library -- plus multi-part sweeps, n = 2 m and m = 3 n, and a thin
pair whose parts take two column tiles each.

Gate 1 (the project's float parity, README.md "Correctness"): |cost - cost64| <= 1e-4 |cost64| and, for both sides,
|residual - residual64| <= 1e-4 max(n, m).  Every case prints its figures (`EMD_FIG ...`) before it asserts, with the error of the
restatement's own fp32 mode next to the kernel's (gate 2: recorded in DESIGN.md section 4.10, not asserted)."""
import numpy as np
import pytest
import torch

import _emd_ref as ER
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4


def ME():
    return pkg("mesh_eval")


def _tiles():
    t = ME().emd_tiles()
    R, C = t["rows"], t["cols"]
    S = next(s for s in range(1, 1 << 16) if ME().emd_parts(s, s) > 1)
    return R, C, S


# sizes as expressions in R (row tile), C (column tile) and S (the smallest size with a second column part), resolved against the
# library when a case runs, so that collecting the tests needs no library
GRID = [(n, m) for n in ("1", "2", "63", "64", "65", "R-1", "R", "R+1") for m in ("1", "C-1", "C", "C+1")]
# (2048, 1024): n = 2 m, 4 and 8 column parts; (683, 2049): m = 3 n, 9 parts of one tile and 3 parts
SIZES = GRID + [("S-1", "S-1"), ("S", "S"), ("S+1", "S+1"), ("2048", "1024"), ("683", "2049")]


def _resolve(expr):
    R, C, S = _tiles()
    assert S + 1 <= 2100, "S is beyond what the dense reference can hold: test the multi-part path through a parts override"
    return int(eval(expr, {"__builtins__": {}}, {"R": R, "C": C, "S": S}))


def dt(a):
    return torch.tensor(np.asarray(a, np.float32), device=DEV)


def clouds(n, m, radius, seed):
    """A sphere of `radius` against a slightly larger, slightly shifted one."""
    return ER.sphere_cloud(n, radius, seed=seed), ER.sphere_cloud(m, radius * 1.05, (0.02 * radius, 0.0, 0.0), seed=seed + 1000)


def run(a, b, **kw):
    cost, res = ME().emd_approx(dt(a)[None], dt(b)[None], return_residual=True, **kw)
    return float(cost[0]), res[0].double().cpu().numpy()


def check(tag, a, b):
    n, m = len(a), len(b)
    c64, r64 = ER.approx_match_cost(a, b, np.float64)
    c32, r32 = ER.approx_match_cost(a, b, np.float32)
    c, r = run(a, b)
    scale = abs(c64) if c64 != 0 else 1.0
    err, err32 = abs(c - c64) / scale, abs(c32 - c64) / scale
    rerr = max(abs(r[0] - r64[0]), abs(r[1] - r64[1])) / max(n, m)
    rerr32 = max(abs(r32[0] - r64[0]), abs(r32[1] - r64[1])) / max(n, m)
    print(f"EMD_FIG {tag} n={n} m={m} cost64={c64:.9g} cost={c:.9g} rel_err={err:.3e} rel_err_fp32_restatement={err32:.3e} "
          f"ratio={err / err32 if err32 > 0 else float('inf'):.3g} residual64=({r64[0]:.6g}, {r64[1]:.6g}) "
          f"residual_err/max(n,m)={rerr:.3e} fp32_restatement={rerr32:.3e}")
    assert np.isfinite(c) and np.isfinite(r).all()
    assert abs(c - c64) <= TOL * abs(c64), (tag, n, m, c, c64)
    assert abs(r[0] - r64[0]) <= TOL * max(n, m) and abs(r[1] - r64[1]) <= TOL * max(n, m), (tag, n, m, r, r64)


@pytest.mark.parametrize("n, m", SIZES)
def test_emd_matches_fp64_reference(n, m):
    n, m = _resolve(n), _resolve(m)
    if n > 1000:
        assert ME().emd_parts(n, m) > 2 and ME().emd_parts(m, n) > 2  # (the multi-part cases are multi-part)
    for radius in (1.0, 0.3):
        a, b = clouds(n, m, radius, seed=n * 7 + m)
        check(f"sphere{radius}", a, b)


@pytest.mark.parametrize("transposed", [False, True])
def test_emd_parts_of_several_column_tiles(transposed):
    """A part takes more than one column tile only when row tiles x column tiles exceed the target number of workgroups, which no
    size with a dense n x m reference reaches -- except a thin one: 2 points against T + 3 column tiles (T = the target) give one
    row tile, parts of two tiles each and a last part of one, partly filled tile, and the fp64 reference is a 2 x 263 000 matrix.
    As (n, m) the long cloud is the columns of steps 1 and 3, transposed it is the columns of step 2."""
    t = ME().emd_tiles()
    C, T = t["cols"], t["target_blocks"]
    few, many = 2, (T + 2) * C + 44
    tiles, parts = -(-many // C), ME().emd_parts(few, many)
    per = -(-tiles // parts)
    assert tiles == T + 3 and per == 2 and parts * per > tiles  # two tiles per part, the last part shorter
    a = ER.sphere_cloud(few, 1.0, seed=8)
    b = ER.sphere_cloud(many, 1.05, (0.02, 0.0, 0.0), seed=9)
    for radius in (1.0, 0.3):
        x, y = a * np.float32(radius), b * np.float32(radius)
        check(f"thin{radius}" + ("T" if transposed else ""), *((y, x) if transposed else (x, y)))


def test_emd_clouds_far_apart_keep_their_mass():
    """Two clouds 5 apart: W underflows at all but the last levels, and some percent of the mass is never moved -- a residual
    a hundred times that of the near clouds, which the kernel has to reproduce."""
    R, C, S = _tiles()
    a = ER.sphere_cloud(S + 43, 0.3, seed=1)
    b = ER.sphere_cloud(S + 43, 0.3, (5.0, 0.0, 0.0), seed=2)
    _, r64 = ER.approx_match_cost(a, b)
    assert r64[0] > 0.01 * len(a)
    check("apart5", a, b)


def test_emd_identical_clouds_and_single_points():
    a = ER.sphere_cloud(300, 1.0, seed=3)
    check("identical", a, a.copy())
    c, r = run(np.zeros((1, 3)), np.array([[0.01, 0.0, 0.0]]))
    assert abs(c - 0.01) <= TOL * 0.01 and abs(r[0]) <= TOL and abs(r[1]) <= TOL
    c, r = run(np.ones((1, 3)), np.ones((1, 3)))
    assert c == 0.0
    # the integer-division quirk: n = 3, m = 2 leaves one unit on the left
    c, r = run(ER.sphere_cloud(3, 0.05, seed=4), ER.sphere_cloud(2, 0.05, seed=5))
    assert abs(r[0] - 1.0) <= 3 * TOL and abs(r[1]) <= 3 * TOL


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_emd_batch_equals_single_calls_bit_for_bit():
    R, C, S = _tiles()
    n, m = S + 60, 2 * C + 5
    A = np.stack([ER.sphere_cloud(n, r, seed=10 + i) for i, r in enumerate((1.0, 0.3, 2.0))])
    B = np.stack([ER.sphere_cloud(m, r * 1.1, (0.05, 0.0, 0.0), seed=20 + i) for i, r in enumerate((1.0, 0.3, 2.0))])
    cost, res = ME().emd_approx(dt(A), dt(B), return_residual=True)
    assert cost.shape == (3,) and res.shape == (3, 2)
    assert len(set(cost.tolist())) == 3
    for i in range(3):
        c1, r1 = ME().emd_approx(dt(A[i:i + 1]), dt(B[i:i + 1]), return_residual=True)
        assert torch.equal(_bits(c1), _bits(cost[i:i + 1])) and torch.equal(_bits(r1), _bits(res[i:i + 1]))
    assert torch.equal(_bits(ME().emd_approx(dt(A), dt(B))), _bits(cost))  # (without the residual)


def test_emd_is_reproducible_and_ignores_scratch_contents():
    n, m = 2048, 1024
    a, b = clouds(n, m, 1.0, seed=5)
    ta, tb = dt(a)[None], dt(b)[None]
    c0, r0 = ME().emd_approx(ta, tb, return_residual=True)
    c1, r1 = ME().emd_approx(ta, tb, return_residual=True)
    assert torch.equal(_bits(c0), _bits(c1)) and torch.equal(_bits(r0), _bits(r1))
    need = int(pkg("_lib").lib().dgm_emd_scratch_floats(1, n, m))
    scratch = torch.full((need + 7,), float("nan"), device=DEV)
    c2, r2 = ME().emd_approx(ta, tb, return_residual=True, scratch=scratch)
    assert torch.equal(_bits(c0), _bits(c2)) and torch.equal(_bits(r0), _bits(r2))
    assert torch.isnan(scratch[need:]).all()  # nothing is written behind the size the library asked for
    with pytest.raises(ValueError, match="scratch"):
        ME().emd_approx(ta, tb, scratch=scratch[:need - 1])


def test_emd_wrapper_rejects_bad_arguments():
    a = torch.zeros((1, 8, 3), device=DEV)
    with pytest.raises(RuntimeError, match="float32"):
        ME().emd_approx(a.double(), a)
    with pytest.raises(ValueError, match="expected"):
        ME().emd_approx(a[0], a)
    with pytest.raises(ValueError, match="expected"):
        ME().emd_approx(a[:, :0], a)
    with pytest.raises(ValueError, match="batch"):
        ME().emd_approx(torch.zeros((2, 8, 3), device=DEV), a)
    with pytest.raises(ValueError, match="one size"):
        ME().emd_cd(a, torch.zeros((1, 9, 3), device=DEV))
