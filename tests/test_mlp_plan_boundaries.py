"""The MLP at every batch size where the host cuts a batch differently, against fp64.

csrc/mlp.hip decides on the host (p4_plan, bwd_plan, group_split) how N rows become 32-row tiles, weight-gradient chunks,
workgroups and partial tiles, and that cutting changes shape at a handful of sizes (tests/_mlp_plan.py restates it and derives the
sizes; DESIGN 4.1b has the table).  Every one of those sizes, both sides of every line, runs here: the HIP trunk of
DeformNetworkNormal(is_blender) against the PyTorch trunk in fp32 and a deep copy in fp64 on the same inputs -- outputs, every
parameter gradient (the time branch's included) and dL/dx, each relative to its tensor's maximum in fp64, rows on a ReLU kink
weighted out (test_mlp.fragile_rows).

Two output gradients per size.  DENSE: randn on every kept row.  LAST TILE ONLY: non-zero on the rows of the last 32-row tile
alone -- every other tile's output gradient is all zero, what a block of culled Gaussians produces -- so that the expected weight
gradients come from the tail rows alone: a plan that loses the last tile of a ragged chunk, lets padding rows in or sums a partial
tile nobody wrote is off by the whole tensor.

Gates, the ones tests/test_mlp.py applies to the same quantities: (a) every tensor within 1e-5 of its maximum against fp64, at
every size; (b) the worst tensor at most twice the worst tensor of the PyTorch trunk in fp32, + 2e-7, from N = 4 096 up (where
test_split_arithmetics_are_fp32_gemms has shown it to hold; below, PyTorch's sums are short and its error can fall under the plane
format's floor: printed, not gated).  Both figures are printed per case."""
import copy
import ctypes
import functools
import time

import pytest
import torch

import _mlp_plan as P
from conftest import pkg
from test_mlp import build, fragile_rows, gemm_mode  # noqa: F401  (gemm_mode: the fixture)
from test_mlp_group import _grouped, _inputs, _nets, _separate

T_VAL = 0.37
GATE_B_FROM = 4096
# N -> RandomState seed of the positions where N % 1000 (test_mlp_group._inputs) puts the one row of the last tile on a ReLU kink:
# two sizes of the 304-CU sweep, none of the 64- or 256-CU ones (test_inputs_keep_most_rows_and_a_row_of_the_last_tile checks all)
SEEDS = {9729: 1729, 19457: 2457}
ISSUE_SIZES_256 = [1, 31, 32, 33, 2016, 2017, 8160, 8192, 8193, 16384, 16385, 24576, 24577, 32736, 32737, 32768, 32769]
HOST_CUS = (256, 304, 64)


def _device_cus():
    """What num_cus() of csrc/mlp.hip reads: the device's CU count, 256 without a device."""
    if torch.cuda.is_available():
        return torch.cuda.get_device_properties(0).multi_processor_count
    return 256


CUS = _device_cus()
SWEEP = P.sweep(CUS)


def _first(cls, cus=CUS):
    return next((n for n in P.sweep(cus) if P.plan_class(n, cus) == cls), None)


def _last(cls, cus=CUS):
    return next((n for n in reversed(P.sweep(cus)) if P.plan_class(n, cus) == cls), None)


def _reduced(cus=CUS):
    """The other plane forms' list: two tiles with a one-row tail, chunks = CUs, the first ragged chunk, the last unpaired size, the
    first paired one (a one-row last tile), the first with idle weight-gradient workgroups.  256 CUs: 33, 8192, 8193, 32736,
    32737, 32769."""
    picks = [P.TILE + 1, _last("B", cus), _first("C", cus), _last("C", cus), _first("D", cus), _first("E", cus)]
    return [n for n in picks if n is not None]


F32_SIZES = [63, 64, 65, 511, 512, 513, 8193]  # GM = 64 rows per GEMM tile, DW_ROWS = 512, HD_ROWS = 256 (top of csrc/mlp.hip)
PER_ROW_SIZES = [n for n in (P.TILE + 1, _first("C"), _first("E")) if n is not None]  # 256 CUs: 33, 8193, 32769


def _positions(N, dev):
    if N in SEEDS:
        import numpy as np
        rng = np.random.RandomState(SEEDS[N])
        return torch.tensor(((rng.rand(N, 3) * 2 - 1) * 1.3).astype("float32"), device=dev)
    return _inputs(N, dev)[0]


def _keep(ref, x, t):
    with torch.no_grad():
        return ~fragile_rows(ref, x, t)


# ---- host: the sizes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", HOST_CUS)
def test_sweep_covers_every_class_and_both_sides_of_every_boundary(cus):
    sweep = P.sweep(cus)
    assert {P.plan_class(n, cus) for n in sweep} == set(P.classes(cus)) == set("ABCDE")
    # every N up to the first size of class E, one by one: wherever the class or the tiles per chunk change between N and N + 1,
    # both are in the sweep, and so is each class's multiple of 32 next to the line
    top = P.TILE * P.PAIR_MIN_TILES * cus + 1
    assert P.plan_class(top, cus) == "E" and P.plan_class(top - 1, cus) == "D"
    kind = lambda n: (P.plan_class(n, cus), P.plan(n, cus).tiles_per_chunk)
    lines = [n for n in range(1, top) if kind(n) != kind(n + 1)]
    assert len(lines) >= 6  # A|B, B|C, 2|3, 3|4 tiles per chunk, C|D, D|E
    for n in lines:
        assert n in sweep and n + 1 in sweep, (cus, n)
        assert n % P.TILE == 0  # the line's multiple of 32 is its lower side
    for cls in "BD":  # one tile count each: the one-row last tile and the full one
        assert _last(cls, cus) - _first(cls, cus) == P.TILE - 1 and _last(cls, cus) % P.TILE == 0
    for n in sweep:  # the plan's own invariants at every size chosen
        p = P.plan(n, cus)
        assert (p.chunks - 1) * p.tiles_per_chunk < p.nt <= p.chunks * p.tiles_per_chunk and p.chunks <= p.gx <= cus
        if p.n_dw > 0:
            assert (p.chunks_pair - 1) * p.tpc_pair < p.nt <= p.chunks_pair * p.tpc_pair and p.chunks_pair <= p.n_dw <= p.chunks
            assert p.n_wg > 0  # with the default share, what pairs also groups


def test_no_pairing_below_64_cus():
    assert P.classes(32) == "ABC" and {P.plan_class(n, 32) for n in P.sweep(32)} == set("ABC")
    assert all(P.plan(n, 32).n_dw == 0 and P.plan(n, 32).n_wg == 0 for n in P.sweep(32) + [10 ** 6])


def test_the_sweep_of_256_cus():
    sweep = P.sweep(256)
    assert set(ISSUE_SIZES_256) <= set(sweep)
    assert len(sweep) <= len(ISSUE_SIZES_256) + 2  # (derived, not padded: 8 161, the first size of class B, is the one extra)
    got = {n: P.plan(n, 256) for n in sweep}
    assert [P.plan_class(n, 256) for n in (8160, 8161, 8192, 8193, 32736, 32737, 32768, 32769)] == list("ABBCCDDE")
    assert [(got[n].nt, got[n].chunks) for n in (8193, 16385, 24577)] == [(257, 129), (513, 171), (769, 193)]
    d = got[32737]
    assert d == got[32768] and (d.n_dw, d.tpc_pair, d.chunks_pair, d.n_wg, d.chunked) == (128, 8, 128, 64, 1)
    e = got[32769]
    assert (e.nt, e.tpc_pair, e.chunks_pair, e.n_dw - e.chunks_pair) == (1025, 9, 114, 14)
    assert _reduced(256) == [33, 8192, 8193, 32736, 32737, 32769]
    assert P.plan(33_000, 256).n_dw > 0 and P.plan(20_000, 256).n_dw == 0  # (what the older tests run)


@pytest.mark.parametrize("N", sorted(set(SWEEP + F32_SIZES)))
def test_workspace_partial_blocks_are_the_plans_chunks(N):
    """dgm_mlp_describe_workspace reports where each layer's weight-gradient partial tiles and bias-gradient partial rows start;
    the blocks lie back to back (carve(): partial_l[0], partial_db_l[0], partial_l[1], ...), so their lengths are differences:
    chunks x Kp x 256 floats and chunks x 8 x 256 floats.  The skip layer's blocks also serve the fp32-MFMA path and are left out."""
    lib = pkg("_lib").lib()
    offs = (ctypes.c_size_t * 64)()
    assert lib.dgm_mlp_describe_workspace(N, offs, 64) == 49
    part, part_db = list(offs)[33:41], list(offs)[41:49]
    chunks = P.plan(N, CUS).chunks
    for l in (0, 1, 2, 3, 4, 6, 7):
        assert part_db[l] - part[l] == chunks * (96 if l == 0 else 256) * 256 * 4, (N, l)
        if l < 7:
            assert part[l + 1] - part_db[l] == chunks * 8 * 256 * 4, (N, l)
    assert part_db[5] - part[5] >= chunks * 352 * 256 * 4 and part[6] - part_db[5] >= chunks * 8 * 256 * 4


@functools.lru_cache(maxsize=None)
def _host_net():
    return build("DeformNetworkNormal", True, "torch")


@pytest.mark.parametrize("N", sorted({n for cus in HOST_CUS for n in P.sweep(cus)} | set(F32_SIZES)))
def test_inputs_keep_most_rows_and_a_row_of_the_last_tile(N):
    """The inputs of the device tests below, on the host with the fp64 PyTorch trunk alone: fragile_rows weights out at most a
    quarter of the rows (15-19 % measured), and at least one row of the last tile keeps its weight -- else the last-tile pattern
    would be all zero and prove nothing."""
    x = _positions(N, "cpu")
    t = torch.tensor([[T_VAL]]).expand(N, -1)
    keep = _keep(_host_net(), x, t)
    share = 1.0 - keep.float().mean().item()
    tail = int(keep[P.TILE * (P.plan(N).nt - 1):].sum())
    print(f"N={N}: {share:.1%} of the rows on a ReLU kink, {tail} of the last tile's {N - P.TILE * (P.plan(N).nt - 1)} rows kept")
    assert share <= 0.25
    assert tail >= 1


# ---- device: the labels -----------------------------------------------------------------------------------------------------------
def _stage_counts(fn, a, b, x, w):
    Lm = pkg("_lib")
    lib = Lm.lib()
    fn(a, b, x, w)  # (allocator and code objects primed outside the bracket)
    lib.dgm_set_profiling_sampling(1)
    lib.dgm_set_profiling(2)
    try:
        fn(a, b, x, w)
        got = Lm.collect_stage_ms()
    finally:
        lib.dgm_set_profiling(0)
    return {k: got[k][1] for k in ("mlp_bwd_pair", "mlp_layer_bwd", "mlp_layer_dw")}


@pytest.mark.gpu
def test_stage_timer_sees_paired_launches_exactly_where_the_plan_pairs():
    """What keeps tests/_mlp_plan.py honest on the real chip.  backward_planes() brackets a paired launch as `mlp_bwd_pair` and,
    where nothing pairs, the backward-data GEMM and the weight gradient of a layer as `mlp_layer_bwd` and `mlp_layer_dw`: layers
    7 .. 1, seven of each per network and none of the other kind.  Both networks, grouped entry point and two ordinary passes."""
    if "D" not in P.classes(CUS):
        pytest.skip(f"no paired launches below {P.PAIR_MIN_GX} CUs (this device has {CUS})")
    a, b = _nets()
    sizes = [_last("C"), _first("D"), _last("D"), _first("E")]  # 256 CUs: 32 736, 32 737, 32 768, 32 769
    assert [P.plan(n, CUS).n_dw > 0 for n in sizes] == [False, True, True, True]
    for N in sizes:
        x, w = _inputs(N)
        for name, fn in (("grouped", _grouped), ("separate", _separate)):
            got = _stage_counts(fn, a, b, x, w)
            print(f"N={N} ({P.label(N, CUS)}) {name}: {got}")
            want = {"mlp_bwd_pair": 14, "mlp_layer_bwd": 0, "mlp_layer_dw": 0} if P.plan(N, CUS).n_dw > 0 else \
                   {"mlp_bwd_pair": 0, "mlp_layer_bwd": 14, "mlp_layer_dw": 14}
            assert got == want, (N, name)


# ---- device: one network against fp64 ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def _module_wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\n[test_mlp_plan_boundaries] module wall time {time.perf_counter() - t0:.1f} s")


@functools.lru_cache(maxsize=None)
def _device_nets():
    ref = build("DeformNetworkNormal", True, "torch").to("cuda")
    hip = build("DeformNetworkNormal", True, "hip").to("cuda")
    return ref, hip, copy.deepcopy(ref).double()


def _pass(net, x0, t, w, dt, with_dx):
    """[(name, tensor in fp64)]: outputs, dL/dx if asked for, every parameter gradient."""
    for p in net.parameters():
        p.grad = None
    x = x0.to(dt).clone().requires_grad_(with_dx)
    out = torch.cat(net(x, t.to(dt)), -1)
    (out * w.to(dt)).sum().backward()
    torch.cuda.synchronize()
    res = [("out", out.detach().double())] + ([("dL/dx", x.grad.double())] if with_dx else [])
    return res + [(n, p.grad.double().clone()) for n, p in net.named_parameters()]


@functools.lru_cache(maxsize=None)
def _reference(N, pattern, per_row, with_dx):
    """Inputs, and the PyTorch trunk's results in fp32 and fp64: computed once per case, shared by every arithmetic, never changed."""
    dev = "cuda"
    ref, _, r64 = _device_nets()
    x = _positions(N, dev)
    t = torch.full((N, 1), T_VAL, device=dev) if per_row else torch.tensor([[T_VAL]], device=dev).expand(N, -1)
    w = _inputs(N, dev)[1][0] * _keep(ref, x, t)[:, None]
    if pattern == "tail":
        w = w * (torch.arange(N, device=dev) >= P.TILE * (P.plan(N).nt - 1))[:, None]
        assert int((w != 0).any(1).sum()) >= 1
    return x, t, w, _pass(ref, x, t, w, torch.float32, with_dx), _pass(r64, x, t, w, torch.float64, with_dx)


def _check(N, pattern, tag, per_row=False, with_dx=True):
    x, t, w, f32, f64 = _reference(N, pattern, per_row, with_dx)
    hip = _pass(_device_nets()[1], x, t, w, torch.float32, with_dx)
    assert [n for n, _ in hip] == [n for n, _ in f64] and "timenet.0.weight" in dict(hip)
    worst = {"hip": (0.0, ""), "f32": (0.0, "")}
    over = []
    for (name, h), (_, s), (_, d) in zip(hip, f32, f64):
        assert torch.isfinite(h).all(), name
        den = d.abs().max().item()
        assert den > 0, name  # (an all-zero expectation would pass anything)
        e_hip, e_f32 = (h - d).abs().max().item() / den, (s - d).abs().max().item() / den
        worst["hip"], worst["f32"] = max(worst["hip"], (e_hip, name)), max(worst["f32"], (e_f32, name))
        if not e_hip < 1e-5:
            over.append(f"{name}: {e_hip:.2e}")
    bound = 2 * worst["f32"][0] + 2e-7
    print(f"[{tag}, {pattern}] N={N} ({P.label(N, CUS)}): worst rel-to-max error vs fp64: hip {worst['hip'][0]:.2e} "
          f"({worst['hip'][1]}), torch fp32 {worst['f32'][0]:.2e} ({worst['f32'][1]}); gate (b) {bound:.2e}"
          f"{'' if N >= GATE_B_FROM else ' (printed, not gated below N = 4 096)'}")
    assert not over, f"gate (a), 1e-5 of the tensor's maximum: {over}"
    if N >= GATE_B_FROM:
        assert worst["hip"][0] <= bound, f"gate (b): {worst['hip'][1]} {worst['hip'][0]:.2e} > {bound:.2e}"


# the unpaired classes come first (the sweep ascends): a fault names its class
@pytest.mark.gpu
@pytest.mark.parametrize("N,pattern", [(n, pat) for n in SWEEP for pat in ("dense", "tail")])
def test_default_arithmetic_at_every_boundary(N, pattern):
    """f16x3p on round 6's forms (one time row: forward_folded, backward_planes<true>), with dL/dx."""
    _check(N, pattern, "f16x3p")


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["dense", "tail"])
@pytest.mark.parametrize("N", _reduced())
@pytest.mark.parametrize("gemm_mode", ["f16x3p5", "f16x3p8"], indirect=True)
def test_other_plane_forms_at_the_class_lines(N, pattern, gemm_mode):
    """One wave per SIMD in every 256-wide GEMM (f16x3p5), and rounds 3-5's forms (f16x3p8: backward_planes<false>, the 96-column
    embedding rows): the same plan, other kernels on its chunks."""
    _check(N, pattern, gemm_mode)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["dense", "tail"])
@pytest.mark.parametrize("N", F32_SIZES)
@pytest.mark.parametrize("gemm_mode", ["f32"], indirect=True)
def test_fp32_mfma_mode_at_its_own_constants(N, pattern, gemm_mode):
    """The native-fp32 mode cuts by GM = 64 rows per GEMM tile, DW_ROWS = 512 per weight-gradient chunk and HD_ROWS = 256 per
    heads chunk, not by the plan; dL/dx exists in the plane arithmetic only (test_plane_format_on_adversarial_statistics)."""
    _check(N, pattern, gemm_mode, with_dx=False)


@pytest.mark.gpu
@pytest.mark.parametrize("N", PER_ROW_SIZES)
def test_a_time_value_per_row_at_the_class_lines(N):
    """No broadcast row: forward_per_row and backward_planes<false> with dL/dt_emb per row behind the time branch; dense only,
    no dL/dx (the plane path differentiates the positions with a broadcast time row only)."""
    _check(N, "dense", "f16x3p per-row t", per_row=True, with_dx=False)
