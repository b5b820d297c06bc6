"""The deformation network and its inverse as ONE autograd node whose backward pass runs both networks in shared launches
(mlp_hip._MLPPairFunction -> dgm_mlp_backward_group) against the two ordinary nodes it replaces.

The grouped pass keeps the row chunks, the partial tiles and the reduction jobs of the ordinary pass (a workgroup runs two of a
network's chunks one after the other), so its gradients are the ordinary pass's bit for bit -- which also puts them within 2e-5 of
the tensor maximum, the gate tests/test_mlp.py::_fullgrads_check applies to every arithmetic mode, and as close to an fp64
restatement as the ordinary pass is (test_split_arithmetics_are_fp32_gemms's gate).  Where the entry point falls back to two
ordinary passes -- small batches, a time input per row -- it IS them."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import pkg
from test_mlp import build, fragile_rows

T_A, T_B = 0.37, 0.61


def _nets(dev="cuda"):
    """Two DeformNetworkNormal(is_blender) networks with different weights, the second one's heads small like a trained inverse."""
    a = build("DeformNetworkNormal", True, "hip").to(dev)
    D = pkg("deform")
    torch.manual_seed(11)
    b = D.DeformNetworkNormal(is_blender=True, trunk_impl="hip").to(dev)
    return a, b


def _inputs(N, dev="cuda"):
    rng = np.random.RandomState(N % 1000)
    x = torch.tensor(((rng.rand(N, 3) * 2 - 1) * 1.3).astype(np.float32), device=dev)
    gen = torch.Generator(device=dev).manual_seed(N)
    w = [torch.randn(N, 13, device=dev, generator=gen), 0.5 * torch.randn(N, 13, device=dev, generator=gen)]
    return x, w


def _times(N, dev="cuda"):
    return (torch.tensor([[T_A]], device=dev).expand(N, -1), torch.tensor([[T_B]], device=dev).expand(N, -1))


def _grouped(a, b, x, w):
    M = pkg("mlp_hip")
    N = x.shape[0]
    ta, tb = _times(N)
    for p in list(a.parameters()) + list(b.parameters()):
        p.grad = None
    ra, _ = a._time_rows(ta)
    rb, _ = b._time_rows(tb)
    oa, ob = M.network_pair_forward(a, a.head_modules(), b, b.head_modules(), x, ra, rb)
    ((oa * w[0]).sum() + (ob * w[1]).sum()).backward()
    torch.cuda.synchronize()
    return [oa.detach().clone(), ob.detach().clone()], [p.grad.clone() for p in list(a.parameters()) + list(b.parameters())]


def _separate(a, b, x, w):
    N = x.shape[0]
    ta, tb = _times(N)
    for p in list(a.parameters()) + list(b.parameters()):
        p.grad = None
    oa = a.heads_out(x, ta)
    means = (x + oa.detach()[:, :3]).contiguous()
    ob = b.heads_out(means, tb)
    ((oa * w[0]).sum() + (ob * w[1]).sum()).backward()
    torch.cuda.synchronize()
    return [oa.detach().clone(), ob.detach().clone()], [p.grad.clone() for p in list(a.parameters()) + list(b.parameters())]


@functools.lru_cache(maxsize=None)
def _case(N):
    """One grouped and one separate pass per N, shared by the tests below (and left unchanged by them)."""
    a, b = _nets()
    x, w = _inputs(N)
    return a, b, x, w, _grouped(a, b, x, w), _separate(a, b, x, w)


def _names(a, b):
    return ["A." + n for n, _ in a.named_parameters()] + ["B." + n for n, _ in b.named_parameters()]


@pytest.mark.gpu
@pytest.mark.parametrize("N", [32_737, 32_768, 32_769, 33_000, 60_000, 100_003])
def test_grouped_pass_equals_two_separate_passes(N):
    """N = 32 737 and 32 768 (256 CUs; tests/_mlp_plan.py derives them): the smallest paired sizes, 1 024 tiles in 128 chunks of 8,
    every workgroup two full chunks, the last tile one row or full; N = 32 769: 1 025 tiles in 114 chunks of 9, a one-row last tile,
    seven workgroups without a chunk; N = 33 000: a ragged last tile, 1 032 tiles in 115 chunks of 9 over 64 workgroups of two chunks:
    the last six workgroups have one chunk or none; N = 60 000: 1 875 tiles in 125 chunks of 15, one workgroup with one chunk, one
    idle; N = 100 003: the bench's size with a ragged tile."""
    a, b, x, w, (og, gg), (os_, gs) = _case(N)
    for u, v in zip(og, os_):
        assert torch.equal(u, v)  # the forward passes are the same launches on the same numbers
    for name, u, v in zip(_names(a, b), gg, gs):
        assert torch.isfinite(u).all(), name
        err = (u - v).abs().max().item() / (v.abs().max().item() + 1e-300)
        print(f"N={N} {name}: grouped vs separate rel-to-max {err:.2e}")
        assert err < 2e-5, f"{name}: {err:.2e}"
        assert torch.equal(u, v), name  # the same chunks summed in the same order: not merely close
    og2, gg2 = _grouped(a, b, x, w)
    for u, v in zip(og + gg, og2 + gg2):
        assert torch.equal(u, v)  # no atomics, fixed summation order: two grouped runs agree bit for bit


@pytest.mark.gpu
@pytest.mark.parametrize("N", [33_000, 60_000, 100_003])
def test_grouped_pass_is_an_fp32_pass(N):
    """Every gradient tensor of the grouped pass against the PyTorch trunk in fp64 on the same inputs (network B's positions are the
    fp32 sums the pair node forms), each tensor's error relative to the tensor's maximum, gated the way
    test_mlp.test_split_arithmetics_are_fp32_gemms gates the ordinary pass: the worst tensor of the grouped pass at most twice the
    worst tensor of the PyTorch trunk in fp32.  Rows on a ReLU kink of either network carry no output gradient
    (test_mlp.fragile_rows).  Every tensor's figures are printed, the ordinary pass's beside them.
    (Measured: tensor by tensor the bound would not hold for either pass -- their gradients are the same bits: the bias gradients, and the time branch behind them, sit at 2e-6 .. 8e-6 against the
    PyTorch trunk's 3e-7 .. 9e-7 -- they are column sums of the binary16 gradient planes -- while the weight gradients sit at or
    below PyTorch's 2e-6 .. 6e-6.  N = 100 003: worst 7.8e-6 (B.linear.3.bias) against 5.7e-6.)"""
    dev = "cuda"
    a, b = _nets()
    x, w = _inputs(N)
    ta, tb = _times(N)
    ref = [copy.deepcopy(n) for n in (a, b)]
    for n in ref:
        n.trunk_impl = "torch"
    with torch.no_grad():
        means = (x + a.heads_out(x, ta)[:, :3]).contiguous()
        bad = fragile_rows(ref[0], x, ta) | fragile_rows(ref[1], means, tb)
    w = [wi * (~bad)[:, None] for wi in w]
    _, gg = _grouped(a, b, x, w)
    _, gs = _separate(a, b, x, w)  # (reported beside the grouped pass's figures, not gated here)
    res = {}
    for key, dt in (("f32", torch.float32), ("f64", torch.float64)):
        nets = [copy.deepcopy(n).to(dt) for n in ref]
        oa = nets[0].heads_out(x.to(dt), ta.to(dt))
        ob = nets[1].heads_out(means.to(dt), tb.to(dt))
        ((oa * w[0].to(dt)).sum() + (ob * w[1].to(dt)).sum()).backward()
        res[key] = [p.grad.double() for n in nets for p in n.parameters()]
    worst_hip = worst_f32 = 0.0
    for name, g, s_, f32, f64 in zip(_names(a, b), gg, gs, res["f32"], res["f64"]):
        den = f64.abs().max().item() + 1e-300
        e_hip, e_f32 = (g.double() - f64).abs().max().item() / den, (f32 - f64).abs().max().item() / den
        e_sep = (s_.double() - f64).abs().max().item() / den
        print(f"N={N} {name}: rel-to-max error vs fp64: grouped {e_hip:.2e}, separate {e_sep:.2e}, torch fp32 {e_f32:.2e}")
        worst_hip, worst_f32 = max(worst_hip, e_hip), max(worst_f32, e_f32)
    print(f"N={N} worst tensor: grouped {worst_hip:.2e}, torch fp32 {worst_f32:.2e}")
    assert worst_hip < 1e-5
    assert worst_hip < 2 * worst_f32 + 2e-7


@pytest.mark.gpu
@pytest.mark.parametrize("N", [32_737, 32_769, 33_000, 60_000])
def test_grouped_pass_reads_only_what_it_wrote(N):
    """The pattern of test_mlp.test_backward_reads_only_what_the_pass_wrote on the grouped pass: the allocator's cached blocks are
    filled with NaN bit patterns before the pass -- partial tiles of the workgroups without tiles do not exist and must not be
    summed -- and the results are finite and bit-identical to a pass over zeroed blocks."""
    dev = "cuda"
    a, b = _nets()
    x, w = _inputs(N)
    ws_bytes = int(pkg("_lib").lib().dgm_mlp_workspace_bytes(N))

    def one_pass(fill):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        junk = [torch.full((ws_bytes,), fill, dtype=torch.uint8, device=dev) for _ in range(3)]
        junk.append(torch.full((64 << 20,), fill, dtype=torch.uint8, device=dev))
        del junk
        return _grouped(a, b, x, w)

    o0, g0 = one_pass(0)
    o1, g1 = one_pass(255)
    for u, v in zip(o0 + g0, o1 + g1):
        assert torch.isfinite(v).all()
        assert torch.equal(u, v)


def _raw_backward(nets, x, temb, temb_stride, dOut, grouped):
    """Forward of both networks through the C ABI, then the backward pass as one grouped call or two ordinary ones."""
    Lm, M = pkg("_lib"), pkg("mlp_hip")
    lib = Lm.lib()
    N = x.shape[0]
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    st = Lm.stream_ptr()
    jobs, keep, out = [], [], []
    for i, net in enumerate(nets):
        heads = net.head_modules()
        Wh = torch.cat([m.weight.detach() for m in heads], 0).contiguous()
        bh = torch.cat([m.bias.detach() for m in heads], 0).contiguous()
        W = [l.weight.detach().contiguous() for l in net.linear]
        b = [l.bias.detach().contiguous() for l in net.linear]
        p = M._params(None, W, b, Wh, bh, temb[i].shape[1])
        ws = torch.zeros(lib.dgm_mlp_workspace_bytes(N), dtype=torch.uint8, device=x.device)
        o = torch.empty(N, Wh.shape[0], device=x.device)
        Lm.check(lib.dgm_mlp_forward(ctypes.byref(p), N, vp(x), vp(temb[i]), temb_stride, vp(ws), vp(o), st))
        dW, db = [torch.empty_like(t) for t in W], [torch.empty_like(t) for t in b]
        dWh, dbh = torch.empty_like(Wh), torch.empty_like(bh)
        dt = torch.empty(N if temb_stride else 1, temb[i].shape[1], device=x.device)
        j = Lm.MlpBackwardJob()
        j.params, j.dOut, j.workspace = ctypes.pointer(p), dOut[i].data_ptr(), ws.data_ptr()
        for l in range(8):
            j.dW[l], j.db[l] = dW[l].data_ptr(), db[l].data_ptr()
        j.dWh, j.dbh, j.dtemb = dWh.data_ptr(), dbh.data_ptr(), dt.data_ptr()
        jobs.append(j)
        keep.append((p, ws, Wh, bh, W, b))
        out += [o, *dW, *db, dWh, dbh, dt]
    if grouped:
        Lm.check(lib.dgm_mlp_backward_group(ctypes.byref(jobs[0]), ctypes.byref(jobs[1]), N, temb_stride, st))
    else:
        arr = ctypes.c_void_p * 8
        for j in jobs:
            Lm.check(lib.dgm_mlp_backward(j.params, N, ctypes.c_void_p(j.dOut), temb_stride, ctypes.c_void_p(j.workspace),
                                          arr(*j.dW), arr(*j.db), ctypes.c_void_p(j.dWh), ctypes.c_void_p(j.dbh),
                                          ctypes.c_void_p(j.dtemb), st))
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("N,per_row", [pytest.param(4096, False, id="False"), pytest.param(4096, True, id="True"),
                                       pytest.param(32_736, False, id="32736")])
def test_fallback_is_bit_identical_to_two_passes(N, per_row):
    """N = 4 096 is below the paired launches' size, N = 32 736 the largest size below it (256 CUs: 1 023 tiles, four per chunk); a
    time input per row has no folded form: either way the grouped entry point runs two ordinary passes and returns their bits."""
    dev = "cuda"
    a, b = _nets()
    x, w = _inputs(N)
    gen = torch.Generator(device=dev).manual_seed(3)
    rows = N if per_row else 1
    temb = [torch.randn(rows, 30, device=dev, generator=gen) for _ in range(2)]
    stride = 30 if per_row else 0
    one = _raw_backward((a, b), x, temb, stride, w, grouped=True)
    two = _raw_backward((a, b), x, temb, stride, w, grouped=False)
    assert len(one) == len(two) == 2 * 20
    for u, v in zip(one, two):
        assert torch.isfinite(u).all()
        assert torch.equal(u, v)


@pytest.mark.gpu
def test_stage_timer_counts_a_grouped_launch_as_two_layer_passes():
    """bench.py --full prices `mlp_bwd_pair` per network and layer: a grouped launch enters the stage's count twice and shares its
    time, so a backward pass of both networks shows 14 layer passes whether it ran as 7 launches or as 14."""
    Lm = pkg("_lib")
    lib = Lm.lib()
    a, b = _nets()
    x, w = _inputs(33_000)
    counts = {}
    for name, fn in (("grouped", _grouped), ("separate", _separate)):
        fn(a, b, x, w)  # (allocator and code objects primed outside the bracket)
        lib.dgm_set_profiling_sampling(1)
        lib.dgm_set_profiling(2)
        try:
            fn(a, b, x, w)
            ms, n = Lm.collect_stage_ms()["mlp_bwd_pair"]
        finally:
            lib.dgm_set_profiling(0)
        print(f"{name}: mlp_bwd_pair {n} layer passes, {ms * 1e3:.1f} us each")
        counts[name] = n
        assert ms > 0
    assert counts == {"grouped": 14, "separate": 14}


def _adam_state(tr):
    out = []
    for o in tr.optimizers:
        for g in o.param_groups:
            for p in g["params"]:
                s = o.state.get(p, {})
                if "exp_avg" in s:  # (a parameter that never received a gradient has no moments)
                    out += [s["exp_avg"].detach().clone(), s["exp_avg_sq"].detach().clone()]
    return out


@pytest.mark.gpu
def test_trainer_small_scene_is_bit_identical_with_and_without_the_pair_node():
    """cfg1-like (P = 20 000, 400 x 400): below the paired launches' size the grouped entry point runs the ordinary kernels, so
    this isolates the autograd restructuring -- one node for both networks, the inverse network's positions formed inside its
    embedding launch, the cycle loss built behind the render.  Three steps: losses, every parameter and both Adam moments agree
    bit for bit."""
    from test_trainer_dp_gpu import make_trainer, snapshot
    runs = []
    for group in (True, False):
        tr = make_trainer(0, 1, P=20_000, W=400, H=400, group_mlp_backward=group)
        assert tr.group_mlp_backward == group
        it = tr.opt.warm_up + 10
        losses = [tr.step(it + s)[0].clone() for s in range(3)]
        torch.cuda.synchronize()
        runs.append((losses, snapshot(tr), _adam_state(tr)))
    for u, v in zip(runs[0][0] + runs[0][1] + runs[0][2], runs[1][0] + runs[1][1] + runs[1][2]):
        assert torch.equal(u.cpu(), v.cpu())
    assert len(runs[0][2]) > 0


@pytest.mark.gpu
def test_trainer_paired_size_one_step():
    """P = 33 000, 200 x 200, one step's gradients with the pair node (grouped kernels) and without: the loss and the Gaussians'
    gradients are bit-identical (the forward passes and both dOut are), the networks' gradients agree to 2e-5 of the tensor
    maximum."""
    from test_trainer_dp_gpu import make_trainer
    res = []
    for group in (True, False):
        tr = make_trainer(0, 1, P=33_000, W=200, H=200, group_mlp_backward=group)
        it = tr.opt.warm_up + 10
        cam = tr.cameras[0]
        for p in tr.params:
            p.grad = None
        losses, _ = tr.loss_terms(cam, it)
        loss = sum(losses.values())
        loss.backward()
        torch.cuda.synchronize()
        gauss = [p.grad.clone() for p in tr.g.parameters()[:6]]
        nets = [(n, p.grad.clone()) for m, tag in ((tr.deform, "deform."), (tr.deform_back, "deform_back."))
                for n, p in ((tag + k, v) for k, v in m.net.named_parameters())]
        res.append((loss.detach().clone(), gauss, nets))
    assert torch.equal(res[0][0], res[1][0])
    for u, v in zip(res[0][1], res[1][1]):
        assert torch.equal(u, v)
    for (name, u), (_, v) in zip(res[0][2], res[1][2]):
        err = (u - v).abs().max().item() / (v.abs().max().item() + 1e-300)
        print(f"{name}: grouped vs separate rel-to-max {err:.2e}")
        assert torch.isfinite(u).all() and err < 2e-5, f"{name}: {err:.2e}"
        assert torch.equal(u, v), name
