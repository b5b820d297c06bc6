"""The reduce role of the grouped paired launches (mlp_planes.hpp: pair_reduce_role; dgm_mlp_set_reduce_in_pair): workgroups of the
paired launch of layer l that have finished their own share sum the first `cap` pieces of layer l + 1's weight-gradient partial
tiles, the pass's final reduction launch sums the rest.  A piece is one device function whoever runs it, so every gradient has the
same bits at every cap; which workgroup takes which piece differs from run to run and must not show either."""
import ctypes
import functools

import pytest
import torch

from conftest import pkg
from test_mlp_group import _inputs, _nets, _raw_backward

NBLOCKS = 256  # pieces of a K = 256 reduction job: (256 / 4) x (256 / 64)
T_DIM = 30
NAN_BYTE = 255  # 0xffffffff: a NaN as a float, a ticket counter far past its end as an unsigned


class _Pass:
    """Both networks' forward passes through the C ABI, once, on workspaces of their own (filled with `fill` bytes before the
    forward: a workspace has no initial state); run() is then one grouped backward pass on them at a given cap."""

    def __init__(self, N, fill=0):
        Lm, M = pkg("_lib"), pkg("mlp_hip")
        self.Lm, self.lib, self.N = Lm, Lm.lib(), N
        lib, dev = self.lib, "cuda"
        a, b = _nets()
        x, dOut = _inputs(N)
        gen = torch.Generator(device=dev).manual_seed(5)
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        offs = (ctypes.c_size_t * 64)()
        assert lib.dgm_mlp_describe_workspace(N, offs, 64) == 49
        o = list(offs)
        part, part_db = o[33:41], o[41:49]  # (emb, Y x 8, mask x 8, Ga, Gb, Eexp, Yexp x 8, Dexp, Gexp x 2, Cin, Dp come first)
        # the sixteen buffers lie back to back (tiles and bias rows of layer 0, of layer 1, ...): one ends where the next begins, and
        # the last, layer 7's bias rows, is as long as layer 0's (the same formula for every layer but 5)
        starts = sorted(part + part_db)
        assert starts[0] == part[0] and starts[1] == part_db[0] and starts[-1] == part_db[7]
        self.regions = list(zip(starts[:-1], starts[1:])) + [(part_db[7], part_db[7] + (part[1] - part_db[0]))]
        assert self.regions[-1][1] <= lib.dgm_mlp_workspace_bytes(N)
        self.jobs, self.keep, self.grads, self.ws = [], [], [], []
        for i, net in enumerate((a, b)):
            heads = net.head_modules()
            Wh = torch.cat([m.weight.detach() for m in heads], 0).contiguous()
            bh = torch.cat([m.bias.detach() for m in heads], 0).contiguous()
            W = [l.weight.detach().contiguous() for l in net.linear]
            bs = [l.bias.detach().contiguous() for l in net.linear]
            temb = torch.randn(1, T_DIM, device=dev, generator=gen)
            p = M._params(None, W, bs, Wh, bh, T_DIM)
            ws = torch.full((lib.dgm_mlp_workspace_bytes(N),), fill, dtype=torch.uint8, device=dev)
            out = torch.empty(N, Wh.shape[0], device=dev)
            Lm.check(lib.dgm_mlp_forward(ctypes.byref(p), N, vp(x), vp(temb), 0, vp(ws), vp(out), Lm.stream_ptr()))
            dW, db = [torch.empty_like(t) for t in W], [torch.empty_like(t) for t in bs]
            dWh, dbh, dt = torch.empty_like(Wh), torch.empty_like(bh), torch.empty(1, T_DIM, device=dev)
            j = Lm.MlpBackwardJob()
            j.params, j.dOut, j.workspace = ctypes.pointer(p), dOut[i].data_ptr(), ws.data_ptr()
            for l in range(8):
                j.dW[l], j.db[l] = dW[l].data_ptr(), db[l].data_ptr()
            j.dWh, j.dbh, j.dtemb = dWh.data_ptr(), dbh.data_ptr(), dt.data_ptr()
            self.jobs.append(j)
            self.keep.append((p, x, dOut, temb, out, Wh, bh, W, bs))
            self.grads += [*dW, *db, dWh, dbh, dt]
            self.ws.append(ws)
        torch.cuda.synchronize()

    def run(self, cap, poison=False):
        """-> clones of 2 x (8 dW, 8 db, dWh, dbh, dtemb).  poison: NaN patterns in every partial-tile buffer and every output first."""
        if poison:
            for ws in self.ws:
                for s, e in self.regions:
                    ws[s:e].fill_(NAN_BYTE)
            for g in self.grads:
                g.fill_(float("nan"))
        prev = self.lib.dgm_mlp_set_reduce_in_pair(cap)
        try:
            assert self.lib.dgm_mlp_set_reduce_in_pair(-1) == cap  # (a query: no change)
            self.Lm.check(self.lib.dgm_mlp_backward_group(ctypes.byref(self.jobs[0]), ctypes.byref(self.jobs[1]), self.N, 0,
                                                          self.Lm.stream_ptr()))
            torch.cuda.synchronize()
        finally:
            self.lib.dgm_mlp_set_reduce_in_pair(prev)
        return [g.clone() for g in self.grads]


@functools.lru_cache(maxsize=None)
def _case(N):
    """One set of forward passes per N and its gradients with the role off -- the launches of before --, shared by the tests below."""
    ps = _Pass(N)
    return ps, ps.run(0)


def _same(got, ref):
    assert len(got) == len(ref) == 2 * 19
    for i, (u, v) in enumerate(zip(got, ref)):
        assert torch.isfinite(u).all(), i
        assert torch.equal(u, v), i


@pytest.mark.gpu
@pytest.mark.parametrize("N", [33_000, 60_000])
def test_gradients_are_bit_identical_at_every_cap(N):
    """N = 33 000: the smallest paired size, 115 chunks of 9 tiles, six workgroups per network with one chunk or none; N = 60 000:
    125 chunks, one workgroup with one chunk, one idle.  Caps 0 (role off), 1, all but one piece, all: sixteen dW, sixteen db, both
    dWh / dbh and both dtemb are the same bits."""
    ps, ref = _case(N)
    for u in ref:
        assert torch.isfinite(u).all()
    for cap in (1, NBLOCKS - 1, NBLOCKS):
        _same(ps.run(cap), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [33_000, 60_000])
def test_passes_in_a_row_and_changing_caps_agree(N):
    """Three passes at the full cap on the same workspaces, then the cap changes between passes: which workgroup draws which ticket
    differs from pass to pass, the gradients do not -- and every pass finds its ticket counters armed."""
    ps, ref = _case(N)
    for cap in (NBLOCKS, NBLOCKS, NBLOCKS, 7, NBLOCKS, 0, NBLOCKS // 2, 10 * NBLOCKS):  # (above a job's piece count = all of it)
        _same(ps.run(cap), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [33_000, 60_000])
def test_no_poisoned_tile_reaches_a_gradient(N):
    """The pattern of test_mlp_group.test_grouped_pass_reads_only_what_it_wrote with the role on: workspaces that were all-ones bytes
    before the forward pass (the ticket counters included), then NaN patterns in every partial-tile buffer and every gradient
    output before each backward pass.  A piece reduced before its tiles were written, a tile of a workgroup without chunks, or a
    piece nobody reduced would leave a NaN; the results are the clean pass's bits."""
    _, ref = _case(N)
    ps = _Pass(N, fill=NAN_BYTE)
    for cap in (NBLOCKS, NBLOCKS // 4, NBLOCKS):
        _same(ps.run(cap, poison=True), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("per_row", [False, True])
def test_fallback_runs_two_ordinary_passes_whatever_the_switch_says(per_row):
    """N = 4 096 is below the paired launches' size and a time input per row has no grouped form: the grouped entry point is two
    ordinary passes with the role on as with it off."""
    dev = "cuda"
    N = 4096
    lib = pkg("_lib").lib()
    a, b = _nets()
    x, w = _inputs(N)
    gen = torch.Generator(device=dev).manual_seed(3)
    temb = [torch.randn(N if per_row else 1, T_DIM, device=dev, generator=gen) for _ in range(2)]
    stride = T_DIM if per_row else 0
    two = _raw_backward((a, b), x, temb, stride, w, grouped=False)
    prev = lib.dgm_mlp_set_reduce_in_pair(-1)
    try:
        for cap in (NBLOCKS, 0):
            lib.dgm_mlp_set_reduce_in_pair(cap)
            one = _raw_backward((a, b), x, temb, stride, w, grouped=True)
            assert len(one) == len(two) == 2 * 20
            for u, v in zip(one, two):
                assert torch.isfinite(u).all()
                assert torch.equal(u, v)
    finally:
        lib.dgm_mlp_set_reduce_in_pair(prev)
