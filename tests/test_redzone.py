"""Red-zone tests: no kernel writes or reads outside its stated buffers ("Memory contracts").

Every case runs a public wrapper three times on the same inputs: (a) plain tensors; (b) inputs placed at their exact size between
guard zones and every tensor the wrapper allocates (outputs and scratch) handed out by tests/_redzone.py at exactly the requested
size, bodies pre-filled with 0xFF; (c) the same with 0x00 bodies.  Asserted:
  writes stay inside     after (b) and (c) every guard of every buffer holds its pattern;
  reads stay inside      the outputs of (b) equal those of (a): just outside every input sits NaN / -1;
  no hidden state        the outputs of (c) equal those of (b);
  the case is covered    an allocation of exactly L.dgm_*_bytes(...) was seen inside the wrapper ("not covered" otherwise);
  alignment as stated    (d) as (b) with the wrapper's flat byte scratch 16 bytes off the 256-byte grid gives the outputs of (b).
Outputs are compared byte for byte, except where the header documents sums by fp32 atomics; there the tolerance is the one the
module's own GPU test uses (TOL_*, each with its source).  Sizes: 1 (or the documented minimum) and one below / at / above the
partition constants named at the top of the module's .hip file.  Nothing here hands a kernel a buffer smaller than the library asks
for."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from _redzone import RedZone
from conftest import ROOT, pkg, raster_args

pytestmark = pytest.mark.gpu
DEV = "cuda"

# tolerances of the modules that sum with fp32 atomics, relative to the reference tensor's largest magnitude unless they say "abs"
TOL_DPSR_SPLAT = 1e-5     # tests/test_dpsr.py:29   (the rasterised normal field)
TOL_DPSR_GRAD = 2e-4      # tests/test_dpsr.py:4, 33-37
TOL_LAPLACE = 1e-5        # tests/test_dpsr.py:106-108
TOL_TRI_DPOS = 1e-3       # tests/test_mesh_raster.py:367, 379
TOL_TRI_DATTR = 1e-5      # tests/test_mesh_raster.py:366
TOL_VNORMALS_ABS = 1e-6   # tests/test_visualize.py:46-55 (absolute: unit vectors)

COVERED = set()  # size functions whose coverage assertion passed in a green case


def L():
    return pkg("_lib").lib()


def rng(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape):
    return torch.randn(shape, generator=g).to(DEV)


def rand(g, *shape):
    return torch.rand(shape, generator=g).to(DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def plain_at(x, offset):
    """A copy of x that starts offset bytes behind an allocation's (512-byte aligned) start."""
    if not offset:
        return x.detach().clone()
    n = x.numel() * x.element_size()
    buf = torch.empty(n + offset, dtype=torch.uint8, device=x.device)
    out = buf[offset:offset + n].view(x.dtype).view(x.shape)
    out.copy_(x.detach())
    return out


def same_bytes(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.dtype}{tuple(a.shape)} against {b.dtype}{tuple(b.shape)}"
    if a.numel() == 0:
        return
    flat = lambda t: t.detach().clone(memory_format=torch.contiguous_format).reshape(-1).view(torch.uint8)
    ab, bb = flat(a), flat(b)
    diff = int((ab != bb).sum())
    assert diff == 0, f"{what}: {diff} of {ab.numel()} bytes differ, the first at byte {int((ab != bb).nonzero()[0])}"


def close(a, b, tol, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.numel() == 0:
        return
    a64, b64 = a.detach().double(), b.detach().double()
    assert bool((torch.isnan(a64) == torch.isnan(b64)).all()), f"{what}: NaNs differ"
    err = float((a64 - b64).nan_to_num(0.0, 0.0, 0.0).abs().max())
    if isinstance(tol, tuple):  # ("abs", bound)
        bound = tol[1]
    else:
        bound = tol * float(b64.nan_to_num(0.0, 0.0, 0.0).abs().max())
    print(f"{what}: max difference {err:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"


def compare(got, ref, tols, what):
    assert len(got) == len(ref), what
    for i, (a, b) in enumerate(zip(got, ref)):
        if a is None or b is None:
            assert a is None and b is None, f"{what}: output {i}"
        elif i in tols:
            close(a, b, tols[i], f"{what}: output {i}")
        else:
            same_bytes(a, b, f"{what}: output {i}")


SCRATCH_SHIFT = 16  # bytes: keeps every 16-byte vector access aligned and takes away the 256-byte alignment torch's allocator gives


def run_case(call, inputs, sizes=(), tols=None, offset=0, scratch_256=None, aligned=()):
    """call(ins) -> list of output tensors; inputs: name -> device tensor (anything else is passed on as it is);
    sizes: (size function's name, bytes) the wrapper must be seen to allocate; tols: output index -> tolerance (atomics only);
    offset: inputs start offset bytes off the 256-byte grid (the plain run too), except those named in `aligned` (inputs whose
    alignment the header demands).
    A fourth run (d) hands out the wrapper's scratch (flat uint8 tensors) SCRATCH_SHIFT bytes off the 256-byte grid: the size functions
    whose launchers align the pointer themselves must have the slack for it, and the others must not care.  scratch_256: the message
    with which an entry point that documents 256-byte alignment of its scratch refuses run (d)."""
    tols = tols or {}
    place = lambda fn: {k: (fn(v, 0 if k in aligned else offset) if torch.is_tensor(v) else v) for k, v in inputs.items()}
    ref = call(place(plain_at))
    torch.cuda.synchronize()
    outs = {}
    for run, body, shift in (("b", 0xFF, 0), ("c", 0x00, 0), ("d", 0xFF, SCRATCH_SHIFT)):
        rz = RedZone(DEV, body=body, scratch_offset=shift)
        ins = place(rz.guarded)
        with rz:
            if run == "d" and scratch_256:
                with pytest.raises(RuntimeError, match=scratch_256):
                    call(ins)
                continue
            outs[run] = call(ins)
        torch.cuda.synchronize()
        rz.check()
        for name, nbytes in sizes:
            rz.require(name, nbytes)
    compare(outs["b"], ref, tols, "guarded run against the plain run (a read outside an input?)")
    compare(outs["c"], outs["b"], tols, "zero-filled against NaN-filled buffers (scratch or output read before it is written?)")
    if "d" in outs:
        compare(outs["d"], outs["b"], tols, "scratch 16 bytes off the 256-byte grid against aligned scratch")
    COVERED.update(name for name, _ in sizes)


def grads(outputs, inputs, grad_outputs):
    return list(torch.autograd.grad(outputs, inputs, grad_outputs=grad_outputs, allow_unused=True))


# ---- knn, densification, Adam ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [4, 257, 2049])  # KNN_BOX 256, RS_TILE 2048
def test_knn(P):
    K = pkg("knn")
    run_case(lambda i: [K.distCUDA2(i["pts"])], {"pts": randn(rng(P), P, 3)}, [("dgm_knn_scratch_bytes", L().dgm_knn_scratch_bytes(P))],
             scratch_256="256-byte aligned")  # (the one scratch whose alignment the header demands, and the call checks)


def _gaussian_set(P, seed):
    g = rng(seed)
    return {"xyz": randn(g, P, 3), "f_dc": randn(g, P, 1, 3), "f_rest": randn(g, P, 3, 3), "opacity": randn(g, P, 1) * 3,
            "scaling": torch.log(rand(g, P, 3) * 0.02 + 0.001), "rotation": randn(g, P, 4), "normal": randn(g, P, 3),
            "accum": rand(g, P, 1) * 1.8e-3, "denom": torch.randint(0, 4, (P, 1), generator=g).float().to(DEV), "z": randn(g, 2, P, 3),
            "mask": (torch.rand(P, generator=g) < 0.3).to(DEV), "radii": rand(g, P) * 40}


def _model(i):
    D = pkg("densify")
    m = types.SimpleNamespace(optimizer=None, percent_dense=0.01, xyz_gradient_accum=i["accum"], denom=i["denom"], max_radii2D=i["radii"])
    for k in D.GROUPS:
        setattr(m, D.ATTR[k], i[k])
    return D, m


@pytest.mark.parametrize("P", [1, 257, 1025])  # block 256, scan stride 1024
def test_densify(P):
    nbytes, off = L().dgm_densify_scratch_bytes(P), L().dgm_densify_totals_offset(P)
    assert off % 4 == 0 and off + 12 <= nbytes  # the three totals the wrapper reads back lie inside the scratch

    def surgery(i, op):
        """Runs op on a model over this run's buffers; the scratch the wrapper allocated must be the size function's, and the three
        words at dgm_densify_totals_offset must be the (K, C, S) that sized the new set."""
        D, m = _model(i)
        seen, decide = [], D._decide
        D._decide = lambda *a, **k: seen.append(decide(*a, **k)) or seen[-1]
        try:
            op(D, m)
        finally:
            D._decide = decide
        scratch, K, C, S = seen[-1]
        out = [getattr(m, D.ATTR[k]).detach() for k in D.GROUPS]
        assert scratch.dtype == torch.uint8 and scratch.numel() == nbytes, "not covered: the decision's scratch is not dgm_densify_scratch_bytes"
        assert scratch[off:off + 12].view(torch.int32).tolist() == [K, C, S] and out[0].shape[0] == K + C + 2 * S
        return out, (K, C, S)

    def densify(i):
        return surgery(i, lambda D, m: D.densify_and_prune(m, 0.0002, 0.005, 0.9, None, samples=i["z"]))[0]

    def prune(i):
        out, (K, C, S) = surgery(i, lambda D, m: D.prune_points(m, i["mask"]))
        assert (K, C, S) == (int((~i["mask"]).sum()), 0, 0)
        return out

    sizes = [("dgm_densify_scratch_bytes", nbytes)]
    run_case(densify, _gaussian_set(P, P), sizes)
    run_case(prune, _gaussian_set(P, P + 1), sizes)
    COVERED.add("dgm_densify_totals_offset")  # (asserted inside every run above)


@pytest.mark.parametrize("P", [1, 257])
def test_densify_stats(P):
    def stats(i):
        lib = pkg("_lib")
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        lib.check(L().dgm_densify_stats(P, vp(i["g2d"]), vp(i["radii"]), vp(i["maxr"]), vp(i["accum"]), vp(i["denom"]), lib.stream_ptr()))
        return [i["maxr"], i["accum"], i["denom"]]

    g = rng(P)
    run_case(stats, {"g2d": randn(g, P, 3), "radii": torch.randint(-1, 30, (P,), generator=g).int().to(DEV), "maxr": rand(g, P) * 20,
                     "accum": rand(g, P, 1), "denom": rand(g, P, 1).round()})


@pytest.mark.parametrize("offset", [0, 4])  # 4: no tensor is 16-byte aligned, the kernel's scalar path
def test_adam(offset):
    numels = (1, 4095, 4097, 8193)  # ADAM_CHUNK 4096: a float4 body with a scalar tail

    def step(i):
        O = pkg("optim")
        params = [torch.nn.Parameter(i[f"p{k}"]) for k in range(len(numels))]
        opt = torch.optim.Adam(params, lr=1e-2, eps=1e-15)
        for k, p in enumerate(params):
            opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": i[f"m{k}"], "exp_avg_sq": i[f"v{k}"]}
            p.grad = i[f"g{k}"]
        ma = O.MultiAdam([opt])
        ma.step()
        ma.step()
        return [t for k in range(len(numels)) for t in (i[f"p{k}"], i[f"m{k}"], i[f"v{k}"])]

    g, ins = rng(7), {}
    for k, n in enumerate(numels):
        ins.update({f"p{k}": randn(g, n), f"g{k}": randn(g, n), f"m{k}": randn(g, n) * 0.1, f"v{k}": rand(g, n) * 0.01})
    run_case(step, ins, offset=offset)


# ---- losses, metrics, glue -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (16, 32), (17, 33)])  # tile 32 x 16, halo 5
def test_image_loss(H, W):
    def loss(i):
        img = i["image"].requires_grad_(True)
        out = pkg("loss").image_loss(img, i["gt"], 0.2)
        return [out.detach()] + grads(out, [img], i["go"])

    g = rng(H * 100 + W)
    run_case(loss, {"image": rand(g, 3, H, W), "gt": rand(g, 3, H, W), "go": rand(g) + 0.5},
             [("dgm_image_loss_workspace_bytes", L().dgm_image_loss_workspace_bytes(3, H, W))])


@pytest.mark.parametrize("B,H,W,ms", [(1, 11, 11, False), (2, 27, 43, False), (2, 161, 163, True)])  # valid tile 32 x 16
def test_image_metrics(B, H, W, ms):
    g = rng(H)
    run_case(lambda i: list(pkg("evaluate").image_metrics(i["images"], i["gt"], ms_ssim=ms).values()),
             {"images": rand(g, B, 3, H, W), "gt": rand(g, 3, H, W)},
             [("dgm_image_metrics_workspace_bytes", L().dgm_image_metrics_workspace_bytes(B, 3, H, W, 5 if ms else 1))])


_LPIPS = {}


@pytest.mark.parametrize("net,H,W", [("alex", 31, 31), ("alex", 35, 67), ("vgg", 16, 16), ("vgg", 33, 18)])
def test_lpips(net, H, W):
    import _lpips_ref as R
    Lp = pkg("lpips")
    if net not in _LPIPS:
        _LPIPS[net] = Lp.LPIPS(net, R.seeded_weights(net, 1), "cuda:0")
    model = _LPIPS[net]
    keys = [(k, n) for k in ("conv_w", "conv_b", "lin") for n in range(len(model._tensors[k]))]

    def run(i):
        m = Lp.LPIPS.__new__(Lp.LPIPS)  # the same weights, from the buffers of this run
        m.net, m.device = model.net, model.device
        m._tensors = {k: [i[f"{k}{n}"] for kk, n in keys if kk == k] for k in ("conv_w", "conv_b", "lin")}
        ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        m._ptrs = tuple(ptrs(m._tensors[k]) for k in ("conv_w", "conv_b", "lin"))
        out = m(i["images"], i["gt"])
        return [out["lpips"], out["layers"]]

    g = rng(H + W)
    ins = {"images": rand(g, 2, 3, H, W), "gt": rand(g, 3, H, W)}
    ins.update({f"{k}{n}": model._tensors[k][n] for k, n in keys})
    run_case(run, ins, [("dgm_lpips_workspace_bytes", L().dgm_lpips_workspace_bytes(Lp.NETS.index(net), 2, H, W))])


@pytest.mark.parametrize("P,ld", [(1, 10), (257, 13)])
def test_gaussian_apply(P, ld):
    def run(i):
        names = ("xyz", "scaling", "rotation", "opacity", "delta")
        ins = [i[k].requires_grad_(True) for k in names]
        outs = pkg("glue").gaussian_apply(*ins)
        return [o.detach() for o in outs] + grads(outs, ins, [i["g0"], i["g1"], i["g2"], i["g3"]])

    g = rng(P)
    run_case(run, {"xyz": randn(g, P, 3), "scaling": randn(g, P, 3), "rotation": randn(g, P, 4), "opacity": randn(g, P, 1),
                   "delta": randn(g, P, ld) * 0.1, "g0": randn(g, P, 3), "g1": randn(g, P, 3), "g2": randn(g, P, 4), "g3": randn(g, P, 1)})


@pytest.mark.parametrize("N,ld", [(1, 6), (257, 10)])
def test_se3(N, ld):
    def run(i):
        G = pkg("glue")
        o, xyz = i["o"].requires_grad_(True), i["xyz"].requires_grad_(True)
        T = G.se3_exp(o)
        Tl = T.detach().requires_grad_(True)
        out = G.se3_transform(Tl, xyz)
        dT, dxyz = grads(out, [Tl, xyz], i["g"])
        return [T.detach(), out.detach(), dT, dxyz] + grads(T, [o], i["gT"])

    g = rng(N)
    run_case(run, {"o": randn(g, N, ld) * 0.5, "xyz": randn(g, N, 3), "g": randn(g, N, 3), "gT": randn(g, N, 4, 4)})


@pytest.mark.parametrize("N,ld", [(1, 10), (1025, 10), (1025, 13), (1023, 13)])  # CYC_ROWS 1024
def test_cycle_loss(N, ld):
    def run(i):
        a, b = i["a"].requires_grad_(True), i["b"].requires_grad_(True)
        out = pkg("glue").cycle_loss(a, b)
        return [out.detach()] + grads(out, [a, b], i["go"])

    g = rng(N + ld)
    run_case(run, {"a": randn(g, N, ld), "b": randn(g, N, ld), "go": rand(g) + 0.5},
             [("dgm_cycle_loss_workspace_bytes", L().dgm_cycle_loss_workspace_bytes(N))])


# ---- the deformation MLP ---------------------------------------------------------------------------------------------------------------
def _mlp_inputs(N, T, seed):
    g = rng(seed)
    ins = {"x": rand(g, N, 3), "t": randn(g, 1, T), "hw": randn(g, 10, 256) * 0.05, "hb": randn(g, 10) * 0.1, "go": randn(g, N, 10)}
    for l in range(8):
        k = 63 + T if l == 0 else (256 + 63 + T if l == 5 else 256)
        ins[f"W{l}"], ins[f"b{l}"] = randn(g, 256, k) * math.sqrt(2.0 / k), randn(g, 256) * 0.1
    return ins


@pytest.mark.parametrize("mode,N", [("f16x3p", 1), ("f16x3p", 65), ("f16x3p", 513), ("f32", 1), ("f32", 65), ("f32", 513)])
def test_mlp(mode, N):  # GEMM tile 64 rows, DW_ROWS 512, HD_ROWS 256
    M = pkg("mlp_hip")
    dx = mode == "f16x3p"  # (dgm_mlp_backward_dx exists in the default arithmetic only)

    def run(i):
        wb = [i[f"W{l}"].requires_grad_(True) for l in range(8)] + [i[f"b{l}"].requires_grad_(True) for l in range(8)]
        x, t = i["x"].requires_grad_(dx), i["t"].requires_grad_(True)
        hw, hb = i["hw"].requires_grad_(True), i["hb"].requires_grad_(True)
        out = M._MLPFunction.apply(x, t, True, 1, hw, hb, *wb)
        return [out.detach()] + grads(out, ([x] if dx else []) + [t, hw, hb] + wb, i["go"])

    prev = L().dgm_mlp_set_gemm(3 if dx else 1)
    try:
        run_case(run, _mlp_inputs(N, 30, N), [("dgm_mlp_workspace_bytes", L().dgm_mlp_workspace_bytes(N))])
    finally:
        L().dgm_mlp_set_gemm(prev)


def test_timenet():
    def run(i):
        w = [i[k].requires_grad_(True) for k in ("W1", "b1", "W2", "b2")]
        out = pkg("mlp_hip")._TimeNetFunction.apply(i["t"], 6, *w)
        return [out.detach()] + grads(out, w, i["go"])

    g = rng(3)
    run_case(run, {"t": rand(g, 1, 1), "W1": randn(g, 256, 13) * 0.3, "b1": randn(g, 256) * 0.1, "W2": randn(g, 30, 256) * 0.1,
                   "b2": randn(g, 30) * 0.1, "go": randn(g, 1, 30)})


# ---- DPSR, Laplacian, opacity field, marching cubes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,res", [(1, 4), (257, 8)])
def test_dpsr(n, res):
    D = pkg("dpsr")

    def run(i):
        V, N, phi = i["V"].requires_grad_(True), i["N"].requires_grad_(True), i["phi"].requires_grad_(True)
        grid = D._Splat.apply(V, N, res)
        fv = D._Interp.apply(phi, V)
        spec = D._Spectral.apply(i["spec"], res, 2.0)
        return [grid.detach(), fv.detach(), torch.view_as_real(spec)] + grads(grid, [V, N], i["gg"]) + grads(fv, [phi, V], i["gf"])

    g = rng(n)
    spec = torch.view_as_complex(randn(g, 3, res, res, res // 2 + 1, 2))
    run_case(run, {"V": rand(g, n, 3) * 0.9 + 0.05, "N": randn(g, n, 3), "phi": randn(g, res, res, res), "spec": spec,
                   "gg": randn(g, 3, res, res, res), "gf": randn(g, n)},
             tols={0: TOL_DPSR_SPLAT, 3: TOL_DPSR_GRAD, 4: TOL_DPSR_GRAD, 5: TOL_DPSR_GRAD, 6: TOL_DPSR_GRAD})


@pytest.mark.parametrize("V,F", [(1, 1), (255, 300), (257, 300), (513, 1000)])  # 256 vertices per partial sum
def test_laplace(V, F):
    def run(i):
        v = i["v"].requires_grad_(True)
        loss = pkg("dpsr").laplace_regularizer_const(v, i["faces"])
        return [loss.detach()] + grads(loss, [v], i["go"])

    g = rng(V)
    run_case(run, {"v": randn(g, V, 3), "faces": torch.randint(0, V, (F, 3), generator=g).int().to(DEV), "go": rand(g) + 0.5},
             [("dgm_laplace_scratch_floats", 4 * L().dgm_laplace_scratch_floats(V))], tols={0: TOL_LAPLACE, 1: TOL_LAPLACE})


@pytest.mark.parametrize("P", [1, 257])  # 256 records per round, ragged last block: res 30 over 4 blocks
def test_opacity_field(P):
    MU = pkg("mesh_utils")

    def run(i):
        MU._COORDS.clear()  # (the wrapper caches the grid coordinates: this run's come from this run's buffers)
        MU._COORDS[(1.25, 30, "cuda", torch.cuda.current_device())] = i["coords"]
        try:
            return [MU.get_opacity_field_from_gaussians(i["xyz"], i["rot"], i["scal"], i["opac"], resolution=30, num_blocks=4)]
        finally:
            MU._COORDS.clear()

    g = rng(P)
    rot = torch.nn.functional.normalize(randn(g, P, 4), dim=1)
    run_case(run, {"xyz": rand(g, P, 3) * 2 - 1, "rot": rot, "scal": rand(g, P, 3) * 0.2 + 0.02, "opac": rand(g, P, 1),
                   "coords": torch.linspace(-1.25, 1.25, 30).to(DEV)},
             [("dgm_opacity_field_scratch_bytes", L().dgm_opacity_field_scratch_bytes(P))])


@pytest.mark.parametrize("dims", [(2, 2, 2), (9, 8, 15), (11, 10, 9), (17, 9, 7)])  # MC_PTS 1024 points, 64-point words
def test_marching_cubes(dims):
    MC = pkg("marching_cubes")
    g = rng(sum(dims))
    grid, deform = randn(g, *dims), (rand(g, *dims, 3) - 0.5) * 0.4
    nV = MC.marching_cubes(grid, deform)[0].shape[0]

    def run(i):
        gr, df = i["grid"].requires_grad_(True), i["deform"].requires_grad_(True)
        v, f = MC.marching_cubes(gr, df, 0.0, True)
        return [v.detach(), f] + grads(v, [gr, df], i["dv"])

    run_case(run, {"grid": grid, "deform": deform, "dv": randn(g, nV, 3)}, [("dgm_mc_scratch_bytes", L().dgm_mc_scratch_bytes(*dims))])


# ---- mesh rasterizer, shading, point splat, frame composition ----------------------------------------------------------------------------
@pytest.mark.parametrize("F,H,W", [(0, 1, 1), (0, 33, 17), (300, 33, 17), (300, 16, 64)])  # TR_THREADS 256, RAST_LARGE 64 pixel centres
def test_mesh_raster(F, H, W):
    from test_mesh_raster import random_scene
    MR = pkg("mesh_raster")
    pos, tri = random_scene(F, H, W, 5)
    g = rng(F + H)

    def run(i):
        p, a = i["pos"].requires_grad_(True), i["attr"].requires_grad_(True)
        rast, _ = MR.rasterize(None, p, i["tri"], (H, W))
        col, _ = MR.interpolate(a, rast, i["tri"])
        out = MR.antialias(col, rast, p, i["tri"])
        return [rast.detach(), col.detach(), out.detach()] + grads(out, [p, a], i["go"])

    Ft = int(tri.shape[0])
    run_case(run, {"pos": pos.to(DEV).unsqueeze(0).contiguous(), "tri": tri.to(DEV).contiguous(), "attr": rand(g, pos.shape[0], 4),
                   "go": randn(g, 1, H, W, 4)},
             [("dgm_tri_raster_scratch_bytes", L().dgm_tri_raster_scratch_bytes(Ft, H, W)), ("dgm_tri_aa_scratch_bytes", L().dgm_tri_aa_scratch_bytes(Ft))],
             tols={3: TOL_TRI_DPOS, 4: TOL_TRI_DATTR})


@pytest.mark.parametrize("H,W", [(1, 1), (17, 33)])
def test_vertex_normals_and_shade(H, W):
    from test_mesh_eval import icosphere
    from test_mesh_raster import random_scene
    V, MR, lib = pkg("visualize"), pkg("mesh_raster"), pkg("_lib")
    v, f = icosphere(1.0, 2)
    verts, faces = dev(v), dev(f)
    run_case(lambda i: [V.vertex_normals(i["verts"], i["faces"])], {"verts": verts, "faces": faces}, tols={0: ("abs", TOL_VNORMALS_ABS)})
    # the shading pass on fixed normals (vertex_normals sums with atomics) and a rast buffer of its own size
    pos, tri = random_scene(0, H, W, 2)
    rast, _ = MR.rasterize(None, pos.to(DEV).unsqueeze(0).contiguous(), tri.to(DEV).contiguous(), (H, W))
    nV = pos.shape[0]
    g = rng(H)
    params = torch.tensor([0.3, 0.4, 0.866, 0.5, 0.0, 0.0, 3.0, 0.3, 1.0, 1.0, 1.0, 0.04, 0.9, 0.8, 0.7, 10.0, 1.0, 0.0, 0.0, 0.0], device=DEV)

    def shade(i):
        image = torch.empty((H, W, 3), dtype=torch.float32, device=DEV)
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        lib.check(L().dgm_mesh_shade(nV, int(tri.shape[0]), H, W, vp(i["verts"]), vp(i["normals"]), vp(i["faces"]), vp(i["rast"]),
                                     vp(i["params"]), vp(image), lib.stream_ptr()))
        return [image]

    run_case(shade, {"verts": randn(g, nV, 3), "normals": torch.nn.functional.normalize(randn(g, nV, 3), dim=1), "faces": tri.to(DEV).contiguous(),
                     "rast": rast.detach(), "params": params})


@pytest.mark.parametrize("N,H,W,size", [(1, 1, 1, 1), (257, 17, 33, 3), (257, 16, 16, 15)])  # VZ_THREADS 256
def test_point_splat(N, H, W, size):
    g = rng(N + size)
    pos = torch.cat([rand(g, N, 2) * 2.4 - 1.2, rand(g, N, 1), torch.ones(N, 1, device=DEV)], 1) * (rand(g, N, 1) + 0.5)
    run_case(lambda i: list(pkg("visualize").splat_points(i["pos"], H, W, colors=i["colors"], size=size, return_ids=True)),
             {"pos": pos.contiguous(), "colors": rand(g, N, 3)}, [("dgm_point_splat_scratch_bytes", L().dgm_point_splat_scratch_bytes(H, W))])


@pytest.mark.parametrize("H,W,d", [(1, 1, 1), (17, 33, 1), (18, 34, 2)])
def test_compose_frame(H, W, d):
    g = rng(H)
    run_case(lambda i: [pkg("visualize").compose_frame([i["a"], i["b"], i["c"]], d, layouts=["chw", "hwc", "chw"])],
             {"a": rand(g, 3, H, W) * 1.2 - 0.1, "b": rand(g, H, W, 3), "c": rand(g, 3, H, W)})


# ---- anchoring, entering the mesh phase ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nq,Nt", [(1, 1), (257, 255), (255, 257), (4097, 300)])  # BF_TILE 256, SCAN_TILE 4096
def test_anchor_nearest(Nq, Nt):
    A = pkg("anchor")
    g = rng(Nq)
    run_case(lambda i: list(A._nearest_raw(i["q"], i["t"], 0.05)) + list(A._nearest_raw(i["q"], i["t"], math.inf)),
             {"q": rand(g, Nq, 3), "t": rand(g, Nt, 3)}, [("dgm_anchor_nn_scratch_bytes", L().dgm_anchor_nn_scratch_bytes(Nq, Nt))])


@pytest.mark.parametrize("P,F", [(1, 1), (257, 65), (4097, 4097)])  # AN_THREADS 256, SCAN_TILE 4096
def test_anchor_classify_and_geometry(P, F):
    A = pkg("anchor")
    g = rng(P)

    def run(i):
        out = A.classify(i["face_of"], F)
        return [out[k] for k in ("counts", "offsets", "lists", "members", "rank")] + list(A.face_geometry(i["verts"], i["faces"]))

    V = F + 2
    faces = torch.randint(0, V, (F, 3), generator=g).int()
    faces[::7, 1] = V  # (an index outside [0, V): a NaN centroid, nothing is read there)
    run_case(run, {"face_of": torch.randint(-1, F + 1, (P,), generator=g).int().to(DEV), "verts": randn(g, V, 3), "faces": faces.to(DEV)},
             [("dgm_anchor_classify_scratch_bytes", L().dgm_anchor_classify_scratch_bytes(P, F))])


@pytest.mark.parametrize("P,offset", [(1, 0), (1023, 0), (1025, 0), (1025, 4)])  # 256 threads x 4 rows; offset 4: the scalar path
def test_ninit_bbox(P, offset):
    # the one scratch with a required initial state: zero before the first call.  The wrapper allocates it with torch.zeros, so it is
    # zero in both guarded runs; the second call below runs on what the first one left.
    NI = pkg("normal_init")

    def run(i):
        scratch = NI.bbox_scratch(i["xyz"].device)
        return [NI.bbox(i["xyz"], i["d"], scratch=scratch), NI.bbox(i["xyz"], None, scratch=scratch)]

    g = rng(P)
    run_case(run, {"xyz": randn(g, P, 3), "d": randn(g, P, 3) * 0.1}, [("dgm_ninit_bbox_scratch_bytes", L().dgm_ninit_bbox_scratch_bytes())],
             offset=offset)


@pytest.mark.parametrize("F,count", [(1, 1), (4095, 257), (4097, 257)])  # SCAN_TILE 4096 faces
def test_ninit_sample(F, count):
    NI = pkg("normal_init")
    g = rng(F)
    V = F + 2
    faces = torch.randint(0, V, (F, 3), generator=g).int()
    if F > 1:
        faces[::9, 2] = -1

    def run(i):
        area = NI.face_areas(i["verts"], i["faces"])
        return [area, NI.cumulative_areas(area)] + list(NI.sample_surface(i["verts"], i["faces"], count, draws=i["u"], check=False))

    run_case(run, {"verts": randn(g, V, 3), "faces": faces.to(DEV), "u": rand(g, count, 3)},
             [("dgm_ninit_scan_scratch_bytes", L().dgm_ninit_scan_scratch_bytes(F))])


# ---- mesh evaluation, cleaning, simplification, correspondence ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,M", [(1, 1, 1), (2, 257, 255), (2, 255, 513)])  # EMD_R 256 rows, EMD_C 256 columns
def test_emd(B, N, M):
    g = rng(N + M)
    run_case(lambda i: list(pkg("mesh_eval").emd_approx(i["a"], i["b"], return_residual=True)), {"a": rand(g, B, N, 3), "b": rand(g, B, M, 3)},
             [("dgm_emd_scratch_floats", 4 * L().dgm_emd_scratch_floats(B, N, M))])


@pytest.mark.parametrize("V,F", [(1, 1), (65, 65), (4097, 4097), (4095, 8193)])  # MC_TILE 4096, MC_THREADS 256
def test_mesh_clean(V, F):
    from test_mesh_clean import soup  # (its faces repeat indices: invalid faces that connect nothing)
    MC = pkg("mesh_clean")
    v, f = soup(V, F, V)
    run_case(lambda i: list(MC.clean_mesh(i["verts"], i["faces"], largest=True, min_faces=2, min_diameter_frac=0.01, return_index=True))
             + list(MC.clean_mesh(i["verts"], i["faces"], return_index=True)), {"verts": dev(v), "faces": dev(f)},
             [("dgm_mesh_cc_scratch_bytes", max(L().dgm_mesh_cc_scratch_bytes(V, F), 1)),
              ("dgm_mesh_cc_select_scratch_bytes", L().dgm_mesh_cc_select_scratch_bytes()),
              ("dgm_mesh_compact_scratch_bytes", max(L().dgm_mesh_compact_scratch_bytes(V, F), 1))])


@pytest.mark.parametrize("V,F", [(1, 1), (65, 65), (4097, 4097), (4095, 8193)])  # SP_TILE 4096, SP_THREADS 256
def test_mesh_simplify(V, F):
    from test_mesh_simplify import soup
    MS = pkg("mesh_simplify")
    v, f = soup(V, F, V)
    f[::11, 0], f[5::13, 2] = -1, V  # indices outside [0, V): dropped before any use
    run_case(lambda i: list(MS.simplify_mesh(i["verts"], i["faces"], grid=5, return_index=True)), {"verts": dev(v), "faces": dev(f)},
             [("dgm_mesh_simplify_scratch_bytes", L().dgm_mesh_simplify_scratch_bytes(V, F)),
              ("dgm_mesh_compact_scratch_bytes", max(L().dgm_mesh_compact_scratch_bytes(V, F), 1))])


@pytest.mark.parametrize("N,sub", [(1, 0), (257, 2), (4097, 3)])  # BF_TILE 256 faces, SCAN_TILE 4096; 20 / 320 / 1280 faces
def test_surface(N, sub):
    from test_mesh_eval import icosphere
    C = pkg("correspondence")
    v, f = icosphere(1.0, sub)
    g = rng(N)

    def run(i):
        near = C.closest_on_mesh(i["points"], i["verts"], i["faces"], max_dist=0.3)
        far = C.closest_on_mesh(i["points"], i["verts"], i["faces"])
        return list(near) + list(far) + [C.interpolate(i["attr"], i["faces"], far[0], far[2]), C.palette(i["points"], (0.0, 0.1, 0.0), 1.3, "checker")]

    pts = torch.nn.functional.normalize(randn(g, N, 3), dim=1) * (0.8 + 0.5 * rand(g, N, 1))
    run_case(run, {"points": pts.contiguous(), "verts": dev(v), "faces": dev(f), "attr": randn(g, v.shape[0], 5)},
             [("dgm_surf_closest_scratch_bytes", L().dgm_surf_closest_scratch_bytes(N, f.shape[0]))])


# ---- dataset ingest and resampling -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,offset", [(1, 1, 1, 3, 0), (2, 5, 7, 4, 0), (2, 17, 33, 3, 0), (2, 17, 33, 3, 4), (2, 17, 33, 3, 1), (2, 17, 33, 4, 4)])
def test_ingest(B, H, W, C, offset):
    DS = pkg("dataset")
    g = rng(H + C)
    byte = lambda *s: torch.randint(0, 256, s, generator=g).to(torch.uint8).to(DEV)

    def run(i):
        out = list(DS.image_ingest(i["pix"], (1.0, 0.5, 0.0))) + [DS.image_composite_bytes(i["pix"], (0.2, 0.4, 1.0))]
        for m in ("m1", "m3"):
            out += list(DS.image_ingest_masked(i["pix"], i[m], (1.0, 1.0, 1.0))) + [DS.image_ingest_masked(i["pix"], i[m], (0.0, 0.0, 0.0), out="bytes")]
        return out

    run_case(run, {"pix": byte(B, H, W, C), "m1": byte(B, H, W, 1) // 128, "m3": byte(B, H, W, 3) // 64}, offset=offset)


@pytest.mark.parametrize("B,H,W,ch", [(1, 1, 1, 1), (2, 33, 17, 1), (2, 33, 17, 3), (2, 1025, 3, 4)])  # UF_ROWS 1024 rows per band
def test_png_unfilter_and_expand(B, H, W, ch):
    PNG = pkg("png_io")
    g = rng(H)
    raw = torch.randint(0, 256, (B, H, 1 + W * ch), generator=g).to(torch.uint8)
    raw[:, :, 0] = torch.randint(0, 5, (B, H), generator=g).to(torch.uint8)

    def run(i):
        out = [PNG.unfilter(i["raw"], B, W, H, ch)]
        if ch == 1:
            out += [PNG.expand(i[f"p{d}"], 8 // d * W - 1 if d < 8 else W, d, PNG.GREY_SCALE[d]) for d in (1, 2, 4, 8)]  # ragged last byte
        return out

    ins = {"raw": raw.reshape(-1).to(DEV)}
    ins.update({f"p{d}": torch.randint(0, 256, (B, H, W), generator=g).to(torch.uint8).to(DEV) for d in (1, 2, 4, 8)})
    run_case(run, ins)


@pytest.mark.parametrize("C,offset", [(1, 0), (3, 0), (3, 4), (3, 1), (4, 0), (4, 4)])  # RS_ROWS 4 rows per block, columns padded to 4
def test_resample(C, offset):
    RS = pkg("resample")
    g = rng(C)
    B, H, W = 2, 21, 19

    def resizes(pix):
        out = [RS.resize(pix, (7, 5), "lanczos"), RS.resize(pix, (33, 21), "bicubic"), RS.resize(pix, (19, 9), "bicubic"),
               RS.resize_nearest(pix, (9, 13))]
        if C > 1:
            out += list(RS.resize(pix, (10, 11), "bicubic", premultiplied=False, out="planes"))
            out += list(RS.resize(pix, (W, H), "bicubic", out="planes"))
        return out

    # The wrapper builds its coefficient / bounds / index tables on the host and caches the uploads.  A first call fills the caches;
    # every run then reads the tables from ITS buffers (exact size between guards: the kernels read them with 16-byte loads), and
    # must not have had to build another one.
    pix = torch.randint(0, 256, (B, H, W, C), generator=g).to(torch.uint8).to(DEV)
    RS._TABLES.clear(), RS._NEAREST.clear()
    resizes(pix)
    tables, nearest = dict(RS._TABLES), dict(RS._NEAREST)
    RS._TABLES.clear(), RS._NEAREST.clear()
    ins = {"pix": pix}
    for n, (taps, bounds, _) in enumerate(tables.values()):
        ins[f"taps{n}"], ins[f"bounds{n}"] = taps, bounds
    ins.update({f"near{n}": t for n, t in enumerate(nearest.values())})

    def run(i):
        RS._TABLES.clear(), RS._NEAREST.clear()
        RS._TABLES.update({k: (i[f"taps{n}"], i[f"bounds{n}"], v[2]) for n, (k, v) in enumerate(tables.items())})
        RS._NEAREST.update({k: i[f"near{n}"] for n, k in enumerate(nearest)})
        try:
            out = resizes(i["pix"])
            assert set(RS._TABLES) == set(tables) and set(RS._NEAREST) == set(nearest), "a table was built outside the guarded ones"
            return out
        finally:
            RS._TABLES.clear(), RS._NEAREST.clear()

    run_case(run, ins, offset=offset, aligned=[k for k in ins if k != "pix"])  # (kx / bounds_x: 16-byte aligned, int32 tables: 4)


# ---- the Gaussian rasterizer's three state chunks, through the C ABI ------------------------------------------------------------------------
def _raw_rasterize(a, dL, rz, chunk_offset=0):
    """dgm_rasterize_forward / _backward with allocator callbacks that hand out guarded chunks of exactly the requested size,
    chunk_offset bytes off the 256-byte grid (dgm_alloc_fn promises 128-byte alignment, the library aligns to 256 itself)."""
    lib = pkg("_lib")
    t = lambda x: torch.empty(0, device=DEV) if x is None else rz.guarded(torch.as_tensor(np.ascontiguousarray(x), device=DEV))
    ptr = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None and x.numel() else None
    P, W, H = a["means3D"].shape[0], a["W"], a["H"]
    bg, means, opac, scales, rots = t(a["bg"]), t(a["means3D"]), t(a["opacities"]), t(a["scales"]), t(a["rotations"])
    vm, pm, cam, sh, dLt = t(a["viewmatrix"]), t(a["projmatrix"]), t(a["campos"]), t(a["sh"]), t(dL)
    M = sh.shape[1]
    asked, chunks = {}, {}

    def callback(name):
        def cb(_ctx, nbytes):
            asked[name] = int(nbytes)
            chunks[name] = rz._alloc("callback " + name, (int(nbytes),), torch.uint8, chunk_offset)
            return chunks[name].data_ptr()
        return lib.ALLOC_FN(cb)

    cbs = [callback(n) for n in ("geometry", "binning", "image")]
    with rz:
        color = torch.empty((3, H, W), dtype=torch.float32, device=DEV)
        radii = torch.empty(P, dtype=torch.int32, device=DEV)
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=DEV)
        g = {"dL_dmeans2D": new(P, 3), "dL_dconic": new(P, 2, 2), "dL_dopacity": new(P, 1), "dL_dcolors": new(P, 3), "dL_dmeans3D": new(P, 3),
             "dL_dcov3D": new(P, 6), "dL_dsh": new(P, M, 3), "dL_dscales": new(P, 3), "dL_drotations": new(P, 4)}
    R = ctypes.c_int(0)
    st = lib.stream_ptr()
    lib.check(L().dgm_rasterize_forward(cbs[0], None, cbs[1], None, cbs[2], None, P, a["degree"], M, ptr(bg), W, H, ptr(means), ptr(sh), None,
                                        ptr(opac), ptr(scales), 1.0, ptr(rots), None, ptr(vm), ptr(pm), ptr(cam), a["tanfovx"], a["tanfovy"], 0,
                                        ptr(color), ptr(radii), 0, st, ctypes.byref(R)))
    lib.check(L().dgm_rasterize_backward(P, a["degree"], M, R.value, ptr(bg), W, H, ptr(means), ptr(sh), None, ptr(scales), 1.0, ptr(rots), None,
                                         ptr(vm), ptr(pm), ptr(cam), a["tanfovx"], a["tanfovy"], ptr(radii), ptr(chunks["geometry"]),
                                         ptr(chunks.get("binning")), ptr(chunks["image"]), ptr(dLt), ptr(g["dL_dmeans2D"]), ptr(g["dL_dconic"]),
                                         ptr(g["dL_dopacity"]), ptr(g["dL_dcolors"]), ptr(g["dL_dmeans3D"]), ptr(g["dL_dcov3D"]), ptr(g["dL_dsh"]),
                                         ptr(g["dL_dscales"]), ptr(g["dL_drotations"]), 0, st))
    torch.cuda.synchronize()
    return R.value, asked, color, radii, g


@pytest.mark.parametrize("P", [1, 257])
def test_gaussian_rasterizer_state_chunks(P, syn):
    import gpu_util
    W, H = 33, 17  # no multiple of the 16 x 16 tile
    a = raster_args(syn, P, W, H, seed=P)
    dL = np.random.RandomState(P).randn(3, H, W).astype(np.float32)
    fwd = gpu_util.hip_forward(a)
    ref = gpu_util.hip_backward(a, fwd, dL)
    outs = {}
    for run, body, chunk_offset in (("b", 0xFF, 0), ("c", 0x00, 0), ("d", 0xFF, 128)):
        rz = RedZone(DEV, body=body)
        R, asked, color, radii, g = _raw_rasterize(a, dL, rz, chunk_offset)
        rz.check()
        assert R == fwd["num_rendered"]
        want = {"geometry": L().dgm_geometry_bytes(P, W, H), "image": L().dgm_image_bytes(W, H)}
        if R > 0 or "binning" in asked:
            want["binning"] = L().dgm_binning_bytes(R)
        assert asked == want, f"the callbacks were asked for {asked}, the size functions say {want}"
        same_bytes(color.cpu(), torch.from_numpy(fwd["color"]), "colour")
        same_bytes(radii.cpu(), torch.from_numpy(fwd["radii"]), "radii")
        for k, v in ref.items():
            same_bytes(g[k].reshape(v.shape).cpu(), torch.from_numpy(v), k)
        outs[run] = [color, radii] + [g[k] for k in sorted(ref)]
    compare(outs["c"], outs["b"], {}, "zero-filled against NaN-filled state chunks")
    compare(outs["d"], outs["b"], {}, "state chunks at 128-byte alignment against 256")
    COVERED.update(("dgm_geometry_bytes", "dgm_binning_bytes", "dgm_image_bytes"))


def test_mark_visible(syn):
    a = raster_args(syn, 257, 33, 17, seed=2)
    run_case(lambda i: [pkg("rasterizer")._C.mark_visible(i["means"], i["vm"], i["pm"])],
             {"means": dev(a["means3D"]), "vm": dev(a["viewmatrix"]), "pm": dev(a["projmatrix"])})


# ---- the harness on the device, and the record ------------------------------------------------------------------------------------------------------------------------
def test_harness_sees_a_torch_write_outside_a_device_buffer():
    """The harness's own check on the device, with torch writes into the guard bytes (never a kernel on a short buffer)."""
    with RedZone(DEV) as rz:
        t = torch.empty(1000, dtype=torch.float32, device=DEV)
    t.fill_(1.0)
    torch.cuda.synchronize()
    rz.check()
    rec = rz.records[0]
    assert t.data_ptr() % 256 == 0 and rec.nbytes == 4000
    rec.raw[rec.start + rec.nbytes + 2] = 7
    rec.raw[rec.start - 1] = 7
    assert rec.damage() == (-1, 4002)
    with pytest.raises(AssertionError, match=r"allocation #0 .*bytes -1 \.\. 4002"):
        rz.check()


def test_zz_every_size_function_has_a_green_case():
    """Runs last in this file: every size function the header declares (a function returning size_t) was seen, at its exact value, in a
    case above that passed.  A size function added later without a case fails here."""
    header = open(os.path.join(ROOT, "include", "dgmesh_hip.h")).read()
    declared = set(re.findall(r"^size_t\s+(dgm_\w+)\s*\(", header, flags=re.M))
    assert len(declared) >= 27 and all(n.endswith(("_bytes", "_floats", "_offset")) for n in declared), sorted(declared)
    print("size functions covered by a green red-zone case:\n  " + "\n  ".join(sorted(COVERED)))
    missing = sorted(declared - COVERED)
    assert not missing, f"size functions without a green red-zone case (run the whole file): {missing}"
