"""The mesh chain end to end -- MeshPhase.psr -> MeshPhase.surface -> mesh_raster.render_mask_and_mesh /
dpsr.laplace_regularizer_const -> loss -- and its gradients, against the fp64 restatement composed in _meshchain_ref.py.

Host tests pin the restatement first: its differentiable marching cubes against _mc_ref, its gradient against central
differences, the normals' scale invariance, and that its own fp32 run stays under a quarter of the stage bounds on the inputs
of the GPU tests.  The GPU tests then hold the device chain to it, stage by stage, on the device's own discrete decisions.

Errors are max |x - x64| / max |x64| (the threshold's scalar gradient and the loss values: relative to the value).  Gates:
e_hip <= 4 e_f32 + 1e-6, e_f32 being the same restatement in fp32 on the same decisions (four fp32 atomic accumulations of free
order lie on the chain: splat, MC adjoint, interpolate / antialias adjoint, Laplacian), and the stage bounds as ceilings: 2e-4
for psr and every figure of the lap term (test_dpsr.py), 1e-3 for everything through the rasterizer (test_mesh_raster.py)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _mc_ref as MC
import _meshchain_ref as C
import _meshrast_ref as MR
from conftest import pkg

D = torch.float64
# (res, P, H, W, scene seed).  The seed is the first of 0, 1, 2, ... at which, with and without deformations, (i) every figure of
# the restatement's fp32 run on the host stays under a fifth of its ceiling, (ii) the threshold's gradient -sum dL/dpsr cancels by
# at most kappa = sum |dL/dpsr| / |sum dL/dpsr| <= MAX_KAPPA in every term and (iii) every figure of the restatement's fp32 run
# on the device stays under YARDSTICK_HEADROOM of the gate set by its run on the host.  Why, and what was measured: DESIGN.md
# section 4.5b.  test_reference_stays_under_a_quarter_of_the_bounds holds (i) and (ii) to account,
# test_gpu_yardstick_holds_on_another_fp32_evaluation (iii), at the gate itself.
SIZES = [(24, 1500, 40, 56, 16), (32, 3000, 48, 64, 35)]
MAX_KAPPA = 25.0
YARDSTICK_HEADROOM = 0.7
TERMS = ("mask", "img", "lap", "sum")
CONFIGS = {"deform": dict(deform=True), "nodeform": dict(deform=False), "freeze": dict(deform=True, freeze=True),
           "freeze_nodeform": dict(deform=False, freeze=True), "negated": dict(deform=True, negate=True)}
LEAVES = ("xyz", "normal", "d_xyz", "d_normal", "thres")
CEIL_DPSR, CEIL_RASTER = 2e-4, 1e-3
MAX_ZERO_WEIGHT = 0.02  # of H W


def ceiling(term, tensor):
    """psr itself (term "-") and every figure of the lap term: the DPSR bound; everything else passes the rasterizer."""
    return CEIL_DPSR if term in ("-", "lap") else CEIL_RASTER


@functools.lru_cache(maxsize=None)
def scene(size):
    res, P, H, W, seed = SIZES[size]
    return C.scene(res, P, H, W, seed)


@functools.lru_cache(maxsize=None)
def host(size, deform=True):
    return C.host_decisions(scene(size), deform)


def detached(lv):
    return tuple(None if t is None else t.detach() for t in lv)


def term_loss(loss, term):
    return loss["mask"] + loss["img"] + loss["lap"] if term == "sum" else loss[term]


def rel_scalar(a, b):
    a, b = (float(x.detach()) if torch.is_tensor(x) else float(x) for x in (a, b))
    return abs(a - b) / max(abs(b), 1e-300)


def err(name, a, b):
    return rel_scalar(a, b) if name == "thres" or name.startswith("loss") else C.rel_max(a, b)


def zero_weight(mask, image, ref, fragile):
    """-> (zero, stray), (H, W) bool.  `zero`: the pixels left out of both sides' rendered losses -- fragile centres whose
    antialiased forward value (mask or any colour channel) also differs from the fp64 restatement's by more than 1e-4,
    test_mesh_raster.py's criterion for an antialias decision taken the other way.  `stray`: pixels that differ so without being
    fragile centres; they keep their weight and every caller asserts that there are none.  (Fragile centres that agree are kept:
    the winners are the device's on both sides, and with the near plane at 0.01 the whole object spans 3e-4 of z/w, so every
    silhouette pixel -- where the mask gradient lives -- is a near-tie.)"""
    differs = torch.maximum((mask.detach().cpu().double() - ref.mask.cpu().double()).abs().amax(-1),
                            (image.detach().cpu().double() - ref.image.cpu().double()).abs().amax(0)) > 1e-4
    return differs & fragile, differs & ~fragile


def grads_per_term(run, lv, active):
    """Backward of each term through one forward: {term: {tensor: gradient}} for dL/dverts, dL/dpsr and the `active` leaves."""
    out = {}
    for term in TERMS:
        for t in (run.psr, run.verts) + tuple(x for x in lv if x is not None):
            t.grad = None
        term_loss(run.loss, term).backward(retain_graph=True)
        g = {"verts": run.verts.grad.detach().clone(), "psr": run.psr.grad.detach().clone()}
        for name, x in zip(LEAVES, lv):
            if name in active:
                g[name] = x.grad.detach().clone()
            elif x is not None:
                g["_" + name] = None if x.grad is None else x.grad.detach().clone()  # (freeze_pos: must be None or all zero)
        out[term] = g
    return out


def restatement(sc, dec, dtype, weight, deform=True, freeze=False, negate=False, device="cpu"):
    lv = C.leaves(sc, dtype, deform, negate, device=device)
    run = C.chain(*lv, sc, dec, dtype, freeze_pos=freeze, weight=weight)
    active = [n for n, x in zip(LEAVES, lv) if x is not None and not (freeze and n in ("xyz", "d_xyz"))]
    return run, lv, grads_per_term(run, lv, active), active


# ---- host: the restatement itself -----------------------------------------------------------------------------------------------
def test_differentiable_mc_is_the_restatements_mc():
    """mc_vertices on a grid equals _mc_ref.marching_cubes in float64, and its autograd gradient _mc_ref.backward."""
    dec, _ = host(0)
    sc = scene(0)
    with torch.no_grad():
        x, n, dx, dn, th = (t.detach() for t in C.leaves(sc, D))
        d = lambda v: v.to(D)
        grid = C.signed_psr(C.unit_points(x, dx, d(sc.center), d(sc.scale)), n + dn, th, sc.res, sc.sig, D, dec.cells)
    v, faces, rec = MC.marching_cubes(grid.numpy(), 0.0, dtype=np.float64)
    g = grid.clone().requires_grad_(True)
    mine = C.mc_vertices(g, rec)
    ev = float(np.abs(mine.detach().numpy() - v).max())
    dverts = torch.randn(mine.shape, generator=torch.Generator().manual_seed(1), dtype=D)
    (mine * dverts).sum().backward()
    ref, _ = MC.backward(rec, dverts.numpy())
    eg = float(np.abs(g.grad.numpy() - ref).max() / np.abs(ref).max())
    print(f"differentiable MC: {len(v)} vertices, max |dv| {ev:.2e}; gradient {eg:.2e} of max")
    assert ev <= 1e-15
    assert eg <= 1e-12


# Ten times the worst better-step figure measured for this construction (mask 9.0e-9, img 1.7e-9, lap 4.9e-10; the rounding of
# a loss of 0.7 differenced over 2e-5 against a derivative of 3e-3 is 3e-9), far inside the cap of 1e-2.  A wiring error in the
# restatement is a factor or a sign.
FD_GATE = 10 * 9.02e-9


@pytest.mark.parametrize("term", C.TERMS)
def test_chain_gradient_matches_central_differences(term):
    """The directional derivative of the whole fp64 chain along one random direction in positions, normals and the threshold at
    once, with cells, topology and winners frozen.  The targets keep the L1 signs fixed; what stays piecewise is the antialias
    rule and the trilinear weights at a cell face, so the better of two steps is gated.  First size only, as measured
    when the construction was laid out; at the second, a point that lies within a step of a cell face can spoil both steps."""
    sc = scene(0)
    dec, _ = host(0)
    w = sc.weight
    gen = torch.Generator().manual_seed(5)
    lv = C.leaves(sc)
    x, n, dx, dn, th = lv
    dirs = [torch.randn(x.shape, generator=gen, dtype=D), torch.randn(n.shape, generator=gen, dtype=D),
            torch.randn((), generator=gen, dtype=D)]
    C.chain(*lv, sc, dec, weight=w).loss[term].backward()
    an = float((x.grad * dirs[0]).sum() + (n.grad * dirs[1]).sum() + th.grad * dirs[2])
    figs = []
    for h in (1e-5, 1e-6):
        val = []
        for s in (1.0, -1.0):
            with torch.no_grad():
                o = C.chain(x.detach() + s * h * dirs[0], n.detach() + s * h * dirs[1], dx.detach(), dn.detach(),
                            th.detach() + s * h * dirs[2], sc, dec, weight=w)
            val.append(float(o.loss[term]))
        fd = (val[0] - val[1]) / (2 * h)
        figs.append(abs(fd - an) / abs(an))
        print(f"MESHCHAIN_FD {term} h={h:g}: autograd {an:.9e} central difference {fd:.9e} rel {figs[-1]:.2e}")
    assert min(figs) <= FD_GATE


@pytest.mark.parametrize("size", range(len(SIZES)))
def test_normals_scale_invariance(size):
    """psr is invariant under N -> c N (every step is linear in N, the result divided by |phi[0, 0, 0]|): sum N . dL/dN = 0."""
    sc = scene(size)
    dec, _ = host(size)
    lv = C.leaves(sc)
    run = C.chain(*lv, sc, dec)
    term_loss(run.loss, "sum").backward()
    nd = (lv[1] + lv[3]).detach() * lv[1].grad
    print(f"scale invariance {SIZES[size][:4]}: |sum N.dL/dN| = {float(nd.sum().abs()):.2e} of {float(nd.abs().sum()):.2e}")
    assert torch.equal(lv[1].grad, lv[3].grad)
    assert float(nd.sum().abs()) <= 1e-12 * float(nd.abs().sum())


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("size", range(len(SIZES)))
def test_reference_stays_under_a_quarter_of_the_bounds(size, config):
    """The restatement's fp32 run against its fp64 run on the GPU tests' inputs (host decisions; the zero-weight rule of the GPU
    tests, with the fp32 run in the device's place): every compared figure under a quarter of its ceiling, i.e. the inputs are well
    conditioned for any fp32 evaluation; and no term's gradient vanishes."""
    sc = scene(size)
    kw = CONFIGS[config]
    dec, fragile = host(size, kw["deform"])
    with torch.no_grad():
        fwd = [C.chain(*detached(C.leaves(sc, dt, kw["deform"], kw.get("negate", False))), sc, dec, dt) for dt in (D, torch.float32)]
    zero, stray = zero_weight(fwd[1].mask, fwd[1].image, fwd[0], fragile)
    print(f"{SIZES[size][:4]} {config}: {dec.rec['a'].size} vertices, {dec.faces.shape[0]} faces, {int(zero.sum())} of "
          f"{sc.H * sc.W} pixels weigh zero; {int(fragile.sum())} fragile centres; {int(stray.sum())} other pixels differ by 1e-4")
    assert int(stray.sum()) == 0
    assert int(fragile.sum()) <= MAX_ZERO_WEIGHT * sc.H * sc.W  # (bounds `zero`, a subset)
    w = sc.weight * (~zero)
    r64, _, g64, active = restatement(sc, dec, D, w, **kw)
    r32, _, g32, _ = restatement(sc, dec, torch.float32, w, **kw)
    worst = []
    e = C.rel_max(r32.psr, r64.psr)
    print(f"MESHCHAIN_REF {size} {config} - psr {e:.2e} (quarter {CEIL_DPSR / 4:.1e})")
    worst.append(e / ceiling("-", "psr"))
    for term in TERMS:
        names = ["loss"] + ["verts", "psr"] + active
        for name in names:
            e = (rel_scalar(term_loss(r32.loss, term), term_loss(r64.loss, term)) if name == "loss"
                 else err(name, g32[term][name], g64[term][name]))
            print(f"MESHCHAIN_REF {size} {config} {term} {name} {e:.2e} (quarter {ceiling(term, name) / 4:.1e})")
            worst.append(e / ceiling(term, name))
    assert max(worst) <= 0.25
    kappa = {t: float(g64[t]["psr"].abs().sum() / g64[t]["psr"].sum().abs()) for t in TERMS}
    print(f"MESHCHAIN_REF {size} {config} kappa of the threshold gradient: " + " ".join(f"{t} {k:.1f}" for t, k in kappa.items()))
    assert max(kappa.values()) <= MAX_KAPPA
    assert all(float(g64[t][n].abs().max()) > 0 for t in TERMS for n in active)
    if config == "negated":  # the same function of -N: the same mesh, every normal gradient negated
        _, _, gb, _ = restatement(sc, dec, D, w, deform=True)
        assert C.rel_max(g64["sum"]["normal"], -gb["sum"]["normal"]) <= 1e-12
        assert C.rel_max(g64["sum"]["xyz"], gb["sum"]["xyz"]) <= 1e-12


# ---- GPU: the device chain against the restatement ------------------------------------------------------------------------------
class _Gaussians:
    """What MeshPhase.psr / surface read of the Gaussian model."""

    def __init__(self, sc, lv):
        self.get_xyz, self.get_normal, self.density_thres_param = lv[0], lv[1], lv[4]
        self.gaussian_center = sc.center.cuda()
        self.gaussian_scale = sc.scale.reshape(1).cuda()


@pytest.mark.gpu
def test_gpu_restatement_runs_on_the_device_too():
    """The fp64 restatement on the device (rocFFT, device index ops) against its host run, on the host's decisions: fp64 rounding
    through a chain that amplifies fp32 rounding (6e-8) to at most 5e-5 in its own fp32 run, i.e. by 1e3: 1e-13 expected, 1e-9
    asked."""
    sc = scene(0)
    dec, _ = host(0)
    out = []
    for dev in ("cpu", "cuda"):
        lv = C.leaves(sc, D, device=dev)
        run = C.chain(*lv, sc, dec)
        term_loss(run.loss, "sum").backward()
        out.append([run.psr] + [x.grad for x in lv])
    figs = [C.rel_max(a, b) for a, b in zip(out[1], out[0])]
    print("restatement on the device vs on the host (psr, dxyz, dnormal, dd_xyz, dd_normal, dthres): "
          + " ".join(f"{e:.1e}" for e in figs))
    assert max(figs) <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("deform", [True, False])
@pytest.mark.parametrize("size", range(len(SIZES)))
def test_gpu_yardstick_holds_on_another_fp32_evaluation(size, deform):
    """The restatement alone, no product code: its fp32 run on the device against the gate 4 e_f32 + 1e-6 that its fp32 run on the
    host sets, both against fp64, on the host's decisions.  Where this fails, e_f32 is a lucky sample and the gate judges the FFT
    library, not the chain; the seeds are chosen so that it holds with headroom (SIZES)."""
    sc = scene(size)
    dec, _ = host(size, deform)
    r64, _, g64, active = restatement(sc, dec, D, sc.weight, deform)
    runs = [restatement(sc, dec, torch.float32, sc.weight, deform, device=dev) for dev in ("cpu", "cuda")]
    worst = (0.0, None)
    for term in TERMS:
        for name in ["verts", "psr"] + active:
            e_host, e_dev = (err(name, g[term][name], g64[term][name]) for _, _, g, _ in runs)
            worst = max(worst, (e_dev / (4 * e_host + 1e-6), f"{term} {name} {e_dev:.2e} against {e_host:.2e}"))
    config = "deform" if deform else "nodeform"
    print(f"MESHCHAIN_FIG {size}/{config} yardstick: worst figure at {worst[0]:.2f} of the gate ({worst[1]})")
    assert worst[0] <= 1.0


_RUNS = {}


def gpu_run(size, config):
    """_gpu_run once per (size, config).  After a device run has failed, no test starts another: they all report that failure."""
    key = (size, config)
    if "failed" in _RUNS:
        raise RuntimeError(f"the device run of {_RUNS['failed'][0]} failed in an earlier test: {_RUNS['failed'][1]!r}")
    if key not in _RUNS:
        try:
            _RUNS[key] = _gpu_run(size, config)
        except BaseException as e:
            _RUNS["failed"] = (key, e)
            raise
    return _RUNS[key]


def _gpu_run(size, config):
    """One forward of the device chain and of the restatement (fp64, fp32) on the device's decisions, one backward per term:
    {figures: {(term, tensor): (e_hip, e_f32)}, ...}.  Shared by every test of (size, config)."""
    T, DP, MRD, S = pkg("trainer"), pkg("dpsr"), pkg("mesh_raster"), pkg("scene")
    sc = scene(size)
    kw = CONFIGS[config]
    deform, freeze, negate = kw["deform"], kw.get("freeze", False), kw.get("negate", False)
    ms = T.MeshPhase(None, None, None, dpsr=DP.DPSR(res=(sc.res,) * 3, sig=sc.sig), n_verts=8, mesh_source="diffmc",
                     mesh_losses="render")
    lv = C.leaves(sc, torch.float32, deform, negate, device="cuda")
    g = _Gaussians(sc, lv)
    cam = S.TorchCamera(sc.camera, "cuda")
    psr = ms.psr(g, lv[2], lv[3], freeze_pos=freeze)
    psr.retain_grad()
    verts, faces = ms.surface(g, psr)
    verts.retain_grad()
    colour = C.vertex_colour(verts, g.gaussian_center, g.gaussian_scale)
    mask, image = MRD.render_mask_and_mesh(None, verts, faces, colour, cam)
    with torch.no_grad():
        pos = MRD.clip_positions(cam, verts)
        rast, _ = MRD.rasterize(None, pos, faces, (sc.H, sc.W))  # (bit-reproducible: the winners render_mask_and_mesh used)
        cells = C.unit_points(lv[0], lv[2], g.gaussian_center, g.gaussian_scale).cpu()
    # the device's decisions
    _, rfaces, rec = MC.marching_cubes(psr.detach().cpu().numpy(), 0.0)
    assert np.array_equal(rfaces, faces.cpu().numpy())
    dec = C.Decisions(cells=cells, rec=rec, faces=torch.as_tensor(rfaces.astype(np.int64)),
                      ids=rast[0, ..., 3].long().cpu(), zw=rast[0, ..., 2].double().cpu())
    # pixels that weigh zero: fragile centres at the device's positions whose antialiased value also differs by more than 1e-4
    _, _, fragile = MR.rasterize_ids(pos[0].double().cpu(), dec.faces, sc.H, sc.W)
    with torch.no_grad():
        f64 = C.chain(*detached(C.leaves(sc, D, deform, negate)), sc, dec, D, freeze_pos=freeze)
    zero, stray = zero_weight(mask, image, f64, fragile)
    w = sc.weight * (~zero)
    print(f"MESHCHAIN_FIG {size}/{config}: {verts.shape[0]} vertices, {faces.shape[0]} faces; {int(zero.sum())} of {sc.H * sc.W} "
          f"pixels weigh zero; {int(fragile.sum())} fragile centres; {int(stray.sum())} other pixels differ by more than 1e-4")
    dev = SimpleNamespace(psr=psr, verts=verts, faces=faces, mask=mask, image=image)
    dev.loss = C.losses(dev, sc, w, lap=DP.laplace_regularizer_const)
    active = [n for n, x in zip(LEAVES, lv) if x is not None and not (freeze and n in ("xyz", "d_xyz"))]
    gd = grads_per_term(dev, lv, active)
    r64, l64, g64, _ = restatement(sc, dec, D, w, deform, freeze, negate)
    r32, _, g32, _ = restatement(sc, dec, torch.float32, w, deform, freeze, negate)
    figs = {("-", "psr"): (C.rel_max(psr, r64.psr), C.rel_max(r32.psr, r64.psr))}
    for term in TERMS:
        ref = term_loss(r64.loss, term)
        figs[(term, "loss")] = (rel_scalar(term_loss(dev.loss, term), ref), rel_scalar(term_loss(r32.loss, term), ref))
        for name in ["verts", "psr"] + active:
            figs[(term, name)] = (err(name, gd[term][name], g64[term][name]), err(name, g32[term][name], g64[term][name]))
    # the exact statements and the identity, per term
    clamped = all(float(gd[t][n][i, ax]) == 0.0 for t in TERMS for n in ("xyz", "d_xyz") if n in gd[t] for i, ax in sc.outside)
    frozen = all(v is None or not bool(v.any()) for t in TERMS for k, v in gd[t].items() if k.startswith("_"))
    N = (lv[1] + lv[3] if deform else lv[1]).detach().double().cpu()
    N64 = (l64[1] + l64[3] if deform else l64[1]).detach()
    ident = {t: (float((N * gd[t]["normal"].double().cpu()).sum().abs()), float((N64.float() * g32[t]["normal"].cpu()).sum().abs()),
                 float((N * gd[t]["normal"].double().cpu()).abs().sum())) for t in TERMS}
    # the threshold's gradient is -sum dL/dpsr: the device's two figures against each other, relative to sum |dL/dpsr|
    wiring = {t: float((gd[t]["thres"].double() + gd[t]["psr"].double().sum()).abs() / gd[t]["psr"].double().abs().sum())
              for t in TERMS}
    normal = {t: (gd[t]["normal"].double().cpu(), g64[t]["normal"]) for t in TERMS}
    return dict(figs=figs, zero=int(zero.sum()), stray=int(stray.sum()), pixels=sc.H * sc.W, normal=normal, clamped=clamped,
                frozen=frozen, ident=ident, wiring=wiring,
                faces=faces.cpu(), has_frozen=any(k.startswith("_") for k in gd["sum"]))


@pytest.mark.gpu
@pytest.mark.parametrize("term", TERMS)
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("size", range(len(SIZES)))
def test_gpu_chain_matches_the_fp64_restatement(size, config, term):
    """psr, the loss value and every tensor gradient of one term, stage by stage (the threshold's scalar gradient: the next test)."""
    r = gpu_run(size, config)
    assert r["stray"] == 0, "the device's antialiased forward differs by more than 1e-4 at pixels that are not fragile centres"
    assert r["zero"] <= MAX_ZERO_WEIGHT * r["pixels"]
    bad = gate(r, size, config, term, lambda name: name != "thres")
    assert not bad, bad


def gate(r, size, config, term, keep):
    bad = []
    for (t, name), (e_hip, e_f32) in r["figs"].items():
        if t not in (term, "-") or not keep(name):
            continue
        bound = min(4 * e_f32 + 1e-6, ceiling(t, name))
        print(f"MESHCHAIN_FIG {size}/{config}/{term} {name} {e_hip:.2e} {e_f32:.2e} {bound:.2e}")
        if not e_hip <= bound:
            bad.append((name, e_hip, e_f32, bound))
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("term", TERMS)
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("size", range(len(SIZES)))
def test_gpu_threshold_gradient_matches_the_fp64_restatement(size, config, term):
    """dL/d(threshold), relative to its value, under the same gate; and that it is minus the sum of the device's dL/dpsr, to the
    rounding of an fp32 tree sum over res^3 values (15 levels x 6e-8 < 1e-6 of sum |dL/dpsr|; 2e-8 measured).

    This scalar is where a lucky e_f32 shows first: at seeds that fail criterion (iii) of SIZES the device chain missed this gate
    by the factor by which the restatement's own fp32 run on the device missed it (24, seed 5: 1.3 against 1.5; 32, seed 13: 1.5
    against 1.2; 24, seed 14: 10.8 against 10.0), with dL/dpsr of the same case inside its gate."""
    r = gpu_run(size, config)
    print(f"MESHCHAIN_FIG {size}/{config}/{term} thres+sum(dL/dpsr) {r['wiring'][term]:.2e} of sum |dL/dpsr| (bound 1e-6)")
    assert r["wiring"][term] <= 1e-6
    bad = gate(r, size, config, term, lambda name: name == "thres")
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["deform", "nodeform", "negated"])
@pytest.mark.parametrize("size", range(len(SIZES)))
def test_gpu_clamped_coordinates_get_exactly_zero(size, config):
    """The Gaussians outside the cube: the coordinate the clamp holds gets no gradient at all, through any term."""
    assert gpu_run(size, config)["clamped"]


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["freeze", "freeze_nodeform"])
@pytest.mark.parametrize("size", range(len(SIZES)))
def test_gpu_freeze_pos_keeps_every_gradient_from_the_positions(size, config):
    """freeze_pos (the normal warm-up): positions and d_xyz get None or all zeros, whether or not a deformation is given; the
    normals' gradient is held to the gate by test_gpu_chain_matches_the_fp64_restatement."""
    r = gpu_run(size, config)
    assert r["has_frozen"] and r["frozen"]
    assert ("sum", "normal") in r["figs"] and ("sum", "xyz") not in r["figs"]


@pytest.mark.gpu
@pytest.mark.parametrize("size", range(len(SIZES)))
def test_gpu_negated_normals_give_the_same_faces(size):
    """N -> -N flips the sign taken from psr[0, 0, 0] and nothing else: the same faces (the gradients: the next test)."""
    assert torch.equal(gpu_run(size, "negated")["faces"], gpu_run(size, "deform")["faces"])


@pytest.mark.gpu
@pytest.mark.parametrize("term", TERMS)
@pytest.mark.parametrize("size", range(len(SIZES)))
def test_gpu_negated_normals_negate_the_normals_gradient(size, term):
    """The device's dL/dnormal of the run with every normal negated, negated, against the fp64 restatement of the run with the
    normals as they are, under that run's gate: the statement itself, device to device, on top of each run's own gate."""
    neg, base = gpu_run(size, "negated"), gpu_run(size, "deform")
    e_hip, e_f32 = C.rel_max(-neg["normal"][term][0], base["normal"][term][1]), base["figs"][(term, "normal")][1]
    bound = min(4 * e_f32 + 1e-6, ceiling(term, "normal"))
    print(f"MESHCHAIN_FIG {size}/negated-vs-deform/{term} normal {e_hip:.2e} {e_f32:.2e} {bound:.2e}")
    assert e_hip <= bound


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("size", range(len(SIZES)))
def test_gpu_normals_scale_identity(size, config):
    """|sum N . dL/dN| on the device's gradients, against four times its value in the fp32 restatement."""
    bad = []
    for term, (hip, f32, total) in gpu_run(size, config)["ident"].items():
        bound = 4 * f32 + 1e-6 * total
        print(f"MESHCHAIN_FIG {size}/{config}/{term} sum_N.dL/dN {hip:.2e} {f32:.2e} {bound:.2e} (sum |N.dL/dN| {total:.2e})")
        if not hip <= bound:
            bad.append((term, hip, f32, bound))
    assert not bad, bad
