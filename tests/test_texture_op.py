"""GPU tests of mesh_raster.texture (csrc/mesh_texture.hip) against the numpy restatement (tests/_texture_ref.py).

Forward: |dev - ref64| <= tol on every value, ref64 the fp64 statement.  tol is not chosen: per case it is 8 x the largest |ref32 - ref64|
of the numpy fp32 statement in the device's operation order -- what the number format gives on that case (the rule of
tests/test_mesh_inside.py).  The factor and the device's largest error are printed per case.
Gradients against the fp64 statement: duv by the same 8 x rule (the kernel stores it, in a stated order); dtex, which the kernel sums with
fp32 atomics in no particular order, within the a-priori bound of _texture_ref.dtex_bound (a sum of m fp32 terms in any order).  The
fp64 duv itself is checked against torch.autograd through grid_sample for the two boundary modes grid_sample has.  The uv of the
gradient cases lie at least 1e-3 texel away from the texel-centre lattice (the kinks of the bilinear weights) and from the texel
boundaries (where `nearest` jumps), by construction of the generator: a condition on the inputs, not a tolerance.
The forward is bit-reproducible: a second run and a batch split in parts give the same bytes."""
import functools

import numpy as np
import pytest
import torch

import _texture_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_FACTOR = 8.0
SHAPES = [(1, 1, 1), (2, 3, 1), (5, 7, 3), (33, 130, 3), (64, 64, 4)]
COUNTS = [1, 63 * 65]
MODES = [(f, b) for f in R.FILTERS for b in R.BOUNDARIES]


def MR():
    return pkg("mesh_raster")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def specials(Ht, Wt):
    """Exact texel centres (the first, the last and one inside), exact 0 and 1, NaN, +-inf and +-1e30."""
    c = lambda i, N: (i + 0.5) / N
    rows = [(c(0, Wt), c(0, Ht)), (c(Wt - 1, Wt), c(Ht - 1, Ht)), (c(Wt // 2, Wt), c(Ht // 2, Ht)), (0.0, 0.0), (1.0, 1.0), (0.0, 1.0),
            (np.nan, 0.3), (0.3, np.nan), (np.inf, 0.5), (0.5, -np.inf), (1e30, 0.25), (0.25, -1e30), (-1e30, 1e30)]
    return np.array(rows, np.float64).astype(np.float32)


@functools.lru_cache(maxsize=None)
def forward_case(Ht, Wt, C, n):
    """tex, uv and dout, shared and read-only: uv uniform in [-1.5, 2.5]^2, the first rows of the large case replaced by the specials."""
    rng = np.random.default_rng(Ht * 1009 + Wt * 31 + C + n)
    tex = rng.standard_normal((Ht, Wt, C)).astype(np.float32)
    uv = rng.uniform(-1.5, 2.5, (n, 2)).astype(np.float32)
    if n > 1:
        sp = specials(Ht, Wt)
        uv[:len(sp)] = sp
    for a in (tex, uv):
        a.setflags(write=False)
    return tex, uv


@functools.lru_cache(maxsize=None)
def grad_case(Ht, Wt, C, n):
    """uv = (k + f + .5) / size with integer k and f in [1e-3, .5 - 1e-3] or [.5 + 1e-3, 1 - 1e-3] (2e-3 before the rounding to fp32,
    which moves a sample by at most 2^-24 * 2.5 * 130 = 2e-5 texel), plus non-finite and huge rows, which get no gradient."""
    rng = np.random.default_rng(Ht * 7 + Wt * 13 + C * 3 + n)
    size = np.array([Wt, Ht], np.float64)
    k = np.floor(rng.uniform(-1.5, 2.5, (n, 2)) * size)
    f = rng.uniform(2e-3, 0.5 - 2e-3, (n, 2)) + 0.5 * rng.integers(0, 2, (n, 2))
    uv = ((k + f + 0.5) / size).astype(np.float32)
    if n > 1:  # (0.2837 is clear of both lattices at every size of SHAPES)
        uv[:5] = np.array([(np.nan, 0.2837), (0.2837, np.inf), (-np.inf, np.nan), (1e30, 0.2837), (0.2837, -1e30)], np.float32)
    near = np.abs(uv) < 10  # (the huge coordinates reduce to exactly 0 or saturate the clamp in either number format)
    d = R.lattice_distance(np.where(near, uv, 0.2837), Ht, Wt)
    assert np.minimum(d, 0.5 - d).min() >= 1e-3
    tex = rng.standard_normal((Ht, Wt, C)).astype(np.float32)
    dout = rng.standard_normal((n, C)).astype(np.float32)
    for a in (tex, uv, dout):
        a.setflags(write=False)
    return tex, uv, dout


def uv_shape(n):
    return (1, 63, 65, 2) if n == 63 * 65 else (1, n, 2)


def same(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


@pytest.mark.parametrize("filter_mode,boundary_mode", MODES)
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("Ht,Wt,C", SHAPES)
def test_forward_values_and_reproducibility(Ht, Wt, C, n, filter_mode, boundary_mode):
    tex, uv = forward_case(Ht, Wt, C, n)
    ref64 = R.sample(tex, uv, filter_mode, boundary_mode, np.float64)
    ref32 = R.sample(tex, uv, filter_mode, boundary_mode, np.float32)
    t, q = dev(tex)[None], dev(uv).reshape(uv_shape(n))
    keep = (t.clone(), q.clone())
    out = MR().texture(t, q, filter_mode=filter_mode, boundary_mode=boundary_mode)
    assert out.shape == uv_shape(n)[:-1] + (C,) and out.dtype == torch.float32 and out.device.type == "cuda"
    got = out.reshape(-1, C).cpu().numpy()
    ref_err = float(np.abs(ref32.astype(np.float64) - ref64).max())
    tol = TOL_FACTOR * ref_err
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    print(f"{(Ht, Wt, C)} n {n} {filter_mode}/{boundary_mode}: device max |out - ref64| {err:.3e}; numpy fp32 statement {ref_err:.3e}, "
          f"factor {TOL_FACTOR:g}, tolerance {tol:.3e}")
    assert np.isfinite(got).all()
    assert err <= tol, f"{err:.3e} > {tol:.3e}"
    bad = ~np.isfinite(uv).all(1)
    assert (got[bad] == 0).all()
    if filter_mode == "linear" and boundary_mode == "wrap" and n > 1:
        assert same(out, MR().texture(t, q, filter_mode="auto"))  # auto is linear, wrap the default
    # the same bytes: a second run, the batch in three parts, one sample alone
    assert same(MR().texture(t, q, filter_mode=filter_mode, boundary_mode=boundary_mode), out)
    flat, whole = q.reshape(1, -1, 2), out.reshape(1, -1, C)
    for lo, hi in ((0, 1), (1, 65), (65, n), (n - 1, n)):
        if lo < hi <= n:
            part = MR().texture(t, flat[:, lo:hi].contiguous(), filter_mode=filter_mode, boundary_mode=boundary_mode)
            assert same(part, whole[:, lo:hi])
    assert same(t, keep[0]) and same(q, keep[1])  # inputs unmodified (NaN compared as bytes)


def grid_sample_duv(tex, uv, dout, padding):
    """duv of sum(grid_sample(tex, 2 uv - 1) * dout) by torch.autograd, fp64 on the host."""
    t = torch.from_numpy(tex.astype(np.float64)).permute(2, 0, 1)[None]
    q = torch.from_numpy(uv.astype(np.float64)).requires_grad_(True)
    out = torch.nn.functional.grid_sample(t, (2 * q - 1).reshape(1, 1, -1, 2), mode="bilinear", padding_mode=padding, align_corners=False)
    (out[0, :, 0].T * torch.from_numpy(dout.astype(np.float64))).sum().backward()
    return q.grad.numpy()


@pytest.mark.parametrize("filter_mode,boundary_mode", MODES)
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("Ht,Wt,C", SHAPES)
def test_gradients(Ht, Wt, C, n, filter_mode, boundary_mode):
    tex, uv, dout = grad_case(Ht, Wt, C, n)
    dtex64, duv64 = R.sample_grads(tex, uv, dout, filter_mode, boundary_mode, np.float64)
    _, duv32 = R.sample_grads(tex, uv, dout, filter_mode, boundary_mode, np.float32)
    finite = np.isfinite(uv).all(1)
    if filter_mode == "linear" and boundary_mode in ("clamp", "zero"):  # the reference's own duv against autograd
        auto = grid_sample_duv(tex, uv[finite], dout[finite], "border" if boundary_mode == "clamp" else "zeros")
        scale = max(1.0, float(np.abs(auto).max()))
        assert np.abs(auto - duv64[finite]).max() <= 1e-12 * scale
    t, q = dev(tex)[None].requires_grad_(True), dev(uv).reshape(uv_shape(n)).requires_grad_(True)
    out = MR().texture(t, q, filter_mode=filter_mode, boundary_mode=boundary_mode)
    g = dev(dout).reshape(out.shape)
    dtex, duv = torch.autograd.grad(out, [t, q], grad_outputs=g)
    assert dtex.shape == t.shape and duv.shape == q.shape
    dtex, duv = dtex[0].cpu().numpy().astype(np.float64), duv.reshape(-1, 2).cpu().numpy().astype(np.float64)
    bound = R.dtex_bound(tex.shape, uv, dout, filter_mode, boundary_mode)
    excess = np.abs(dtex - dtex64) - bound
    duv_ref_err = float(np.abs(duv32.astype(np.float64) - duv64).max())
    duv_err = float(np.abs(duv - duv64).max())
    print(f"{(Ht, Wt, C)} n {n} {filter_mode}/{boundary_mode}: dtex max error {np.abs(dtex - dtex64).max():.3e} (largest bound {bound.max():.3e}, "
          f"max |dtex| {np.abs(dtex64).max():.3e}); duv max error {duv_err:.3e}, numpy fp32 statement {duv_ref_err:.3e}, tolerance "
          f"{TOL_FACTOR * duv_ref_err:.3e}, max |duv| {np.abs(duv64).max():.3e}")
    assert np.isfinite(dtex).all() and np.isfinite(duv).all()
    assert excess.max() <= 0, f"dtex: {np.abs(dtex - dtex64).max():.3e} outside the summation bound by {excess.max():.3e}"
    assert duv_err <= TOL_FACTOR * duv_ref_err, f"duv: {duv_err:.3e} > {TOL_FACTOR * duv_ref_err:.3e}"
    assert (duv[~finite] == 0).all()
    if filter_mode == "nearest":
        assert (duv == 0).all()


def test_argument_checks_on_device_tensors():
    M = MR()
    tex, uv = torch.zeros(1, 4, 4, 3, device=DEV), torch.zeros(1, 2, 2, 2, device=DEV)
    assert M.texture(tex, uv).shape == (1, 2, 2, 3)
    assert M.texture(tex, uv.reshape(1, 4, 2)).shape == (1, 4, 3) and M.texture(tex, uv[:, :0]).shape == (1, 0, 2, 3)
    with pytest.raises(RuntimeError, match="only batch size 1"):
        M.texture(tex.expand(2, -1, -1, -1).contiguous(), uv)
    with pytest.raises(RuntimeError, match="only batch size 1"):
        M.texture(tex, uv.expand(2, -1, -1, -1).contiguous())
    with pytest.raises(RuntimeError, match="must be torch.float32"):
        M.texture(tex.double(), uv)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        M.texture(tex.permute(0, 2, 1, 3), uv)
    with pytest.raises(RuntimeError, match=r"uv must be \(1, ..., 2\)"):
        M.texture(tex, torch.zeros(1, 2, 2, 3, device=DEV))
    with pytest.raises(RuntimeError, match=r"tex must be \(1, Ht, Wt, C\)"):
        M.texture(tex[0], uv)
