"""evaluate.image_metrics (dgm_image_metrics, csrc/metrics.hip) against the float64 restatement tests/_metrics_ref.py.

Bounds.  PSNR: 1e-5 dB (the squared error is summed in fp64; 10 / ln 10 times a relative error of 1e-6 is 4.3e-6 dB).  SSIM and
MS-SSIM: twice the largest fp32 deviation the golden records for the reference itself (ssim_fp32_err: rgb_ssim on fp32 against fp64
tensors; msssim_fp32_err: the restatement on fp32 against fp64 arrays), each with a floor of 2^-20.  The kernel computes in fp64 on
the fp32 inputs, and the restatement is run on those same fp32 values: measured deviations are in DESIGN.md section 4.8."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg

sys.path.insert(0, os.path.join(ROOT, "tests"))
import _metrics_ref as MR  # noqa: E402
from test_metrics_ref import GOLD, KINDS, SHAPES, pair8  # noqa: E402

FLOOR = 2.0 ** -20
SSIM_TOL = max(FLOOR, 2 * max(float(GOLD[f"{k}_{H}x{W}/ssim_fp32_err"]) for k in KINDS for H, W in SHAPES))
MSSSIM_TOL = max(FLOOR, 2 * max(float(GOLD[f"{k}_{H}x{W}/msssim_fp32_err"]) for k in KINDS for H, W in SHAPES if min(H, W) > 160))
PSNR_TOL = 1e-5
CASES = [(11, 11)] + SHAPES
_REF = {}


def pair32(kind, H, W):
    """fp32 (3, H, W) pair; 11x11 is a crop of the 12x43 pair."""
    if (H, W) == (11, 11):
        x, y = pair8(kind, 12, 43)
        x, y = x[:, 1:12, 20:31], y[:, 1:12, 20:31]
    else:
        x, y = pair8(kind, H, W)
    return (x.astype(np.float64) / 255).astype(np.float32), (y.astype(np.float64) / 255).astype(np.float32)


def reference(kind, H, W):
    """The restatement in float64 on the fp32 values the kernel sees; computed once per pair."""
    key = (kind, H, W)
    if key not in _REF:
        x, y = (a.astype(np.float64) for a in pair32(kind, H, W))
        _REF[key] = dict(mse=MR.mse(x, y), psnr=MR.psnr(x, y), ssim=MR.ssim(x, y), ms_ssim=MR.ms_ssim(x, y) if min(H, W) > 160 else None)
    return _REF[key]


def check(row, ref, label):
    err = {k: (0.0 if row[k] == ref[k] else abs(row[k] - ref[k])) for k in row}  # (inf == inf for identical images)
    print(label, " ".join(f"{k} {row[k]:.12g} err {err[k]:.3e}" for k in row))
    assert err["mse"] <= 1e-6 * ref["mse"]
    assert err["psnr"] <= PSNR_TOL
    assert err["ssim"] <= SSIM_TOL
    if "ms_ssim" in row:
        assert err["ms_ssim"] <= MSSSIM_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", CASES)
def test_matches_the_restatement(H, W):
    E = pkg("evaluate")
    dev = torch.device("cuda:0")
    ms = min(H, W) > 160
    print(f"bounds: psnr {PSNR_TOL:.1e} ssim {SSIM_TOL:.3e} ms_ssim {MSSSIM_TOL:.3e}")
    for kind in KINDS:
        x, y = pair32(kind, H, W)
        other = pair32("flat" if kind != "flat" else "smooth", H, W)[0]
        ref = reference(kind, H, W)
        gt = torch.tensor(y, device=dev)
        one = E.image_metrics(torch.tensor(x, device=dev), gt, ms_ssim=ms)                          # B = 1, (C, H, W)
        two = E.image_metrics(torch.tensor(np.stack([other, x]), device=dev), gt, ms_ssim=ms)      # B = 2, this pair second
        assert set(one) == ({"mse", "psnr", "ssim", "ms_ssim"} if ms else {"mse", "psnr", "ssim"})
        assert all(v.shape == (1,) and v.is_cuda for v in one.values()) and all(v.shape == (2,) for v in two.values())
        check({k: float(v[0]) for k, v in one.items()}, ref, f"{kind} {H}x{W} B=1")
        check({k: float(v[1]) for k, v in two.items()}, ref, f"{kind} {H}x{W} B=2")
    if ms:
        x, _ = pair32("smooth", H, W)
        t = torch.tensor(x, device=dev)
        assert float(E.image_metrics(t, t)["ms_ssim"][0]) == 1.0 and float(E.image_metrics(t, t)["ssim"][0]) == 1.0
        inv = E.image_metrics(*(torch.tensor(a, device=dev) for a in pair32("inverse", H, W)))
        assert float(inv["ms_ssim"][0]) == 0.0  # negative cs: the relu engages


@pytest.mark.gpu
def test_data_range_scales_the_constants():
    """Both images and data_range times 255: SSIM and MS-SSIM are unchanged up to rounding, the MSE scales by 255^2."""
    E = pkg("evaluate")
    dev = torch.device("cuda:0")
    x, y = (torch.tensor(a, device=dev) for a in pair32("smooth", 161, 163))
    a = E.image_metrics(x, y)
    b = E.image_metrics(x * 255, y * 255, data_range=255.0)
    assert abs(float(a["ssim"][0]) - float(b["ssim"][0])) <= SSIM_TOL and abs(float(a["ms_ssim"][0]) - float(b["ms_ssim"][0])) <= MSSSIM_TOL
    assert abs(float(b["mse"][0]) / 255.0 ** 2 - float(a["mse"][0])) <= 1e-5 * float(a["mse"][0])


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(33, 70), (176, 162)])
def test_reproducible_and_independent_of_the_batch(H, W):
    E = pkg("evaluate")
    dev = torch.device("cuda:0")
    ms = min(H, W) > 160
    x, y = pair32("smooth", H, W)
    f = pair32("flat", H, W)[0]
    gt = torch.tensor(y, device=dev)
    both = torch.tensor(np.stack([x, f]), device=dev)
    a, b = E.image_metrics(both, gt, ms_ssim=ms), E.image_metrics(both, gt, ms_ssim=ms)
    s0, s1 = E.image_metrics(both[0], gt, ms_ssim=ms), E.image_metrics(both[1], gt, ms_ssim=ms)
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k], torch.cat([s0[k], s1[k]])), k
        assert a[k].dtype == torch.float64 and bool(torch.isfinite(a[k]).all())


@pytest.mark.gpu
def test_errors():
    E = pkg("evaluate")
    dev = torch.device("cuda:0")
    with pytest.raises(ValueError):
        E.image_metrics(torch.zeros(3, 160, 200, device=dev), torch.zeros(3, 160, 200, device=dev), ms_ssim=True)
    assert set(E.image_metrics(torch.zeros(3, 160, 200, device=dev), torch.zeros(3, 160, 200, device=dev), ms_ssim=False)) == {"mse", "psnr", "ssim"}
    with pytest.raises(ValueError):
        E.image_metrics(torch.zeros(3, 10, 40, device=dev), torch.zeros(3, 10, 40, device=dev), ms_ssim=False)
    with pytest.raises(ValueError):
        E.image_metrics(torch.zeros(2, 3, 12, 40, device=dev), torch.zeros(3, 12, 41, device=dev), ms_ssim=False)
    with pytest.raises(RuntimeError):
        E.image_metrics(torch.zeros(3, 176, 176), torch.zeros(3, 176, 176))
    with pytest.raises(RuntimeError):
        E.image_metrics(torch.zeros(3, 176, 176, device=dev, dtype=torch.float64), torch.zeros(3, 176, 176, device=dev, dtype=torch.float64))


def test_cpu_tensors_raise_without_a_gpu():
    E = pkg("evaluate")
    with pytest.raises(RuntimeError):
        E.image_metrics(torch.zeros(3, 176, 176), torch.zeros(3, 176, 176))


def test_abi_lists_the_metrics_entry_points():
    L = pkg("_lib")
    assert {"dgm_image_metrics", "dgm_image_metrics_workspace_bytes"} <= set(L.SYMBOLS) and L.ABI_VERSION == 5
    lib = L.lib()
    assert lib.dgm_image_metrics_workspace_bytes(2, 3, 176, 162, 5) > 0
    assert lib.dgm_image_metrics_workspace_bytes(2, 3, 160, 200, 5) == 0 and lib.dgm_image_metrics_workspace_bytes(1, 3, 10, 40, 1) == 0
    assert lib.dgm_image_metrics_workspace_bytes(1, 3, 11, 11, 1) > 0 and lib.dgm_image_metrics_workspace_bytes(1, 3, 200, 200, 3) == 0
