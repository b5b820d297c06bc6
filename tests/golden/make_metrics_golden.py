"""Writes tests/golden/metrics_small.npz: the REFERENCE's rgb_ssim (R/utils/metric_utils.py:26-79, R/ = dgmesh/) and get_psnr
(R/utils/image_utils.py:24-28) executed from their source text on synthetic image pairs.

Run from the repository root:  python tests/golden/make_metrics_golden.py   (needs the reference tree at REF below and scipy).

Pairs, at 12x43, 33x70, 161x163 and 176x162, three channels, stored as uint8 (the tests use k / 255):
  smooth   a band-limited image against a noisy copy;
  flat     two images with large exactly-flat regions at different places and levels, so that the variance clip and the sigma01 rule
           of rgb_ssim engage (recorded in `<pair>/clip`, from tests/_metrics_ref.py);
  self     the smooth image against itself                 (y is not stored: it is x);
  inverse  the smooth image against 1 - image = (255 - k) / 255, so that cs is negative and the relu of MS-SSIM engages
           (y is not stored; asserted below for the two sizes that MS-SSIM accepts).
Per pair: `ssim64` / `psnr64`, the reference on float64 tensors; `ssim32` / `psnr32`, the reference on float32 tensors, which is how
testing() (R/train.py:647-651) calls it; `ssim_fp32_err` = |ssim32 - ssim64|.  For the two sizes above 160: `msssim64`, the float64
restatement tests/_metrics_ref.ms_ssim, and `msssim_fp32_err` = |the restatement on float32 arrays - msssim64|."""
import ast
import os
import sys

import numpy as np
import scipy
import scipy.signal  # noqa: F401  (rgb_ssim calls scipy.signal.convolve2d)
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _metrics_ref as MR  # noqa: E402

REF = "/root/reference/dgmesh"
SHAPES = ((12, 43), (33, 70), (161, 163), (176, 162))
KINDS = ("smooth", "flat", "self", "inverse")


def function(path, name, ns):
    """Compile one function of the file at `path` from its source text, wherever in the module it is defined."""
    node = next(n for n in ast.walk(ast.parse(open(path).read())) if isinstance(n, ast.FunctionDef) and n.name == name)
    exec(compile(ast.Module([node], []), os.path.basename(path), "exec"), ns)
    return ns[name]


def make_pair(kind, H, W, rng):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    if kind in ("smooth", "self", "inverse"):
        x = np.stack([0.5 + 0.3 * np.sin(0.9 * xx + 0.4 * c) * np.cos(0.7 * yy - 0.3 * c) + 0.15 * np.sin(0.11 * xx * (c + 1) + 0.07 * yy)
                      for c in range(3)])
        x8 = np.clip(np.rint(x * 255), 0, 255).astype(np.uint8)
        if kind == "self":
            return x8, x8
        if kind == "inverse":
            return x8, (255 - x8).astype(np.uint8)
        y8 = np.clip(np.rint(x * 255 + rng.normal(0, 12, x.shape)), 0, 255).astype(np.uint8)
        return x8, y8
    # flat: x is grey on its left 55 % (every window there is exactly flat) and white elsewhere; y is white with a block at another
    # level and a textured stripe on the right
    x8 = np.full((3, H, W), 255, np.uint8)
    y8 = np.full((3, H, W), 255, np.uint8)
    x8[:, :, :W * 11 // 20] = np.array([128, 77, 200], np.uint8)[:, None, None]
    y8[:, H // 3:H // 3 + H // 2, W // 4:W // 4 + W // 2] = np.array([131, 60, 255], np.uint8)[:, None, None]
    stripe = rng.randint(0, 256, (3, H, max(W // 8, 2))).astype(np.uint8)
    y8[:, :, W - stripe.shape[2]:] = stripe
    return x8, y8


def main():
    rgb_ssim = function(os.path.join(REF, "utils/metric_utils.py"), "rgb_ssim", {"np": np, "scipy": scipy, "torch": torch})
    get_psnr = function(os.path.join(REF, "utils/image_utils.py"), "get_psnr", {"np": np, "torch": torch})
    rng = np.random.RandomState(7)
    rec = {"kinds": np.array(KINDS), "shapes": np.array(SHAPES, np.int64)}
    for H, W in SHAPES:
        for kind in KINDS:
            x8, y8 = make_pair(kind, H, W, rng)
            key = f"{kind}_{H}x{W}"
            if kind in ("smooth", "flat"):
                rec[key + "/x"], rec[key + "/y"] = x8, y8
            out = {}
            for dt in (torch.float64, torch.float32):  # k / 255 rounded to the dtype, (H, W, 3) as testing() passes it
                a = (torch.tensor(x8, dtype=torch.float64) / 255).to(dt).permute(1, 2, 0).contiguous()
                b = (torch.tensor(y8, dtype=torch.float64) / 255).to(dt).permute(1, 2, 0).contiguous()
                with np.errstate(divide="ignore"):
                    out[dt] = (float(rgb_ssim(a, b, 1)), float(get_psnr(a, b)))
            x64, y64 = x8.astype(np.float64) / 255, y8.astype(np.float64) / 255
            _, clip = MR.ssim(x64, y64, return_clipped=True)
            rec[key + "/ssim64"], rec[key + "/psnr64"] = np.float64(out[torch.float64][0]), np.float64(out[torch.float64][1])
            rec[key + "/ssim32"], rec[key + "/psnr32"] = np.float64(out[torch.float32][0]), np.float64(out[torch.float32][1])
            rec[key + "/ssim_fp32_err"] = np.float64(abs(out[torch.float32][0] - out[torch.float64][0]))
            rec[key + "/clip"] = np.bool_(clip)
            line = f"{key:20s} ssim64 {out[torch.float64][0]:.12f} fp32 err {rec[key + '/ssim_fp32_err']:.3e} psnr64 {out[torch.float64][1]:.6f} clip {clip}"
            if min(H, W) > 160:
                m64 = MR.ms_ssim(x64, y64)
                m32 = MR.ms_ssim(x64.astype(np.float32), y64.astype(np.float32))
                rec[key + "/msssim64"] = np.float64(m64)
                rec[key + "/msssim_fp32_err"] = np.float64(abs(np.float64(m32) - m64))
                line += f" msssim64 {m64:.12f} fp32 err {rec[key + '/msssim_fp32_err']:.3e}"
                if kind == "inverse":
                    cs, _ = MR.level_terms(x64, y64)
                    assert (cs < 0).all(), cs  # the relu engages
                    assert m64 == 0.0
            if kind == "flat":
                assert clip
            print(line)
    path = os.path.join(HERE, "metrics_small.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
