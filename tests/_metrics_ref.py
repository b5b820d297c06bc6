"""numpy restatement of the test-view image metrics (dgm_image_metrics, include/dgmesh_hip.h): MSE / PSNR, SSIM in the rgb_ssim
definition, and MS-SSIM with the defaults of the pytorch_msssim package stated in this project's own words (that package is not a
dependency).  Images are (C, H, W).  Every function computes in the dtype of its inputs: float64 arrays give the reference the GPU
tests compare against, float32 arrays give the fp32 deviation that tests/golden/make_metrics_golden.py records as a yardstick."""
import numpy as np

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
WIN = 11


def window(dtype=np.float64):
    g = np.exp(-((np.arange(WIN) - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    return (g / g.sum()).astype(dtype)


def blur_valid(z):
    """Separable 11-tap window, no padding: (..., H, W) -> (..., H - 10, W - 10), taps accumulated in ascending order."""
    g = window(z.dtype)
    H, W = z.shape[-2:]
    h = np.zeros(z.shape[:-1] + (W - 10,), z.dtype)
    for k in range(WIN):
        h = h + g[k] * z[..., :, k:k + W - 10]
    v = np.zeros(z.shape[:-2] + (H - 10, W - 10), z.dtype)
    for k in range(WIN):
        v = v + g[k] * h[..., k:k + H - 10, :]
    return v


def moments(x, y):
    mu0, mu1 = blur_valid(x), blur_valid(y)
    s00 = blur_valid(x * x) - mu0 * mu0
    s11 = blur_valid(y * y) - mu1 * mu1
    s01 = blur_valid(x * y) - mu0 * mu1
    return mu0, mu1, s00, s11, s01


def mse(x, y):
    return np.mean((x - y) ** 2)


def psnr(x, y):
    with np.errstate(divide="ignore"):
        return -10.0 * np.log10(mse(x, y))


def ssim(x, y, data_range=1.0, return_clipped=False):
    """rgb_ssim: clipped variances, |s01| bounded by sqrt(s00 s11); mean over pixels and channels."""
    c1, c2 = x.dtype.type((0.01 * data_range) ** 2), x.dtype.type((0.03 * data_range) ** 2)
    mu0, mu1, s00, s11, s01 = moments(x, y)
    c00, c11 = np.maximum(0, s00), np.maximum(0, s11)
    c01 = np.sign(s01) * np.minimum(np.sqrt(c00 * c11), np.abs(s01))
    m = ((2 * mu0 * mu1 + c1) * (2 * c01 + c2)) / ((mu0 * mu0 + mu1 * mu1 + c1) * (c00 + c11 + c2))
    if return_clipped:
        return m.mean(), bool((s00 < 0).any() or (s11 < 0).any() or (c01 != s01).any())
    return m.mean()


def level_terms(x, y, data_range=1.0):
    """-> (cs, ssim_l), each (C,): the per-channel means of one MS-SSIM level, variances not clipped."""
    c1, c2 = x.dtype.type((0.01 * data_range) ** 2), x.dtype.type((0.03 * data_range) ** 2)
    mu0, mu1, s00, s11, s01 = moments(x, y)
    cs = (2 * s01 + c2) / (s00 + s11 + c2)
    sl = ((2 * mu0 * mu1 + c1) / (mu0 * mu0 + mu1 * mu1 + c1)) * cs
    return cs.mean(axis=(-2, -1)), sl.mean(axis=(-2, -1))


def pool(z):
    """2x2 average, stride 2; an odd side is zero-padded by one on both ends and the divisor stays 4."""
    H, W = z.shape[-2:]
    ph, pw = H % 2, W % 2
    zp = np.zeros(z.shape[:-2] + (H + 2 * ph, W + 2 * pw), z.dtype)
    zp[..., ph:ph + H, pw:pw + W] = z
    Ho, Wo = (H + 2 * ph) // 2, (W + 2 * pw) // 2
    zp = zp[..., :2 * Ho, :2 * Wo]
    return ((zp[..., 0::2, 0::2] + zp[..., 0::2, 1::2]) + (zp[..., 1::2, 0::2] + zp[..., 1::2, 1::2])) * z.dtype.type(0.25)


def pooled_sizes(s, levels=5):
    out = [s]
    for _ in range(levels - 1):
        out.append(out[-1] // 2 + out[-1] % 2)
    return out


def ms_ssim(x, y, data_range=1.0):
    if min(x.shape[-2:]) <= 160:
        raise ValueError("ms_ssim needs min(H, W) > 160")
    w = np.asarray(WEIGHTS, x.dtype)
    prod = np.ones(x.shape[0], x.dtype)
    for l in range(5):
        cs, sl = level_terms(x, y, data_range)
        prod = prod * np.maximum(cs if l < 4 else sl, 0) ** w[l]
        if l < 4:
            x, y = pool(x), pool(y)
    return prod.mean()
