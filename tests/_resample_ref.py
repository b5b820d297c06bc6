"""numpy restatement of Pillow's Image.resize for 8 bits per channel (Lanczos and bicubic), one function per behaviour: the
coefficients of one axis, their fixed-point form, one pass, premultiplying and its inverse, the pass order and the copy for an
unchanged size.  tests/golden/resample_small.npz holds Pillow's own outputs; tests/test_resample.py holds this file to them bit for
bit, and the kernels (csrc/resample.hip) to this file."""
import numpy as np

PRECISION_BITS = 22
SUPPORT = {"lanczos": 3.0, "bicubic": 2.0}


def sinc(x):
    x = np.asarray(x, np.float64)
    px = x * np.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(x == 0.0, 1.0, np.sin(px) / px)


def lanczos(x):
    x = np.asarray(x, np.float64)
    return np.where((-3.0 <= x) & (x < 3.0), sinc(x) * sinc(x / 3), 0.0)


def bicubic(x):
    a = -0.5
    x = np.abs(np.asarray(x, np.float64))
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


FILTER = {"lanczos": lanczos, "bicubic": bicubic}


def float_coefficients(in_size, out_size, filter):
    """(w (out, ksize) float64, zero past each row's count and normalised; bounds (out, 2) = (xmin, count))."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = SUPPORT[filter] * fs
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    w = np.zeros((out_size, ksize), np.float64)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), in_size) - xmin
        row = FILTER[filter]((np.arange(count) + xmin - center + 0.5) * ss)
        total = 0.0
        for v in row:  # (left to right, as the C loop adds them; np.sum adds pairwise)
            total += v
        if total != 0.0:
            row = row / total
        w[xx, :count] = row
        bounds[xx] = (xmin, count)
    return w, bounds


def fixed_point(w):
    """int(w 2^22 + 0.5), or int(w 2^22 - 0.5) for negative w; int() truncates towards zero."""
    s = w * float(1 << PRECISION_BITS)
    return np.trunc(np.where(w < 0, s - 0.5, s + 0.5)).astype(np.int32)


def coefficients(in_size, out_size, filter):
    w, bounds = float_coefficients(in_size, out_size, filter)
    return fixed_point(w), bounds


def resample_axis(img, out_size, filter, axis):
    """One pass over `axis` (0 = vertical, 1 = horizontal) of an (H, W, C) uint8 image, with an int32 accumulator that wraps."""
    taps, bounds = coefficients(img.shape[axis], out_size, filter)
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for i in range(out_size):
        lo, n = bounds[i]
        with np.errstate(over="ignore"):
            acc = np.int32(1 << (PRECISION_BITS - 1)) + np.tensordot(taps[i, :n], src[lo:lo + n], axes=(0, 0)).astype(np.int32)
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def premultiply(rgba):
    """RGBA -> RGBa: c' = ((t >> 8) + t) >> 8 with t = c a + 128."""
    out = rgba.copy()
    t = rgba[..., :3].astype(np.uint32) * rgba[..., 3:4].astype(np.uint32) + 128
    out[..., :3] = ((t >> 8) + t) >> 8
    return out


def unpremultiply(rgba):
    """RGBa -> RGBA: a copy where alpha is 0 or 255, otherwise min(255, 255 c // a)."""
    out = rgba.copy()
    a = rgba[..., 3:4].astype(np.uint32)
    q = np.minimum(255, (255 * rgba[..., :3].astype(np.uint32)) // np.maximum(a, 1))
    out[..., :3] = np.where((a == 0) | (a == 255), rgba[..., :3], q)
    return out


def resize_plain(img, size, filter):
    """Horizontal pass if the width changes, then vertical pass if the height changes; (H, W, C) uint8, size = (ow, oh)."""
    ow, oh = size
    if ow != img.shape[1]:
        img = resample_axis(img, ow, filter, 1)
    if oh != img.shape[0]:
        img = resample_axis(img, oh, filter, 0)
    return img


def resize(img, size, filter, premultiplied=None):
    """Image.resize(size, filter) of an (H, W) or (H, W, C) uint8 image: a copy for an unchanged size; RGBA goes through RGBa."""
    img = np.asarray(img)
    if img.ndim == 2:
        return resize(img[..., None], size, filter, False)[..., 0]
    if tuple(size) == (img.shape[1], img.shape[0]):
        return img.copy()
    if premultiplied is None:
        premultiplied = img.shape[2] == 4
    if premultiplied:
        return unpremultiply(resize_plain(premultiply(img), size, filter))
    return resize_plain(img, size, filter)


def resize_rgba(img, size, filter="lanczos"):
    """What `downsample` does to a file's pixels: Pillow's premultiplied path for RGBA, the plain one for RGB."""
    return resize(img, size, filter)
