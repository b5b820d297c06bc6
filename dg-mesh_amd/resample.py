"""Image resizing on the device with Pillow's 8-bit arithmetic: what `downsample` (image.resize(..., LANCZOS),
R/scene/dataset_readers.py:289) and `resolution` (PILtoTorch's bicubic image.resize, R/utils/camera_utils.py:23-46,
R/utils/general_utils.py:23-29; R/ = dgmesh/) do to a frame, without an image library.

Pillow's Image.resize for 8 bits per channel, restated:
  * an unchanged size is a copy; nothing below happens;
  * RGBA is premultiplied first, c' = ((t >> 8) + t) >> 8 with t = c a + 128, and divided out last: unchanged for a = 0 or 255,
    otherwise min(255, 255 c' // a); RGB and single-plane images skip both;
  * a horizontal pass if the width changes, then a vertical pass if the height changes, with a byte image between them;
  * one axis's coefficients, in float64: scale = in / out, fs = max(scale, 1), support = S fs (S = 3 Lanczos, 2 bicubic),
    ksize = ceil(support) 2 + 1; for output xx: center = (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0),
    xmax = min(int(center + support + 0.5), in) - xmin, w[x] = filter((x + xmin - center + 0.5) (1 / fs)), summed left to right and
    divided by the sum when it is not zero; fixed point k = int(w 2^22 + 0.5), or int(w 2^22 - 0.5) for negative w;
  * an output byte is clamp((2^21 + sum pixel k) >> 22, 0, 255), int32 accumulator, arithmetic shift.
`coefficients` is the host part (a few thousand libm calls per axis); `resize` runs the passes (dgm_resample, csrc/resample.hip).
tests/golden/resample_small.npz pins the arithmetic against Pillow itself.

Modes P and 1 (palette and bilevel images: the segmentation masks of real captures) are never filtered: Image.resize replaces any
filter by NEAREST for them: an affine scaler whose source coordinate along an axis starts at 0.5 * in / out and grows by in / out per
output pixel, both in float64, each index the running sum truncated (the sum, not the product (i + 0.5) * in / out: they differ
where the product is an integer).  `nearest_indices` is that table, `resize_nearest` the gather (dgm_resample_nearest);
tests/golden/capture_small.npz pins it against Pillow."""
import ctypes
import math

import numpy as np

PRECISION_BITS = 22
FILTERS = ("lanczos", "bicubic")


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_FILTER = {"lanczos": (_lanczos, 3.0), "bicubic": (_bicubic, 2.0)}


def target_size_downsample(w, h, d):
    """(width, height) after `downsample` = d: readCamerasFromTransforms' (int(w / d), int(h / d))."""
    return int(w / d), int(h / d)


def target_size_resolution(w, h, r):
    """(width, height) after `resolution` = r, as loadCam picks it: round(w / r), round(h / r) (half to even) for r in 1, 2, 4, 8;
    otherwise (int(w / s), int(h / s)) with s = w / 1600 for r = -1 and w > 1600, s = 1 for r = -1 and w <= 1600, s = w / r else."""
    if r != -1 and not r > 0:
        raise ValueError(f"target_size_resolution: resolution must be -1 or positive, got {r}")
    if r in (1, 2, 4, 8):
        return round(w / (1.0 * r)), round(h / (1.0 * r))
    if r == -1:
        s = w / 1600 if w > 1600 else 1
    else:
        s = w / r
    s = float(s) * 1.0
    return int(w / s), int(h / s)


def coefficients(in_size, out_size, filter):
    """One axis's fixed-point taps: (taps (out_size, ksize) int32, zero past each row's count; bounds (out_size, 2) int32 =
    (first input index, count))."""
    if filter not in _FILTER:
        raise ValueError(f"coefficients: unknown filter {filter!r} (known: {list(FILTERS)})")
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"coefficients: sizes must be positive, got {in_size} -> {out_size}")
    fn, S = _FILTER[filter]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = S * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    one = float(1 << PRECISION_BITS)
    taps = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        taps[xx, :xmax] = [int(v * one - 0.5) if v < 0 else int(v * one + 0.5) for v in w]
        bounds[xx] = (xmin, xmax)
    return taps, bounds


def identity_coefficients(size):
    """Taps under which a pass copies: one tap of 2^22 per output, (2^21 + p 2^22) >> 22 = p."""
    taps = np.full((size, 1), 1 << PRECISION_BITS, np.int32)
    return taps, np.stack([np.arange(size, dtype=np.int32), np.ones(size, np.int32)], axis=1)


_TABLES = {}  # (in, out, filter, horizontal, device) -> the device tables; a scene has a handful of shapes


def _device_tables(in_size, out_size, filter, horizontal, device):
    """The tables as dgm_resample takes them (include/dgmesh_hip.h): tap-major and padded to four columns for the horizontal pass.
    filter None: identity taps.  Computed and uploaded once per key."""
    import torch
    key = (in_size, out_size, filter, horizontal, device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key in _TABLES:
        return _TABLES[key]
    taps, bounds = coefficients(in_size, out_size, filter) if filter is not None else identity_coefficients(in_size)
    ksize = taps.shape[1]
    if horizontal:
        n, ksize = taps.shape
        npad = (n + 3) & ~3
        t = np.zeros((ksize, npad), np.int32)
        t[:, :n] = taps.T
        b = np.zeros((2, npad), np.int32)
        b[:, :n] = bounds.T
        taps, bounds = t, b
    _TABLES[key] = (torch.from_numpy(np.ascontiguousarray(taps)).to(device), torch.from_numpy(np.ascontiguousarray(bounds)).to(device), ksize)
    return _TABLES[key]


def resize(pixels, size, filter, premultiplied=None, out="bytes"):
    """Image.resize(size, filter) of a batch.  pixels: (B, H, W, C) uint8 on the device, C 1, 3 or 4; size = (ow, oh);
    filter "lanczos" or "bicubic".  premultiplied: Pillow's handling of RGBA (alpha-weighted colour); None = when C is 4.  With
    premultiplied=False the four channels are resampled independently.
    out="bytes"  -> (B, oh, ow, C) uint8; an unchanged size returns `pixels` itself, without a launch, as Pillow returns a copy.
    out="planes" -> (image (B, 3, oh, ow), mask (B, oh, ow, 1)) fp32 = byte / 255 as dataset.image_ingest divides; C 3 or 4 (C = 3:
                    mask 1).  An unchanged size is a single pass with identity taps, never premultiplied."""
    import torch

    from . import _lib
    if not (torch.is_tensor(pixels) and pixels.is_cuda and pixels.dtype == torch.uint8 and pixels.dim() == 4 and pixels.shape[3] in (1, 3, 4)):
        raise RuntimeError("resize needs a (B, H, W, 1, 3 or 4) uint8 CUDA/HIP tensor (dg-mesh_amd has no CPU path for its kernels)")
    if out not in ("bytes", "planes"):
        raise ValueError(f"resize: out must be 'bytes' or 'planes', got {out!r}")
    if filter not in _FILTER:
        raise ValueError(f"resize: unknown filter {filter!r} (known: {list(FILTERS)})")
    B, H, W, C = pixels.shape
    ow, oh = (int(v) for v in size)
    if ow < 1 or oh < 1:
        raise ValueError(f"resize: size must be positive, got {(ow, oh)}")
    if premultiplied is None:
        premultiplied = C == 4
    if premultiplied and C != 4:
        raise ValueError("resize: premultiplied needs four channels")
    planes = out == "planes"
    if planes and C == 1:
        raise ValueError("resize: out='planes' needs three or four channels")
    if (ow, oh) == (W, H):
        if not planes:
            return pixels
        premultiplied = False
    pixels = pixels.contiguous()
    dev = pixels.device
    kx = bx = ky = by = None
    ksx = ksy = 0
    if ow != W:
        kx, bx, ksx = _device_tables(W, ow, filter, True, dev)
    if oh != H or kx is None:
        ky, by, ksy = _device_tables(H, oh, filter if oh != H else None, False, dev)
    tmp = torch.empty((B, H, ow, C), dtype=torch.uint8, device=dev) if (kx is not None and ky is not None) else None
    flags = (1 if premultiplied else 0) | (2 if planes else 0)
    if planes:
        image = torch.empty((B, 3, oh, ow), dtype=torch.float32, device=dev)
        mask = torch.empty((B, oh, ow, 1), dtype=torch.float32, device=dev)
        res = None
    else:
        res = torch.empty((B, oh, ow, C), dtype=torch.uint8, device=dev)
        image = mask = None
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    with _lib.device_guard(dev):
        _lib.check(_lib.lib().dgm_resample(B, H, W, C, ptr(pixels), oh, ow, ptr(kx), ptr(bx), ksx, ptr(ky), ptr(by), ksy, flags, ptr(tmp),
                                           ptr(res), ptr(image), ptr(mask), _lib.stream_ptr()))
    return (image, mask) if planes else res


def nearest_indices(in_size, out_size):
    """One axis's NEAREST source indices as Pillow's affine scaler walks them: (out_size,) int32.  In float64, s = in_size / out_size;
    the coordinate starts at 0.5 s and s is ADDED per output pixel; each index is the running sum truncated (at most in_size - 1).
    The sum is not the product (i + 0.5) s: where that product is an integer the sum can lie just below it, and Pillow takes the
    pixel before (8 -> 6, 270 -> 67, 536 -> 178 are such sizes)."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"nearest_indices: sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    out = np.empty(out_size, np.int32)
    xo = 0.5 * scale
    for i in range(out_size):
        out[i] = min(int(xo), in_size - 1)
        xo += scale
    return out


_NEAREST = {}  # (in, out, device) -> the device table


def _nearest_table(in_size, out_size, device):
    import torch
    key = (in_size, out_size, device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _NEAREST:
        _NEAREST[key] = torch.from_numpy(nearest_indices(in_size, out_size)).to(device)
    return _NEAREST[key]


def resize_nearest(pixels, size):
    """Image.resize(size) of a batch of mode P / 1 images (any filter: Pillow uses NEAREST).  pixels: (B, H, W, C) uint8 on the
    device, C 1, 3 or 4; size = (ow, oh) -> (B, oh, ow, C) uint8; an unchanged size returns `pixels` itself."""
    import torch

    from . import _lib
    if not (torch.is_tensor(pixels) and pixels.is_cuda and pixels.dtype == torch.uint8 and pixels.dim() == 4 and pixels.shape[3] in (1, 3, 4)):
        raise RuntimeError("resize_nearest needs a (B, H, W, 1, 3 or 4) uint8 CUDA/HIP tensor (dg-mesh_amd has no CPU path for its kernels)")
    B, H, W, C = pixels.shape
    ow, oh = (int(v) for v in size)
    if ow < 1 or oh < 1:
        raise ValueError(f"resize_nearest: size must be positive, got {(ow, oh)}")
    if (ow, oh) == (W, H):
        return pixels
    pixels = pixels.contiguous()
    dev = pixels.device
    xs, ys = _nearest_table(W, ow, dev), _nearest_table(H, oh, dev)
    out = torch.empty((B, oh, ow, C), dtype=torch.uint8, device=dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    with _lib.device_guard(dev):
        _lib.check(_lib.lib().dgm_resample_nearest(B, H, W, C, ptr(pixels), oh, ow, ptr(xs), ptr(ys), ptr(out), _lib.stream_ptr()))
    return out
