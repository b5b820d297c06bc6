"""Times loading a scene's frames (png_io.decode_pngs + dataset.image_ingest, csrc/ingest.hip) on the GPU and prints one JSON line.

  python tools/ingest_bench.py [--frames 200] [--size 800] [--distinct 8] [--iters 5]

`frames` synthetic size x size RGBA PNGs (`distinct` different images, repeated), rendering-like content with every row's filter
type drawn from all five, held in memory:
  * `inflate_ms`: the host part of decode_pngs -- parse_png (CRC, inflate, checks) over its thread pool -- wall clock, all frames;
  * `stage_ms`: a page-locked buffer allocated and the scanlines copied into it; `upload_ms`: that buffer to the device;
  * `unfilter_ms`, `ingest_ms`: HIP events around dgm_png_unfilter and dgm_image_ingest for all frames, median of `iters`;
  * `ingest_GBps`: 20 bytes per pixel (4 in, 16 out) over ingest_ms.
  * `lanczos_ms`: the frames halved (size -> size // 2) by resample.resize, Lanczos through Pillow's premultiplied RGBA path (two
    launches of csrc/resample.hip), HIP events, median of `iters`; `lanczos_GBps`: bytes read and written by the two passes
    (in + 2 x intermediate + out) over it; `pillow_lanczos_ms`: Image.resize of the same frames on one host thread, wall clock,
    when Pillow imports (null otherwise); the device result of every distinct frame is compared with Pillow's.  Informational.
The decoded pixels are compared with the images the files were made from.  No GPU: the script fails; it never falls back."""
import argparse
import importlib
import json
import os
import statistics
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = lambda n: importlib.import_module("dg-mesh_amd." + n)


def picture(size, seed):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:size, 0:size].astype(np.float32)
    r = np.hypot(x - size / 2 + 40 * rng.rand(), y - size / 2 + 40 * rng.rand()) / (0.3 * size)
    alpha = np.clip((1.0 - r) / 0.02, 0, 1)
    rgb = [np.clip(200 - 120 * r + 30 * np.sin(0.05 * (k + 1) * x + seed) + rng.randint(-2, 3, x.shape), 0, 255) for k in range(3)]
    return np.stack(rgb + [255 * alpha], axis=2).astype(np.uint8)


def filter_rows(px, types):
    """PNG filtering (specification section 9) of (H, W, C) uint8 with one filter type per row, vectorised."""
    H, W, C = px.shape
    cur = px.reshape(H, W * C).astype(np.int32)
    a = np.zeros_like(cur)
    a[:, C:] = cur[:, :-C]
    b = np.zeros_like(cur)
    b[1:] = cur[:-1]
    c = np.zeros_like(cur)
    c[1:, C:] = cur[:-1, :-C]
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    pred = np.stack([np.zeros_like(cur), a, b, (a + b) // 2, paeth])[np.asarray(types), np.arange(H)]
    out = np.empty((H, 1 + W * C), np.uint8)
    out[:, 0] = types
    out[:, 1:] = (cur - pred) & 255
    return out.tobytes()


def png_bytes(px, types):
    chunk = lambda tag, d: struct.pack(">I", len(d)) + tag + d + struct.pack(">I", zlib.crc32(tag + d) & 0xFFFFFFFF)
    H, W, C = px.shape
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 6 if C == 4 else 2, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(filter_rows(px, types), 6)) + chunk(b"IEND", b""))


def timed(fn, iters):
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ingest_bench needs a GPU"
    P, D = pkg("png_io"), pkg("dataset")
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    pictures = [picture(args.size, k) for k in range(min(args.distinct, args.frames))]
    files = [png_bytes(p, rng.randint(0, 5, args.size)) for p in pictures]
    frames = [files[k % len(files)] for k in range(args.frames)]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=min(P.MAX_WORKERS, len(frames))) as pool:
        parsed = list(pool.map(P.parse_png, frames))
    inflate_ms = (time.perf_counter() - t0) * 1e3
    W, H, C, _ = parsed[0]
    B, n = len(frames), H * (1 + W * C)
    t0 = time.perf_counter()  # as decode_pngs stages them: one page-locked buffer, each frame copied into its slot by the pool
    host = torch.empty(B * n, dtype=torch.uint8, pin_memory=True)
    slots = host.numpy().reshape(B, n)

    def fill(k):
        slots[k] = np.frombuffer(parsed[k][3], np.uint8)
    with ThreadPoolExecutor(max_workers=min(P.MAX_WORKERS, B)) as pool:
        list(pool.map(fill, range(B)))
    stage_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    filtered = host.to(dev)
    torch.cuda.synchronize()
    upload_ms = (time.perf_counter() - t0) * 1e3
    P.unfilter(filtered, B, W, H, C)  # (warm-up)
    unfilter_ms, pixels = timed(lambda: P.unfilter(filtered, B, W, H, C), args.iters)
    D.image_ingest(pixels, [1.0, 1.0, 1.0])
    ingest_ms, (image, mask) = timed(lambda: D.image_ingest(pixels, [1.0, 1.0, 1.0]), args.iters)
    for k in range(len(files)):
        assert np.array_equal(pixels[k].cpu().numpy(), pictures[k]), f"frame {k} decoded wrongly"
    RS = pkg("resample")
    half = (W // 2, H // 2)
    RS.resize(pixels, half, "lanczos")  # (warm-up; the coefficient tables are computed and uploaded here)
    lanczos_ms, small = timed(lambda: RS.resize(pixels, half, "lanczos"), args.iters)
    lanczos_bytes = B * C * (W * H + 2 * half[0] * H + half[0] * half[1])
    pillow_ms = None
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        want = [np.asarray(Image.fromarray(p, "RGBA").resize(half, Image.Resampling.LANCZOS)) for p in pictures]
        t0 = time.perf_counter()
        for k in range(B):
            Image.fromarray(pictures[k % len(pictures)], "RGBA").resize(half, Image.Resampling.LANCZOS)
        pillow_ms = (time.perf_counter() - t0) * 1e3
        for k in range(len(pictures)):
            assert np.array_equal(small[k].cpu().numpy(), want[k]), f"frame {k} resized differently from Pillow"
    print(json.dumps({"frames": B, "size": [W, H], "channels": C, "file_MB": sum(len(f) for f in frames) / 1e6,
                      "inflate_ms": inflate_ms, "inflate_workers": min(P.MAX_WORKERS, B), "stage_ms": stage_ms, "upload_ms": upload_ms,
                      "unfilter_ms": unfilter_ms, "ingest_ms": ingest_ms, "ingest_GBps": B * W * H * 20 / (ingest_ms * 1e-3) / 1e9,
                      "unfilter_GBps": B * W * H * C * 2 / (unfilter_ms * 1e-3) / 1e9, "lanczos_size": list(half), "lanczos_ms": lanczos_ms,
                      "lanczos_GBps": lanczos_bytes / (lanczos_ms * 1e-3) / 1e9, "pillow_lanczos_ms": pillow_ms}))


if __name__ == "__main__":
    main()
