"""Times loading a real capture's frames and masks (png_io.decode_png_groups / decode_mask_groups + dataset.image_ingest_masked,
csrc/ingest.hip) on the GPU and prints one JSON line.  Split as tools/ingest_bench.py splits a Blender scene's load:

  python tools/capture_bench.py [--frames 200] [--width 960] [--height 720] [--distinct 8] [--iters 5]

`frames` synthetic RGB PNGs and as many 2-bit palette masks (three object ids, what Pillow writes for a three-colour P image), held
in memory:
  * `inflate_ms`: parse_png over the frames and parse_png_any over the masks on the thread pool, wall clock;
  * `upload_ms`: both staged buffers to the device;
  * `unfilter_ms`: dgm_png_unfilter of the frames (3 bytes per pixel) and of the masks' packed rows (1 byte per pixel);
    `expand_ms`: dgm_png_expand of the masks; `ingest_ms`: dgm_image_ingest_masked; HIP events, median of `iters`;
  * `ingest_GBps`: 20 bytes per pixel (3 + 1 in, 16 out) over ingest_ms.
The decoded frames, masks and the composite of every distinct frame are compared with the arrays the files were made from.
Informational; no GPU: the script fails."""
import argparse
import json
import os
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ingest_bench import filter_rows, pkg, png_bytes, timed  # noqa: E402


def scene(W, H, seed):
    """(frame (H, W, 3), object ids (H, W) in 0..2) of one synthetic view."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    r = np.hypot(x - W / 2 + 40 * rng.rand(), y - H / 2 + 40 * rng.rand()) / (0.3 * H)
    rgb = [np.clip(200 - 120 * r + 30 * np.sin(0.05 * (k + 1) * x + seed) + rng.randint(-2, 3, x.shape), 0, 255) for k in range(3)]
    ids = np.where(r < 0.6, 1, np.where(r < 1.0, 2, 0)).astype(np.uint8)
    return np.stack(rgb, axis=2).astype(np.uint8), ids


def palette_png(ids, types, depth=2):
    """A colour-type-3 PNG of `depth` bits per pixel around the indices, rows filtered as bytes."""
    H, W = ids.shape
    per = 8 // depth
    padded = np.zeros((H, -(-W // per) * per), np.uint8)
    padded[:, :W] = ids
    packed = np.zeros((H, padded.shape[1] // per), np.uint8)
    for k in range(per):
        packed |= padded[:, k::per] << (8 - depth * (k + 1))
    chunk = lambda tag, d: struct.pack(">I", len(d)) + tag + d + struct.pack(">I", zlib.crc32(tag + d) & 0xFFFFFFFF)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, 3, 0, 0, 0)) + chunk(b"PLTE", bytes(range(9)))
            + chunk(b"IDAT", zlib.compress(filter_rows(packed[..., None], types), 6)) + chunk(b"IEND", b""))


def staged(parsed):
    host = torch.empty(sum(len(p[-1]) for p in parsed), dtype=torch.uint8, pin_memory=True)
    host.numpy()[:] = np.frombuffer(b"".join(p[-1] for p in parsed), np.uint8)
    return host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "capture_bench needs a GPU"
    P, D = pkg("png_io"), pkg("dataset")
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    W, H, B = a.width, a.height, a.frames
    views = [scene(W, H, k) for k in range(min(a.distinct, B))]
    frame_files = [png_bytes(f, rng.randint(0, 5, H)) for f, _ in views]
    mask_files = [palette_png(m, rng.randint(0, 5, H)) for _, m in views]
    pick = lambda files: [files[k % len(files)] for k in range(B)]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=min(P.MAX_WORKERS, B)) as pool:
        frames = list(pool.map(P.parse_png, pick(frame_files)))
        masks = list(pool.map(P.parse_png_any, pick(mask_files)))
    inflate_ms = (time.perf_counter() - t0) * 1e3
    rb, depth = masks[0][4], masks[0][3]
    hf, hm = staged(frames), staged(masks)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ff, fm = hf.to(dev), hm.to(dev)
    torch.cuda.synchronize()
    upload_ms = (time.perf_counter() - t0) * 1e3
    unf = lambda: (P.unfilter(ff, B, W, H, 3), P.unfilter(fm, B, rb, H, 1).reshape(B, H, rb))
    unf()
    unfilter_ms, (pixels, packed) = timed(unf, a.iters)
    P.expand(packed, W, depth, 1)
    expand_ms, ids = timed(lambda: P.expand(packed, W, depth, 1), a.iters)
    D.image_ingest_masked(pixels, ids, [1.0, 1.0, 1.0])
    ingest_ms, (image, alpha) = timed(lambda: D.image_ingest_masked(pixels, ids, [1.0, 1.0, 1.0]), a.iters)
    for k, (f, m) in enumerate(views):
        assert np.array_equal(pixels[k].cpu().numpy(), f) and np.array_equal(ids[k, :, :, 0].cpu().numpy(), m), f"frame {k} decoded wrongly"
        want = np.where((m > 0)[..., None], f, 255).astype(np.float32) / np.float32(255.0)
        assert np.array_equal(image[k].cpu().numpy(), want.transpose(2, 0, 1)) and np.array_equal(alpha[k, :, :, 0].cpu().numpy() > 0, m > 0)
    print(json.dumps({"frames": B, "size": [W, H], "mask_depth": depth, "file_MB": sum(map(len, pick(frame_files) + pick(mask_files))) / 1e6,
                      "inflate_ms": inflate_ms, "inflate_workers": min(P.MAX_WORKERS, B), "upload_ms": upload_ms, "unfilter_ms": unfilter_ms,
                      "expand_ms": expand_ms, "ingest_ms": ingest_ms, "ingest_GBps": B * W * H * 20 / (ingest_ms * 1e-3) / 1e9}))


if __name__ == "__main__":
    main()
