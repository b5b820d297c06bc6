"""Writes capture_small.npz: segmentation masks as Pillow writes them -- bilevel, grey, palette files of 1, 2, 4 and 8 bits per pixel,
RGB and RGBA -- with what Pillow reads back from them and what its Image.resize(..., LANCZOS) makes of them (NEAREST for modes P and
1, whatever filter is asked for).  Run by hand where Pillow is installed; neither the tests nor the product import PIL.  The file
records the Pillow version it was made with.

Keys:
  "file/<flavour>/<W>x<H>/png"     the file's bytes (uint8);  ".../pixels" np.asarray(Image.open(file)) (bool for mode 1);
                                   ".../gt0" the mask the readers take: pixels > 0, of the first channel for colour files
  "resize/<W>x<H>_<ow>x<oh>/<P | 1>/in", ".../out", ".../gt0"   a mode P (indices) or mode 1 (bool) image, its resize, out > 0
                                   (NEAREST: shapes where the closed form int((i + 0.5) in / out) is Pillow's index;
                                   NEAREST_SUMMED: shapes where only Pillow's running sum is)
  "scene/<flavour>/png", ".../pixels", ".../gt0", ".../half", ".../half_gt0"   48 x 40 masks for the scenes of
                                   tests/_capture_fixture.py: the file, and its resize to 24 x 20 (`half`) as a Nerfies scene with
                                   downsample = 2 resizes it
Flavours: 1, L, P256 (256-entry palette: 8 bits), P3 (3 colours: 2 bits), P16 (16 colours: 4 bits), Pbits1 (saved with bits=1), RGB,
RGBA."""
import io
import os

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))

# (W, H): row tails at every depth, more rows than a wave, no row above, no pixel to the left
SIZES = [(1, 1), (3, 5), (9, 7), (17, 1), (67, 70)]
# (W, H) -> (ow, oh) for the NEAREST resize
NEAREST = [((9, 7), (4, 3)), ((20, 20), (2, 2)), ((67, 70), (33, 35)), ((13, 11), (20, 17)), ((300, 40), (150, 20)), ((540, 960), (270, 480)),
           ((5, 5), (3, 2))]
# shapes at which (i + 0.5) * in / out is an integer for some i: Pillow's scaler ADDS in / out per output pixel, and the running sum
# lies just below such a product, so it takes the pixel before the one the closed form names
NEAREST_SUMMED = [((8, 8), (6, 7)), ((16, 24), (6, 9)), ((270, 540), (67, 135)), ((536, 960), (178, 320)), ((536, 40), (357, 27))]
FLAVOURS = ("1", "L", "P256", "P3", "P16", "Pbits1", "RGB", "RGBA")
SCENE_SIZE = (48, 40)


def palette(n, rng):
    return [int(v) for v in rng.randint(0, 256, 3 * n)]


def make(flavour, idx, rng):
    """A Pillow image of `flavour` whose first channel / index / bit is idx (H, W) -- reduced to the flavour's range."""
    H, W = idx.shape
    if flavour == "1":
        return Image.fromarray(idx % 2 == 1)
    if flavour == "L":
        return Image.fromarray((idx * 37 % 256).astype(np.uint8) * (idx > 0), "L")
    if flavour in ("P256", "P3", "P16", "Pbits1"):
        n = {"P256": 256, "P3": 3, "P16": 16, "Pbits1": 2}[flavour]
        im = Image.fromarray((idx % n).astype(np.uint8), "P")
        im.putpalette(palette(n, rng))
        return im
    px = rng.choice(np.array([0, 7, 200, 255], np.uint8), (H, W, 4))  # (few values: the file stays small)
    px[..., 0] = (idx * 53 % 255 + 1) * (idx % 4 > 0)  # (zeros in the channel that counts, anything in the others)
    return Image.fromarray(np.ascontiguousarray(px[..., :3]), "RGB") if flavour == "RGB" else Image.fromarray(px, "RGBA")


def png_bytes(im, flavour):
    buf = io.BytesIO()
    im.save(buf, "PNG", **({"bits": 1} if flavour == "Pbits1" else {}))
    return buf.getvalue()


def gt0(a):
    a = np.asarray(a)
    return (a[..., 0] if a.ndim == 3 else a) > 0


def blobs(W, H, k):
    """Object ids 0 (background), 1, 2, ...: two discs and a bar, placed by k."""
    y, x = np.mgrid[0:H, 0:W]
    idx = np.zeros((H, W), np.int64)
    idx[np.hypot(x - W * (0.35 + 0.03 * k), y - H * 0.45) < 0.28 * min(W, H)] = 1 + k % 5
    idx[np.hypot(x - W * 0.7, y - H * (0.6 - 0.02 * k)) < 0.17 * min(W, H)] = 2 + k
    idx[(abs(y - H * 0.2) < 2) & (x > W * 0.1) & (x < W * 0.8)] = 7 + k
    return idx


def main():
    rng = np.random.RandomState(20250307)
    out = {"pillow_version": np.array(PIL.__version__)}
    for W, H in SIZES:
        for flavour in FLAVOURS:
            data = png_bytes(make(flavour, rng.randint(0, 256, (H, W)), rng), flavour)
            px = np.asarray(Image.open(io.BytesIO(data)))
            key = f"file/{flavour}/{W}x{H}"
            out[key + "/png"], out[key + "/pixels"], out[key + "/gt0"] = np.frombuffer(data, np.uint8), px, gt0(px)
    nearest(out, rng, NEAREST)
    scenes(out, rng)
    nearest(out, np.random.RandomState(20250308), NEAREST_SUMMED)  # (its own stream: the entries above stay as they were)
    np.savez_compressed(os.path.join(HERE, "capture_small.npz"), **out)


def nearest(out, rng, shapes):
    for (W, H), (ow, oh) in shapes:
        y, x = np.mgrid[0:H, 0:W]
        # every pixel differs from its neighbours, so a wrong source index shows; periodic, so the large shape compresses
        idx = ((x * 3 + y * 5) % 64 * 4 + 1 if W * H > 10000 else rng.randint(0, 256, (H, W))).astype(np.uint8)
        idx[H // 2:, :W // 3] = 0
        p = Image.fromarray(idx, "P")
        p.putpalette(palette(256, rng))
        bits = (x * 3 + y * 5) % 7 < 3 if W * H > 10000 else rng.randint(0, 2, (H, W)).astype(bool)
        for name, im in (("P", p), ("1", Image.fromarray(bits))):
            res = np.asarray(im.resize((ow, oh), Image.Resampling.LANCZOS))
            key = f"resize/{W}x{H}_{ow}x{oh}/{name}"
            out[key + "/in"], out[key + "/out"], out[key + "/gt0"] = np.asarray(im), res, gt0(res)


def scenes(out, rng):
    W, H = SCENE_SIZE
    for k, flavour in enumerate(FLAVOURS):
        data = png_bytes(make(flavour, blobs(W, H, k), rng), flavour)
        im = Image.open(io.BytesIO(data))
        half = np.asarray(im.resize((int(W / 2.0), int(H / 2.0)), Image.Resampling.LANCZOS))
        key = f"scene/{flavour}"
        out[key + "/png"], out[key + "/pixels"], out[key + "/gt0"] = np.frombuffer(data, np.uint8), np.asarray(im), gt0(np.asarray(im))
        out[key + "/half"], out[key + "/half_gt0"] = half, gt0(half)


if __name__ == "__main__":
    main()
