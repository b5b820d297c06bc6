"""Writes png_small.npz: a handful of small RGBA and RGB PNG files encoded by PIL (an encoder independent of this project), as raw
file bytes, with the pixel arrays they were made from.  Run by hand where PIL is installed; neither the tests nor the product
import PIL."""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def smooth(rng, H, W, C):
    """Smooth ramps plus a little noise, so that PIL's adaptive encoder picks Sub, Up, Average and Paeth rows."""
    y, x = np.mgrid[0:H, 0:W]
    chans = [(np.sin(0.21 * x * (c + 1)) * 60 + np.cos(0.17 * y * (c + 2)) * 60 + 128 + rng.randint(-3, 4, (H, W))) for c in range(C)]
    return np.clip(np.stack(chans, axis=2), 0, 255).astype(np.uint8)


def main():
    rng = np.random.RandomState(20240607)
    cases = {
        "rgba_smooth_70x67": smooth(rng, 67, 70, 4),
        "rgb_smooth_33x19": smooth(rng, 19, 33, 3),
        "rgba_noise_17x5": rng.randint(0, 256, (5, 17, 4)).astype(np.uint8),
        "rgb_flat_9x9": np.full((9, 9, 3), 200, np.uint8),
        "rgba_1x1": rng.randint(0, 256, (1, 1, 4)).astype(np.uint8),
    }
    a = smooth(rng, 40, 48, 4)
    yy, xx = np.mgrid[0:40, 0:48]
    a[..., 3] = np.where((xx - 24) ** 2 + (yy - 20) ** 2 < 200, 255, 0)
    a[..., 3][(xx + yy) % 7 == 0] = 128
    cases["rgba_cutout_48x40"] = a
    out = {}
    for name, px in cases.items():
        buf = io.BytesIO()
        Image.fromarray(px, "RGBA" if px.shape[2] == 4 else "RGB").save(buf, format="PNG", optimize=(px.shape[0] % 2 == 0))
        out[name + "/png"] = np.frombuffer(buf.getvalue(), np.uint8)
        out[name + "/pixels"] = px
    np.savez_compressed(os.path.join(HERE, "png_small.npz"), **out)


if __name__ == "__main__":
    main()
