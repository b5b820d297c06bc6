"""Writes resample_small.npz: small RGBA images and what Pillow's Image.resize makes of them under Lanczos and bicubic, as RGBA (which
Pillow premultiplies), as RGB (the first three channels) and as a single plane (the alpha channel, mode L).  Run by hand where
Pillow is installed; neither the tests nor the product import PIL.  The file records the Pillow version it was made with.

Keys: "<W>x<H>_<ow>x<oh>/<content>/in" (H, W, 4) and "<W>x<H>_<ow>x<oh>/<content>/<filter>/<rgba | rgb | l>"."""
import os

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))

# (W, H) -> (ow, oh): the smallest real resize; a non-integer ratio with windows clipped at both edges; a Lanczos window (61 taps)
# wider than the image; 49 taps; more than a wave in both axes, odd sizes; one pass only, each way; an upscale; more than one tile
# along x; an unchanged size (a copy: no premultiply round trip)
SHAPES = [((2, 2), (1, 1)), ((9, 7), (4, 3)), ((20, 20), (2, 2)), ((64, 48), (8, 6)), ((67, 70), (33, 35)), ((16, 16), (16, 8)),
          ((16, 16), (8, 16)), ((13, 11), (20, 17)), ((300, 40), (150, 20)), ((5, 5), (5, 5))]
CONTENTS = ("noise", "smooth", "sparse_alpha")
FILTERS = {"lanczos": Image.Resampling.LANCZOS, "bicubic": Image.Resampling.BICUBIC}


def content(rng, kind, W, H):
    if kind == "smooth":
        y, x = np.mgrid[0:H, 0:W]
        chans = [np.sin(0.21 * x * (c + 1)) * 60 + np.cos(0.17 * y * (c + 2)) * 60 + 128 + rng.randint(-3, 4, (H, W)) for c in range(4)]
        return np.clip(np.stack(chans, axis=2), 0, 255).astype(np.uint8)
    px = rng.randint(0, 256, (H, W, 4)).astype(np.uint8)
    if kind == "sparse_alpha":  # both copy branches of the un-premultiply, its clamp at 255, negative accumulators from overshoot
        px[..., 3] = rng.choice(np.array([0, 1, 2, 128, 254, 255], np.uint8), (H, W))
    return px


def main():
    rng = np.random.RandomState(20240611)
    out = {"pillow_version": np.array(PIL.__version__)}
    for (W, H), (ow, oh) in SHAPES:
        for kind in CONTENTS:
            px = content(rng, kind, W, H)
            key = f"{W}x{H}_{ow}x{oh}/{kind}"
            out[key + "/in"] = px
            for fname, f in FILTERS.items():
                out[f"{key}/{fname}/rgba"] = np.asarray(Image.fromarray(px, "RGBA").resize((ow, oh), f))
                out[f"{key}/{fname}/rgb"] = np.asarray(Image.fromarray(np.ascontiguousarray(px[..., :3]), "RGB").resize((ow, oh), f))
                out[f"{key}/{fname}/l"] = np.asarray(Image.fromarray(np.ascontiguousarray(px[..., 3]), "L").resize((ow, oh), f))
    np.savez_compressed(os.path.join(HERE, "resample_small.npz"), **out)


if __name__ == "__main__":
    main()
