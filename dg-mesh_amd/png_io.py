"""PNG writer for the frames of visualize.py: 8-bit RGB, no interlace, filter type 0 on every row, one IDAT chunk.  Standard
library only (zlib + struct) -- imageio, PIL and cv2 are not dependencies."""
import os
import struct
import zlib

import numpy as np


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, image, compress_level=6):
    """image: (H, W, 3) uint8 (a numpy array, or anything np.asarray takes)."""
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png: image must be (H, W, 3) uint8, got {a.dtype} {a.shape}")
    H, W = a.shape[:2]
    rows = np.zeros((H, 1 + W * 3), np.uint8)  # (a leading 0 per row: filter type None)
    rows[:, 1:] = a.reshape(H, W * 3)
    data = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(rows.tobytes(), compress_level)) + _chunk(b"IEND", b""))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(data)
