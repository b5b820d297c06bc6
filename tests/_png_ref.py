"""Test-side restatement of PNG filtering, straight from the PNG specification (section 9, "Filtering"), independent of the product's
reader and of its kernel: a per-byte unfilter, an encoder that applies a chosen filter type to every row, and a minimal file
reader / writer.  Slow by design (one Python step per byte): the test images are small."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    if pb <= pc:
        return b
    return c


def _predict(ft, a, b, c):
    if ft == 0:
        return 0
    if ft == 1:
        return a
    if ft == 2:
        return b
    if ft == 3:
        return (a + b) // 2
    if ft == 4:
        return paeth(a, b, c)
    raise ValueError(f"filter type {ft}")


def unfilter(filtered, W, H, channels):
    """filtered: H * (1 + W * channels) bytes -> (H, W, channels) uint8."""
    stride = W * channels
    data = bytes(filtered)
    assert len(data) == H * (1 + stride)
    out = [[0] * stride for _ in range(H)]
    for y in range(H):
        ft = data[y * (1 + stride)]
        row = data[y * (1 + stride) + 1:(y + 1) * (1 + stride)]
        cur, up = out[y], out[y - 1] if y else None
        for i in range(stride):
            a = cur[i - channels] if i >= channels else 0
            b = up[i] if up is not None else 0
            c = up[i - channels] if up is not None and i >= channels else 0
            cur[i] = (row[i] + _predict(ft, a, b, c)) & 255
    return np.array(out, np.uint8).reshape(H, W, channels)


def filter_rows(pixels, types):
    """pixels (H, W, channels) uint8, types: H filter types -> the filtered scanlines as bytes."""
    H, W, channels = pixels.shape
    stride = W * channels
    rows = pixels.reshape(H, stride).astype(np.int64).tolist()
    out = bytearray()
    for y in range(H):
        ft = int(types[y])
        cur, up = rows[y], rows[y - 1] if y else None
        out.append(ft)
        for i in range(stride):
            a = cur[i - channels] if i >= channels else 0
            b = up[i] if up is not None else 0
            c = up[i - channels] if up is not None and i >= channels else 0
            out.append((cur[i] - _predict(ft, a, b, c)) & 255)
    return bytes(out)


def chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def wrap_png(filtered, W, H, channels, idat_split=1, depth=8, colour=None, interlace=0):
    """A PNG file around already filtered scanlines; idat_split: the number of IDAT chunks the stream is cut into."""
    colour = {3: 2, 4: 6}[channels] if colour is None else colour
    z = zlib.compress(filtered, 6)
    cuts = [len(z) * k // idat_split for k in range(idat_split + 1)]
    body = b"".join(chunk(b"IDAT", z[cuts[k]:cuts[k + 1]]) for k in range(idat_split))
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, colour, 0, 0, interlace)) + body + chunk(b"IEND", b"")


def encode_png(pixels, types, idat_split=1):
    H, W, channels = pixels.shape
    return wrap_png(filter_rows(pixels, types), W, H, channels, idat_split)


def read_png(data):
    """-> (W, H, channels, filtered) of an 8-bit RGB / RGBA file; no checks beyond what decoding needs."""
    assert data[:8] == SIGNATURE
    pos, idat, head = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
    W, H, depth, colour = head[:4]
    assert depth == 8 and colour in (2, 6)
    return W, H, 3 if colour == 2 else 4, zlib.decompress(idat)


def decode_png(data):
    W, H, channels, filtered = read_png(data)
    return unfilter(filtered, W, H, channels)
