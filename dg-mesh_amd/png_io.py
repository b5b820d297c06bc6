"""PNG writer for the frames of visualize.py: 8-bit RGB, no interlace, filter type 0 on every row, one IDAT chunk.  Standard
library only (zlib + struct) -- imageio, PIL and cv2 are not dependencies.

PNG reader for dataset.py: parse_png checks a file and inflates its IDAT stream on the host (zlib, at C speed); the byte-serial
part of decoding -- undoing the per-row filters -- runs on the device (decode_pngs -> dgm_png_unfilter, csrc/ingest.hip).  8-bit
RGB and RGBA without interlace, which is what the Blender / D-NeRF scenes ship; anything else is refused by name."""
import ctypes
import os
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_WORKERS = 8


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


def parse_png(src):
    """src: a path or the file's bytes -> (W, H, channels, filtered): `filtered` is the inflated IDAT stream, H rows of
    1 + W * channels bytes, each led by its filter type (0..4, checked here).  ValueError, naming the file and the reason, for
    anything but an intact 8-bit RGB / RGBA PNG without interlace."""
    if isinstance(src, (bytes, bytearray, memoryview)):
        name, data = "<bytes>", bytes(src)
    else:
        name = os.fspath(src)
        with open(name, "rb") as fh:
            data = fh.read()

    def bad(why):
        return ValueError(f"parse_png: {name}: {why}")

    if data[:8] != SIGNATURE:
        raise bad("not a PNG file (bad signature)")
    pos, header, idat, ended = 8, None, [], False
    while pos < len(data):
        if pos + 8 > len(data):
            raise bad("truncated (chunk header cut short)")
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        if pos + 12 + n > len(data):
            raise bad(f"truncated (chunk {tag!r} cut short)")
        body = data[pos + 8:pos + 8 + n]
        if zlib.crc32(tag + body) & 0xFFFFFFFF != struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]:
            raise bad(f"bad CRC in chunk {tag!r}")
        pos += 12 + n
        if header is None and tag != b"IHDR":
            raise bad("the first chunk is not IHDR")
        if tag == b"IHDR":
            if n != 13:
                raise bad("IHDR is not 13 bytes")
            header = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            ended = True
            break
    if header is None or not ended:
        raise bad("truncated (no IEND chunk)")
    W, H, depth, colour, compression, filter_method, interlace = header
    if W < 1 or H < 1:
        raise bad(f"empty image {W}x{H}")
    if interlace != 0:
        raise bad("interlaced (Adam7) files are not supported")
    if depth != 8:
        raise bad(f"bit depth {depth} is not supported (8 only)")
    if colour not in (2, 6):
        raise bad(f"colour type {colour} is not supported (2 = RGB and 6 = RGBA only)")
    if compression != 0 or filter_method != 0:
        raise bad("unknown compression or filter method")
    channels = 3 if colour == 2 else 4
    try:
        filtered = zlib.decompress(b"".join(idat))
    except zlib.error as e:
        raise bad(f"truncated or corrupt IDAT stream ({e})") from None
    stride = 1 + W * channels
    if len(filtered) != H * stride:
        raise bad(f"the IDAT stream inflates to {len(filtered)} bytes, not H * (1 + W * channels) = {H * stride}")
    types = np.frombuffer(filtered, np.uint8)[::stride]
    if types.max() > 4:
        row = int(np.argmax(types > 4))
        raise bad(f"bad filter type {int(types[row])} on row {row}")
    return W, H, channels, filtered


def unfilter(filtered, B, W, H, channels):
    """dgm_png_unfilter: `filtered` a uint8 device tensor of B * H * (1 + W * channels) bytes -> (B, H, W, channels) uint8."""
    import torch

    from . import _lib
    if not (torch.is_tensor(filtered) and filtered.is_cuda and filtered.dtype == torch.uint8 and filtered.is_contiguous()):
        raise RuntimeError("unfilter needs a contiguous uint8 CUDA/HIP tensor (dg-mesh_amd has no CPU path for its kernels)")
    if filtered.numel() != B * H * (1 + W * channels):
        raise ValueError(f"unfilter: {filtered.numel()} bytes for B={B} H={H} W={W} channels={channels}")
    out = torch.empty((B, H, W, channels), dtype=torch.uint8, device=filtered.device)
    with _lib.device_guard(filtered.device):
        _lib.check(_lib.lib().dgm_png_unfilter(B, W, H, channels, ctypes.c_void_p(filtered.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                               _lib.stream_ptr()))
    return out


def decode_png_groups(paths, device):
    """The files' pixels, grouped by (W, H, channels): a list of (indices, batch), `indices` the positions in `paths` of the
    files of one shape, in order, and `batch` their (len(indices), H, W, C) uint8 device tensor.  The files are inflated on a pool
    of at most MAX_WORKERS threads (zlib releases the GIL); each group has one page-locked staging buffer, one upload and one
    dgm_png_unfilter call."""
    import torch
    paths = list(paths)
    if not paths:
        raise ValueError("decode_pngs: no files")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("decode_pngs needs a CUDA/HIP device (dg-mesh_amd has no CPU path for its kernels)")
    groups, out = {}, []
    with ThreadPoolExecutor(max_workers=min(MAX_WORKERS, len(paths))) as pool:
        parsed = list(pool.map(parse_png, paths))
        for i, (W, H, ch, _) in enumerate(parsed):
            groups.setdefault((W, H, ch), []).append(i)
        for (W, H, ch), idx in groups.items():
            # each file's scanlines are copied into their slot of the staging buffer once, by the pool
            n = H * (1 + W * ch)
            host = torch.empty(len(idx) * n, dtype=torch.uint8, pin_memory=True)
            slots = host.numpy().reshape(len(idx), n)

            def fill(k, i):
                slots[k] = np.frombuffer(parsed[i][3], np.uint8)
                parsed[i] = None
            list(pool.map(fill, range(len(idx)), idx))
            out.append((idx, unfilter(host.to(device), len(idx), W, H, ch)))
    return out


def decode_pngs(paths, device):
    """(B, H, W, C) uint8 device tensor of files of ONE shape, in the order of `paths` (decode_png_groups takes mixed shapes)."""
    groups = decode_png_groups(paths, device)
    if len(groups) != 1:
        shapes = sorted(tuple(b.shape[1:]) for _, b in groups)
        raise ValueError(f"decode_pngs: the files have {len(groups)} shapes {shapes}; decode_png_groups returns one batch per shape")
    return groups[0][1]
