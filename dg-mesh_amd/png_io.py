"""PNG writer for the frames of visualize.py: 8-bit RGB, no interlace, filter type 0 on every row, one IDAT chunk.  Standard
library only (zlib + struct) -- imageio, PIL and cv2 are not dependencies.

PNG reader for dataset.py: parse_png checks a file and inflates its IDAT stream on the host (zlib, at C speed); the byte-serial
part of decoding -- undoing the per-row filters -- runs on the device (decode_pngs -> dgm_png_unfilter, csrc/ingest.hip).  8-bit
RGB and RGBA without interlace, which is what the Blender / D-NeRF scenes ship; anything else is refused by name.

The segmentation masks of real captures (captures.py) are palette, grey and bilevel files, often of 1, 2 or 4 bits per pixel:
parse_png_any reads those as well, decode_mask_groups unfilters their packed rows as bytes (the PNG filters of a sub-byte image work
on whole bytes) and dgm_png_expand turns them into one byte per pixel, with Pillow's scaling of grey samples."""
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


def encode_png(image, compress_level=6):
    """The bytes of write_png's file.  image: (H, W, 3) uint8 (a numpy array, or anything np.asarray takes)."""
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png: image must be (H, W, 3) uint8, got {a.dtype} {a.shape}")
    H, W = a.shape[:2]
    rows = np.zeros((H, 1 + W * 3), np.uint8)  # (a leading 0 per row: filter type None)
    rows[:, 1:] = a.reshape(H, W * 3)
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(rows.tobytes(), compress_level)) + _chunk(b"IEND", b""))


def write_png(path, image, compress_level=6):
    """image: (H, W, 3) uint8 (a numpy array, or anything np.asarray takes)."""
    data = encode_png(image, compress_level)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(data)


def _read_chunks(src, who):
    """-> (name, bad, IHDR fields, joined IDAT bytes, whether a PLTE chunk was seen) of an intact chunk sequence."""
    if isinstance(src, (bytes, bytearray, memoryview)):
        name, data = "<bytes>", bytes(src)
    else:
        name = os.fspath(src)
        with open(name, "rb") as fh:
            data = fh.read()

    def bad(why):
        return ValueError(f"{who}: {name}: {why}")

    if data[:8] != SIGNATURE:
        raise bad("not a PNG file (bad signature)")
    pos, header, idat, ended, palette = 8, None, [], False, False
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
        elif tag == b"PLTE":
            palette = True
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            ended = True
            break
    if header is None or not ended:
        raise bad("truncated (no IEND chunk)")
    return name, bad, header, b"".join(idat), palette


def _inflate_rows(bad, idat, H, row_bytes, what):
    """The inflated IDAT stream, H rows of 1 + row_bytes bytes, with its length and filter types checked."""
    try:
        filtered = zlib.decompress(idat)
    except zlib.error as e:
        raise bad(f"truncated or corrupt IDAT stream ({e})") from None
    stride = 1 + row_bytes
    if len(filtered) != H * stride:
        raise bad(f"the IDAT stream inflates to {len(filtered)} bytes, not H * (1 + {what}) = {H * stride}")
    types = np.frombuffer(filtered, np.uint8)[::stride]
    if types.max() > 4:
        row = int(np.argmax(types > 4))
        raise bad(f"bad filter type {int(types[row])} on row {row}")
    return filtered


def parse_png(src):
    """src: a path or the file's bytes -> (W, H, channels, filtered): `filtered` is the inflated IDAT stream, H rows of
    1 + W * channels bytes, each led by its filter type (0..4, checked here).  ValueError, naming the file and the reason, for
    anything but an intact 8-bit RGB / RGBA PNG without interlace."""
    name, bad, header, idat, _ = _read_chunks(src, "parse_png")
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
    return W, H, channels, _inflate_rows(bad, idat, H, W * channels, "W * channels")


_ANY_CHANNELS = {0: 1, 3: 1, 2: 3, 6: 4}


def parse_png_any(src):
    """parse_png for the files masks come in as well: -> (W, H, colour, depth, row_bytes, bpp, filtered).  Colour types 0 (grey)
    and 3 (palette; a PLTE chunk must be there, its entries are not needed: a mask is tested against index 0) at bit depths 1, 2,
    4 and 8; 2 (RGB) and 6 (RGBA) at depth 8.  row_bytes = ceil(W * channels * depth / 8), bpp = max(1, channels * depth / 8) =
    the distance in bytes between a byte and its `left` neighbour under the PNG filters; `filtered`: H rows of 1 + row_bytes bytes.
    ValueError by name for 16-bit samples, grey + alpha (type 4), interlace, a bad CRC or filter byte, a cut file."""
    name, bad, header, idat, palette = _read_chunks(src, "parse_png_any")
    W, H, depth, colour, compression, filter_method, interlace = header
    if W < 1 or H < 1:
        raise bad(f"empty image {W}x{H}")
    if interlace != 0:
        raise bad("interlaced (Adam7) files are not supported")
    if colour == 4:
        raise bad("colour type 4 (grey + alpha) is not supported (0 = grey, 2 = RGB, 3 = palette and 6 = RGBA only)")
    if colour not in _ANY_CHANNELS:
        raise bad(f"colour type {colour} is not supported (0 = grey, 2 = RGB, 3 = palette and 6 = RGBA only)")
    if depth == 16:
        raise bad("bit depth 16 is not supported (1, 2, 4 and 8 for grey and palette files, 8 for RGB and RGBA)")
    if depth not in ((1, 2, 4, 8) if colour in (0, 3) else (8,)):
        raise bad(f"bit depth {depth} is not supported for colour type {colour}")
    if compression != 0 or filter_method != 0:
        raise bad("unknown compression or filter method")
    if colour == 3 and not palette:
        raise bad("a palette file (colour type 3) without a PLTE chunk")
    channels = _ANY_CHANNELS[colour]
    row_bytes = (W * channels * depth + 7) // 8
    return W, H, colour, depth, row_bytes, max(1, channels * depth // 8), _inflate_rows(bad, idat, H, row_bytes, "row bytes")


def read_png_host(src):
    """src: a path or the file's bytes -> (H, W, channels) uint8 numpy array of an 8-bit RGB / RGBA PNG, decoded on the host.  For the
    small files this project writes itself (write_png: filter type 0 on every row, one reshape); rows with other filter types are
    unfiltered one by one in numpy -- Sub, Average and Paeth byte by byte, so a large foreign file is slow.  The dataset path is
    decode_pngs."""
    W, H, ch, filtered = parse_png(src)
    rows = np.frombuffer(filtered, np.uint8).reshape(H, 1 + W * ch)
    types, out = rows[:, 0], rows[:, 1:].copy()
    if not types.any():
        return out.reshape(H, W, ch)
    zero = np.zeros(W * ch, np.uint8)
    for y in range(H):
        t, up = int(types[y]), (out[y - 1] if y else zero)
        if t == 2:
            out[y] += up
        elif t:
            cur, upi = out[y].astype(np.int64), up.astype(np.int64)
            for x in range(W * ch):
                a = cur[x - ch] if x >= ch else 0
                b, c = upi[x], (upi[x - ch] if x >= ch else 0)
                if t == 1:
                    pred = a
                elif t == 3:
                    pred = (a + b) // 2
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[x] = (cur[x] + pred) & 255
            out[y] = cur.astype(np.uint8)
    return out.reshape(H, W, ch)


def unfilter(filtered, B, W, H, channels):
    """dgm_png_unfilter: `filtered` a uint8 device tensor of B * H * (1 + W * channels) bytes -> (B, H, W, channels) uint8;
    channels 1, 3 or 4 (the packed rows of a sub-byte image: W = the row's bytes, channels = 1)."""
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


def expand(packed, W, depth, scale):
    """dgm_png_expand: packed (B, H, ceil(W * depth / 8)) uint8 on the device -> (B, H, W, 1) uint8, sample * scale."""
    import torch

    from . import _lib
    if not (torch.is_tensor(packed) and packed.is_cuda and packed.dtype == torch.uint8 and packed.dim() == 3 and packed.is_contiguous()):
        raise RuntimeError("expand needs a contiguous (B, H, row bytes) uint8 CUDA/HIP tensor (dg-mesh_amd has no CPU path for its kernels)")
    B, H, rb = packed.shape
    if depth not in (1, 2, 4, 8) or rb != (W * depth + 7) // 8:
        raise ValueError(f"expand: rows of {rb} bytes for W={W} depth={depth}")
    out = torch.empty((B, H, W, 1), dtype=torch.uint8, device=packed.device)
    with _lib.device_guard(packed.device):
        _lib.check(_lib.lib().dgm_png_expand(B, W, H, depth, scale, ctypes.c_void_p(packed.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                             _lib.stream_ptr()))
    return out


GREY_SCALE = {1: 255, 2: 85, 4: 17, 8: 1}  # Pillow's expansion of grey samples to 8 bits


def mask_kind(colour, depth):
    """What a mask file's bytes mean after decoding: "index" (palette indices, and 1-bit grey, which Pillow opens as mode 1: both
    resize with NEAREST), "grey" (mode L), "rgb", "rgba"."""
    if colour == 3 or (colour == 0 and depth == 1):
        return "index"
    return {0: "grey", 2: "rgb", 6: "rgba"}[colour]


def _staged_groups(paths, device, parse, key_of, stride_of, who):
    """parse the files on a thread pool, group them by key_of(parsed), stage each group in one page-locked buffer and upload it
    once: yields (key, indices, device bytes of the group)."""
    import torch
    paths = list(paths)
    if not paths:
        raise ValueError(f"{who}: no files")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{who} needs a CUDA/HIP device (dg-mesh_amd has no CPU path for its kernels)")
    groups = {}
    with ThreadPoolExecutor(max_workers=min(MAX_WORKERS, len(paths))) as pool:
        parsed = list(pool.map(parse, paths))
        for i, rec in enumerate(parsed):
            groups.setdefault(key_of(rec), []).append(i)
        for key, idx in groups.items():
            # each file's scanlines are copied into their slot of the staging buffer once, by the pool
            n = stride_of(key)
            host = torch.empty(len(idx) * n, dtype=torch.uint8, pin_memory=True)
            slots = host.numpy().reshape(len(idx), n)

            def fill(k, i):
                slots[k] = np.frombuffer(parsed[i][-1], np.uint8)
                parsed[i] = None
            list(pool.map(fill, range(len(idx)), idx))
            yield key, idx, host.to(device)


def decode_mask_groups(paths, device):
    """decode_png_groups for mask files: a list of (indices, (n, H, W, C) uint8 batch, kind), one entry per (size, colour type,
    bit depth).  kind as mask_kind; C is 1 for "index" and "grey", 3 and 4 for "rgb" and "rgba".  Grey samples are scaled to 8 bits
    as Pillow scales them; palette indices are the indices."""
    out = []
    for (W, H, colour, depth, rb, bpp), idx, dev_bytes in _staged_groups(paths, device, parse_png_any, lambda r: r[:6],
                                                                         lambda k: k[1] * (1 + k[4]), "decode_masks"):
        if colour in (2, 6):
            batch = unfilter(dev_bytes, len(idx), W, H, bpp)
        else:
            packed = unfilter(dev_bytes, len(idx), rb, H, 1).reshape(len(idx), H, rb)
            batch = expand(packed, W, depth, GREY_SCALE[depth] if colour == 0 else 1)
        out.append((idx, batch, mask_kind(colour, depth)))
    return out


def decode_png_groups(paths, device):
    """The files' pixels, grouped by (W, H, channels): a list of (indices, batch), `indices` the positions in `paths` of the
    files of one shape, in order, and `batch` their (len(indices), H, W, C) uint8 device tensor.  The files are inflated on a pool
    of at most MAX_WORKERS threads (zlib releases the GIL); each group has one page-locked staging buffer, one upload and one
    dgm_png_unfilter call."""
    return [(idx, unfilter(dev_bytes, len(idx), W, H, ch))
            for (W, H, ch), idx, dev_bytes in _staged_groups(paths, device, parse_png, lambda r: r[:3], lambda k: k[1] * (1 + k[0] * k[2]),
                                                             "decode_pngs")]


def decode_pngs(paths, device):
    """(B, H, W, C) uint8 device tensor of files of ONE shape, in the order of `paths` (decode_png_groups takes mixed shapes)."""
    groups = decode_png_groups(paths, device)
    if len(groups) != 1:
        shapes = sorted(tuple(b.shape[1:]) for _, b in groups)
        raise ValueError(f"decode_pngs: the files have {len(groups)} shapes {shapes}; decode_png_groups returns one batch per shape")
    return groups[0][1]
