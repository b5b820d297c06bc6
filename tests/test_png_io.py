"""The PNG reader's host half (png_io.parse_png) and the test-side restatement it is checked against (tests/_png_ref.py), on the
golden files PIL encoded (tests/golden/png_small.npz).  Nothing here touches a device: malformed files never leave the host."""
import os
import struct
import zlib

import numpy as np
import pytest

import _png_ref
from conftest import ROOT, pkg

GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "png_small.npz"))
NAMES = sorted(k[:-4] for k in GOLDEN.files if k.endswith("/png"))


def golden(name):
    return GOLDEN[name + "/png"].tobytes(), GOLDEN[name + "/pixels"]


def test_the_golden_set_is_what_the_issue_asks_for():
    assert len(NAMES) >= 5
    chans = set()
    for n in NAMES:
        px = golden(n)[1]
        assert px.shape[0] <= 67 and px.shape[1] <= 70
        chans.add(px.shape[2])
    assert chans == {3, 4}


@pytest.mark.parametrize("name", NAMES)
def test_ref_decodes_the_golden_png(name):
    data, pixels = golden(name)
    assert np.array_equal(_png_ref.decode_png(data), pixels)


def test_ref_encoder_round_trips_every_filter_type():
    rng = np.random.RandomState(0)
    for shape in ((5, 7, 4), (1, 6, 3), (9, 1, 4)):
        for content in (rng.randint(0, 256, shape), rng.choice([0, 1, 2, 255], shape)):
            px = content.astype(np.uint8)
            for types in [[t] * shape[0] for t in range(5)] + [rng.randint(0, 5, shape[0])]:
                f = _png_ref.filter_rows(px, types)
                assert list(f[::1 + shape[1] * shape[2]]) == list(types)
                assert np.array_equal(_png_ref.unfilter(f, shape[1], shape[0], shape[2]), px)


@pytest.mark.parametrize("name", NAMES)
def test_parse_png_header_and_bytes(name, tmp_path):
    P = pkg("png_io")
    data, pixels = golden(name)
    W, H, ch, filtered = P.parse_png(data)
    assert (H, W, ch) == pixels.shape
    assert (W, H, ch, filtered) == _png_ref.read_png(data)
    path = tmp_path / (name + ".png")
    path.write_bytes(data)
    assert P.parse_png(str(path)) == (W, H, ch, filtered) == P.parse_png(path)


def test_parse_png_joins_idat_chunks():
    P = pkg("png_io")
    px = np.random.RandomState(1).randint(0, 256, (6, 5, 4)).astype(np.uint8)
    one, three = _png_ref.encode_png(px, [4] * 6, 1), _png_ref.encode_png(px, [4] * 6, 3)
    assert three.count(b"IDAT") == 3 and P.parse_png(one) == P.parse_png(three)


def _rechunk(data, edit):
    """The file with edit(tag, body) -> body applied to every chunk and the CRCs made right again."""
    pos, out = 8, data[:8]
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        out += _png_ref.chunk(tag, edit(tag, data[pos + 8:pos + 8 + n]))
        pos += 12 + n
    return out


def _malformed():
    px = np.random.RandomState(2).randint(0, 256, (6, 5, 4)).astype(np.uint8)
    filt = _png_ref.filter_rows(px, [0, 1, 2, 3, 4, 1])
    good = _png_ref.wrap_png(filt, 5, 6, 4)
    cases = {"interlace": (_png_ref.wrap_png(filt, 5, 6, 4, interlace=1), "interlace"),
             "depth16": (_png_ref.wrap_png(filt, 5, 6, 4, depth=16), "bit depth 16"),
             "depth4": (_png_ref.wrap_png(filt, 5, 6, 4, depth=4), "bit depth 4")}
    for colour in (0, 3, 4):
        cases[f"colour{colour}"] = (_png_ref.wrap_png(filt, 5, 6, 4, colour=colour), f"colour type {colour}")
    cases["cut_mid_chunk"] = (good[:len(good) - 20], "truncated")
    cases["cut_before_iend"] = (good[:len(good) - 12], "truncated")
    cases["cut_in_header"] = (good[:20], "truncated")
    short = zlib.compress(filt, 6)[:-9]
    cases["cut_zlib_stream"] = (_rechunk(good, lambda tag, body: short if tag == b"IDAT" else body), "truncated")
    cases["short_image"] = (_png_ref.wrap_png(filt[:-21], 5, 6, 4), "inflates to")
    bad_crc = bytearray(good)
    bad_crc[good.index(b"IDAT") + 6] ^= 0x40
    cases["bad_crc"] = (bytes(bad_crc), "bad CRC")
    bad_filter = bytearray(filt)
    bad_filter[3 * 21] = 5
    cases["bad_filter"] = (_png_ref.wrap_png(bytes(bad_filter), 5, 6, 4), "bad filter type 5 on row 3")
    cases["signature"] = (b"\x89PNX" + good[4:], "signature")
    return good, cases


GOOD, MALFORMED = _malformed()


def test_the_well_formed_twin_parses():
    assert pkg("png_io").parse_png(GOOD)[:3] == (5, 6, 4)


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_parse_png_refuses(case, tmp_path):
    P = pkg("png_io")
    data, reason = MALFORMED[case]
    with pytest.raises(ValueError) as e:
        P.parse_png(data)
    assert reason in str(e.value) and "<bytes>" in str(e.value)
    path = tmp_path / f"{case}.png"
    path.write_bytes(data)
    with pytest.raises(ValueError) as e:
        P.parse_png(str(path))
    assert reason in str(e.value) and f"{case}.png" in str(e.value)


def test_decode_pngs_needs_a_device(tmp_path):
    P = pkg("png_io")
    path = tmp_path / "a.png"
    path.write_bytes(GOOD)
    with pytest.raises(RuntimeError):
        P.decode_pngs([str(path)], "cpu")
    with pytest.raises(ValueError):
        P.decode_pngs([], "cuda")


def test_write_png_output_is_read_back():
    """write_png's files (filter type 0 on every row) pass the reader."""
    import tempfile
    P = pkg("png_io")
    px = np.random.RandomState(3).randint(0, 256, (4, 9, 3)).astype(np.uint8)
    with tempfile.TemporaryDirectory() as d:
        P.write_png(os.path.join(d, "x.png"), px)
        W, H, ch, filtered = P.parse_png(os.path.join(d, "x.png"))
    assert (W, H, ch) == (9, 4, 3) and np.array_equal(_png_ref.unfilter(filtered, W, H, ch), px)
