"""Image resampling (resample.py, csrc/resample.hip): the numpy restatement of Pillow's 8-bit Image.resize (tests/_resample_ref.py)
against Pillow's own outputs (tests/golden/resample_small.npz), the host's coefficient tables and size formulas against the
restatement, and the kernels against the restatement, all bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _resample_ref as R
from conftest import ROOT, pkg

SHAPES = [((2, 2), (1, 1)), ((9, 7), (4, 3)), ((20, 20), (2, 2)), ((64, 48), (8, 6)), ((67, 70), (33, 35)), ((16, 16), (16, 8)),
          ((16, 16), (8, 16)), ((13, 11), (20, 17)), ((300, 40), (150, 20)), ((5, 5), (5, 5))]
CONTENTS = ("noise", "smooth", "sparse_alpha")
FILTERS = ("lanczos", "bicubic")
MODES = ("rgba", "rgb", "l")
SHAPE_IDS = [f"{W}x{H}-{ow}x{oh}" for (W, H), (ow, oh) in SHAPES]


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "resample_small.npz"))
    return {k: z[k] for k in z.files}


def source(px, mode):
    return {"rgba": px, "rgb": np.ascontiguousarray(px[..., :3]), "l": np.ascontiguousarray(px[..., 3])}[mode]


def key(shape, kind):
    (W, H), (ow, oh) = shape
    return f"{W}x{H}_{ow}x{oh}/{kind}"


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_restatement_equals_pillow(golden, shape):
    assert str(golden["pillow_version"]), "the golden file records the Pillow version it was made with"
    for kind in CONTENTS:
        px = golden[key(shape, kind) + "/in"]
        assert px.shape == (shape[0][1], shape[0][0], 4)
        for f in FILTERS:
            for mode in MODES:
                want = golden[f"{key(shape, kind)}/{f}/{mode}"]
                got = R.resize(source(px, mode), shape[1], f)
                assert got.shape == want.shape and np.array_equal(got, want), (kind, f, mode)


def test_golden_reaches_the_branches(golden):
    """The sparse-alpha content reaches both copy branches of the un-premultiply, its clamp at 255 and negative accumulators (here
    in the upscale, whose first pass is the horizontal one)."""
    shape = SHAPES[7]
    px = golden[key(shape, "sparse_alpha") + "/in"]
    pre = R.resize_plain(R.premultiply(px), shape[1], "lanczos")
    a = pre[..., 3].astype(np.int64)
    mid = (a > 0) & (a < 255)
    assert (a == 0).any() and (a == 255).any() and mid.any()
    assert ((255 * pre[..., :3].astype(np.int64))[mid] // a[mid][:, None] > 255).any(), "no clamp at 255"
    taps, bounds = R.coefficients(shape[0][0], shape[1][0], "lanczos")
    cols = np.moveaxis(R.premultiply(px).astype(np.int64), 1, 0)
    acc = [((taps[i, :n, None, None] * cols[lo:lo + n]).sum(0) + (1 << 21)).min() for i, (lo, n) in enumerate(bounds)]
    assert (taps < 0).any() and min(acc) < 0, "no negative accumulator"


@pytest.mark.parametrize("f", FILTERS)
def test_coefficients_equal_the_restatement(f):
    P = pkg("resample")
    sizes = {(a, b) for (W, H), (ow, oh) in SHAPES for a, b in ((W, ow), (H, oh))} | {(801, 400), (800, 400), (1, 7), (7, 1), (37, 36)}
    for a, b in sorted(sizes):
        taps, bounds = P.coefficients(a, b, f)
        want_t, want_b = R.coefficients(a, b, f)
        assert taps.dtype == np.int32 and bounds.dtype == np.int32 and taps.shape == want_t.shape and bounds.shape == (b, 2)
        assert np.array_equal(taps, want_t) and np.array_equal(bounds, want_b), (a, b)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= a).all() and (bounds[:, 1] <= taps.shape[1]).all()
    assert P.coefficients(20, 2, "lanczos")[0].shape[1] == 61 and P.coefficients(64, 8, "lanczos")[0].shape[1] == 49
    with pytest.raises(ValueError):
        P.coefficients(4, 2, "nearest")
    with pytest.raises(ValueError):
        P.coefficients(4, 0, f)


def test_size_formulas():
    P = pkg("resample")
    assert P.target_size_downsample(800, 800, 2.0) == (400, 400) and P.target_size_downsample(801, 33, 2.0) == (400, 16)
    assert P.target_size_downsample(40, 24, 1.5) == (26, 16) and P.target_size_downsample(40, 24, 1.0) == (40, 24)
    # round half to even, as Python's round
    assert P.target_size_resolution(100, 20, 8) == (12, 2) and P.target_size_resolution(28, 28, 8) == (4, 4)
    assert P.target_size_resolution(800, 800, 2) == (400, 400) and P.target_size_resolution(801, 33, 2) == (400, 16)
    assert P.target_size_resolution(40, 24, 1) == (40, 24) and P.target_size_resolution(50, 30, 4) == (12, 8)
    assert P.target_size_resolution(1600, 900, -1) == (1600, 900) and P.target_size_resolution(800, 600, -1) == (800, 600)
    w, h = 1700, 900
    assert P.target_size_resolution(w, h, -1) == (int(w / (w / 1600)), int(h / (w / 1600))) == (1600, 847)
    assert P.target_size_resolution(800, 600, 400) == (int(800 / (800 / 400)), int(600 / (800 / 400))) == (400, 300)
    assert P.target_size_resolution(48, 48, 5) == (int(48 / (48 / 5)), int(48 / (48 / 5)))
    with pytest.raises(ValueError):
        P.target_size_resolution(48, 48, 0)


def test_host_tensors_are_refused():
    P, D = pkg("resample"), pkg("dataset")
    with pytest.raises(RuntimeError):
        P.resize(torch.zeros((1, 4, 4, 4), dtype=torch.uint8), (2, 2), "lanczos")
    with pytest.raises(RuntimeError):
        P.resize(torch.zeros((1, 4, 4, 4), dtype=torch.uint8), (4, 4), "lanczos")
    with pytest.raises(RuntimeError):
        D.image_composite_bytes(torch.zeros((1, 2, 2, 4), dtype=torch.uint8), [0, 0, 0])


def test_c_abi_argument_errors_without_gpu():
    """Validation comes before any HIP call.  The pointers are never dereferenced: every call below is refused."""
    L = pkg("_lib")
    lib = L.lib()
    vp = ctypes.c_void_p
    p = vp(4096)  # (non-null, 16-byte aligned)
    bg = (ctypes.c_float * 3)(0, 0, 0)

    def resample(B=1, H=8, W=8, C=4, src=p, oh=4, ow=4, kx=p, bx=p, ksx=7, ky=p, by=p, ksy=7, flags=0, tmp=p, out=p, image=None, mask=None):
        return lib.dgm_resample(B, H, W, C, src, oh, ow, kx, bx, ksx, ky, by, ksy, flags, tmp, out, image, mask, None)

    cases = [dict(B=0), dict(B=65536), dict(H=0), dict(W=(1 << 20) + 1), dict(oh=0), dict(ow=-1), dict(C=2), dict(C=5), dict(src=None),
             dict(flags=4), dict(flags=1, C=3), dict(flags=2, C=1), dict(kx=None, ky=None), dict(kx=None), dict(ky=None),
             dict(bx=None), dict(by=None), dict(ksx=0), dict(ksy=0), dict(kx=vp(4100)), dict(bx=vp(4104)), dict(ky=vp(4097)),
             dict(tmp=None), dict(out=None), dict(flags=2), dict(flags=2, image=p), dict(flags=2, image=p, mask=vp(4098)),
             dict(src=vp(4098)), dict(tmp=vp(4097)), dict(out=vp(4099))]
    for kw in cases:
        assert resample(**kw) == 1, kw
        assert b"resample: bad argument" in lib.dgm_last_error(), kw
    for kw in (dict(B=0), dict(B=65536), dict(W=0), dict(H=(1 << 24) + 1), dict(C=1), dict(src=None), dict(bg3=None), dict(out=None),
               dict(src=vp(4097)), dict(out=vp(4098))):
        a = dict(B=1, H=4, W=4, C=4, src=p, bg3=bg, out=p)
        a.update(kw)
        assert lib.dgm_image_composite_bytes(a["B"], a["H"], a["W"], a["C"], a["src"], a["bg3"], a["out"], None) == 1, kw
        assert b"image_composite_bytes: bad argument" in lib.dgm_last_error(), kw
    assert {"dgm_resample", "dgm_image_composite_bytes"} <= set(L.SYMBOLS) and L.ABI_VERSION == 5


# ---- on the device ------------------------------------------------------------------------------------------------------------------

def planes_of(img):
    """(H, W, 3 or 4) uint8 -> what out="planes" holds: image (3, H, W) = byte / 255 in fp32, mask (H, W, 1) = alpha / 255."""
    image = np.ascontiguousarray((img[..., :3].astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1))
    mask = (img[..., 3:4] / 255.0).astype(np.float32) if img.shape[2] == 4 else np.ones(img.shape[:2] + (1,), np.float32)
    return image, mask


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_resize_equals_the_restatement(golden, shape):
    """Every content as one batch of three distinct images, under both filters, as RGBA (premultiplied and not), RGB and a single
    plane, in both output forms."""
    P = pkg("resample")
    size = shape[1]
    batch = np.stack([golden[key(shape, kind) + "/in"] for kind in CONTENTS])
    assert not np.array_equal(batch[0], batch[1]) and not np.array_equal(batch[1], batch[2])
    dev = torch.device("cuda:0")
    same = size == shape[0]
    for mode, premultiplied in (("rgba", None), ("rgba", False), ("rgb", None), ("l", None)):
        src = np.stack([source(b, mode) for b in batch])
        t = torch.tensor(src if src.ndim == 4 else src[..., None], device=dev)
        for f in FILTERS:
            want = [R.resize(s, size, f, premultiplied) for s in src]
            got = P.resize(t, size, f, premultiplied=premultiplied)
            assert (got is t) == same, "an unchanged size returns the input itself, and only then"
            got = got.cpu().numpy()
            assert got.shape == (3, size[1], size[0], t.shape[3]) and got.dtype == np.uint8
            for b in range(3):
                w = want[b] if want[b].ndim == 3 else want[b][..., None]
                bad = np.argwhere(got[b] != w)
                assert bad.size == 0, f"{mode} premultiplied={premultiplied} {f} image {b}: {len(bad)} bytes differ, first {bad[0].tolist()}"
                if mode != "l":
                    if premultiplied is None:
                        assert np.array_equal(w, golden[f"{key(shape, CONTENTS[b])}/{f}/{mode}"]), "the restatement left the golden"
                    image, mask = P.resize(t[b:b + 1], size, f, premultiplied=premultiplied, out="planes")
                    wi, wm = planes_of(w)
                    assert image.shape == (1, 3, size[1], size[0]) and mask.shape == (1, size[1], size[0], 1)
                    assert np.array_equal(image[0].cpu().numpy(), wi) and np.array_equal(mask[0].cpu().numpy(), wm), (mode, f, b)
    with pytest.raises(ValueError):
        P.resize(torch.zeros((1, 4, 4, 1), dtype=torch.uint8, device=dev), (2, 2), "bicubic", out="planes")
    with pytest.raises(ValueError):
        P.resize(torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=dev), (2, 2), "bicubic", premultiplied=True)


@pytest.mark.gpu
@pytest.mark.parametrize("f", FILTERS)
def test_resize_rgb_slice_at_an_odd_address(f):
    """A contiguous slice of an RGB batch may start at any byte (here 3 * 7 * 9 = 189 past the allocation)."""
    P = pkg("resample")
    px = np.random.RandomState(11).randint(0, 256, (3, 7, 9, 3)).astype(np.uint8)
    t = torch.tensor(px, device="cuda:0")[1:]
    assert t.is_contiguous() and t.data_ptr() % 4 != 0
    got = P.resize(t, (4, 3), f).cpu().numpy()
    image, _ = P.resize(t, (13, 7), f, out="planes")  # (horizontal pass only, upscale)
    for b in range(2):
        assert np.array_equal(got[b], R.resize(px[b + 1], (4, 3), f))
        assert np.array_equal(image[b].cpu().numpy(), planes_of(R.resize(px[b + 1], (13, 7), f))[0])


@pytest.mark.gpu
@pytest.mark.parametrize("white", [False, True])
def test_composite_bytes_are_the_ingest_bytes(white):
    """All 256 x 256 (colour, alpha) pairs and an odd-sized RGB image: the byte variant holds image_ingest's bytes before the
    division, with the file's alpha beside them."""
    import _ingest_ref
    from test_ingest_kernels import table_image
    D = pkg("dataset")
    bg = [1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0]
    for px in (np.stack([table_image(1), table_image(2)]), np.random.RandomState(3).randint(0, 256, (2, 7, 5, 3)).astype(np.uint8)):
        got = D.image_composite_bytes(torch.tensor(px, device="cuda:0"), bg).cpu().numpy()
        assert got.shape == px.shape[:3] + (4,)
        for b in range(2):
            want_i, want_m = _ingest_ref.ingest(px[b], white)
            assert np.array_equal(got[b, ..., :3].astype(np.float32) / np.float32(255.0), want_i.transpose(1, 2, 0))
            assert np.array_equal(got[b, ..., 3], px[b, ..., 3] if px.shape[3] == 4 else np.full(px.shape[1:3], 255, np.uint8))
