"""The two ingest kernels (csrc/ingest.hip) bit for bit against the test-side restatements: dgm_png_unfilter against tests/_png_ref.py,
dgm_image_ingest against tests/_ingest_ref.py."""
import os

import numpy as np
import pytest
import torch

import _ingest_ref
import _png_ref
from conftest import ROOT, pkg

# (W, H, channels): the smallest; no row above; no pixel to the left; more rows than a wave's 64 lanes; a skew longer than the image
# is tall; more rows than any 1024-row band
SHAPES = [(1, 1, 4), (1, 1, 3), (17, 1, 4), (17, 1, 3), (1, 9, 4), (1, 9, 3), (67, 70, 4), (300, 5, 4), (300, 5, 3), (3, 1100, 3)]


def contents(rng, H, W, ch):
    return {"noise": rng.randint(0, 256, (H, W, ch)).astype(np.uint8),
            "constant": np.full((H, W, ch), 77, np.uint8),
            "low_entropy": rng.choice(np.array([0, 1, 2, 255], np.uint8), (H, W, ch))}  # (Paeth ties)


def filter_choices(rng, H):
    return [[t] * H for t in range(5)] + [list(rng.randint(0, 5, H))]


def run_unfilter(filtered_list, W, H, ch):
    P = pkg("png_io")
    dev = torch.device("cuda:0")
    host = torch.frombuffer(bytearray(b"".join(filtered_list)), dtype=torch.uint8)
    out = P.unfilter(host.to(dev), len(filtered_list), W, H, ch)
    torch.cuda.synchronize()
    assert out.shape == (len(filtered_list), H, W, ch) and out.dtype == torch.uint8
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,ch", SHAPES)
def test_unfilter_bit_exact(W, H, ch):
    """Every content under every filter choice, all in one batched call (18 images)."""
    rng = np.random.RandomState(W * 7 + H * 3 + ch)
    pixels, filtered = [], []
    for px in contents(rng, H, W, ch).values():
        for types in filter_choices(rng, H):
            pixels.append(px)
            filtered.append(_png_ref.filter_rows(px, types))
    want = np.stack([_png_ref.unfilter(f, W, H, ch) for f in filtered])
    assert np.array_equal(want, np.stack(pixels)), "the restatement does not invert its own encoder"
    got = run_unfilter(filtered, W, H, ch)
    bad = np.argwhere((got != want).reshape(len(filtered), -1).any(axis=1)).ravel()
    assert bad.size == 0, f"images {bad.tolist()} differ (6 filter choices per content: noise, constant, low entropy)"


@pytest.mark.gpu
def test_unfilter_three_distinct_images_in_one_call():
    rng = np.random.RandomState(5)
    W, H, ch = 21, 13, 4
    pixels = [rng.randint(0, 256, (H, W, ch)).astype(np.uint8) for _ in range(3)]
    filtered = [_png_ref.filter_rows(px, rng.randint(0, 5, H)) for px in pixels]
    got = run_unfilter(filtered, W, H, ch)
    for k in range(3):
        assert np.array_equal(got[k], _png_ref.unfilter(filtered[k], W, H, ch)), k
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])


@pytest.mark.gpu
def test_decode_pngs_on_the_golden_files(tmp_path):
    P = pkg("png_io")
    z = np.load(os.path.join(ROOT, "tests", "golden", "png_small.npz"))
    names = sorted(k[:-4] for k in z.files if k.endswith("/png"))
    paths = []
    for n in names + names[:2]:  # (two shapes twice: groups of two images)
        paths.append(str(tmp_path / f"{len(paths)}.png"))
        with open(paths[-1], "wb") as fh:
            fh.write(z[n + "/png"].tobytes())
    groups = P.decode_png_groups(paths, "cuda:0")
    order = names + names[:2]
    assert sorted(i for idx, _ in groups for i in idx) == list(range(len(paths))) and len(groups) == len(names)
    for idx, batch in groups:
        assert batch.dtype == torch.uint8 and batch.shape[0] == len(idx) and idx == sorted(idx)
        for k, i in enumerate(idx):
            assert np.array_equal(batch[k].cpu().numpy(), z[order[i] + "/pixels"]), order[i]
    assert sorted(len(idx) for idx, _ in groups) == [1] * (len(names) - 2) + [2, 2]
    same = P.decode_pngs([paths[0], paths[len(names)]], "cuda:0")  # one shape: the batch tensor itself
    assert torch.is_tensor(same) and same.shape[0] == 2 and np.array_equal(same[1].cpu().numpy(), z[names[0] + "/pixels"])
    with pytest.raises(ValueError, match="2 shapes"):
        P.decode_pngs(paths[:2], "cuda:0")


def run_ingest(pixels, white):
    D = pkg("dataset")
    t = torch.tensor(np.ascontiguousarray(pixels), device="cuda:0")
    image, mask = D.image_ingest(t, [1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0])
    torch.cuda.synchronize()
    B, H, W, _ = pixels.shape
    assert image.shape == (B, 3, H, W) and mask.shape == (B, H, W, 1) and image.dtype == mask.dtype == torch.float32
    return image.cpu().numpy(), mask.cpu().numpy()


def table_image(perm_seed):
    """All 256 x 256 (colour, alpha) pairs: row = alpha, column = colour in R, two permutations of it in G and B."""
    rng = np.random.RandomState(perm_seed)
    c = np.arange(256, dtype=np.uint8)
    img = np.empty((256, 256, 4), np.uint8)
    img[..., 0] = c[None, :]
    img[..., 1] = rng.permutation(c)[None, :]
    img[..., 2] = rng.permutation(c)[None, :]
    img[..., 3] = c[:, None]
    return img


@pytest.mark.gpu
@pytest.mark.parametrize("white", [False, True])
def test_ingest_exhaustive_table(white):
    """Every (colour, alpha) pair in every channel, as a batch of two tables with different permutations.  The float64 expression
    truncates to another byte than the exact integer quotient for ~150 pairs: the table would show an integer shortcut."""
    px = np.stack([table_image(1), table_image(2)])
    image, mask = run_ingest(px, white)
    for b in range(2):
        want_i, want_m = _ingest_ref.ingest(px[b], white)
        diff = np.argwhere(image[b] != want_i)
        assert diff.size == 0, f"batch {b}: {len(diff)} values differ, first (channel, alpha, column) = {diff[0].tolist()}"
        assert np.array_equal(mask[b], want_m)
    # the quirk the kernel has to reproduce is present in this table
    c, a, bg = px[0][..., 0].astype(np.int64), px[0][..., 3].astype(np.int64), 255 * int(white)
    exact = (c * a + bg * (255 - a)) // 255
    assert np.count_nonzero(np.rint(image[0][0] * 255).astype(np.int64) != exact) > 100


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,ch", [(5, 7, 3), (33, 19, 4)])
@pytest.mark.parametrize("white", [False, True])
def test_ingest_odd_sizes(W, H, ch, white):
    """Pixel counts that are no multiple of four: the vector path's tail; RGB reads alpha as 255."""
    rng = np.random.RandomState(W + H)
    px = rng.randint(0, 256, (2, H, W, ch)).astype(np.uint8)
    image, mask = run_ingest(px, white)
    for b in range(2):
        want_i, want_m = _ingest_ref.ingest(px[b], white)
        assert np.array_equal(image[b], want_i) and np.array_equal(mask[b], want_m)
    if ch == 3:
        assert float(mask.min()) == 1.0


@pytest.mark.gpu
def test_ingest_rgb_slice_at_an_odd_address():
    """A contiguous slice of an RGB batch starts at any byte (here 105 past the allocation): the three-channel path takes it."""
    D = pkg("dataset")
    px = np.random.RandomState(9).randint(0, 256, (3, 7, 5, 3)).astype(np.uint8)
    t = torch.tensor(px, device="cuda:0")[1:]
    assert t.is_contiguous() and t.data_ptr() % 4 != 0
    image, mask = D.image_ingest(t, [1.0, 1.0, 1.0])
    torch.cuda.synchronize()
    for b in range(2):
        want_i, want_m = _ingest_ref.ingest(px[b + 1], True)
        assert np.array_equal(image[b].cpu().numpy(), want_i) and np.array_equal(mask[b].cpu().numpy(), want_m)


def test_kernels_refuse_host_tensors():
    P, D = pkg("png_io"), pkg("dataset")
    with pytest.raises(RuntimeError):
        P.unfilter(torch.zeros(5, dtype=torch.uint8), 1, 1, 1, 4)
    with pytest.raises(RuntimeError):
        D.image_ingest(torch.zeros((1, 2, 2, 4), dtype=torch.uint8), [0, 0, 0])
