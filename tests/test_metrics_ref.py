"""CPU checks of the image-metric definitions: the float64 restatement tests/_metrics_ref.py against the reference's rgb_ssim /
get_psnr values recorded in tests/golden/metrics_small.npz, the MS-SSIM pooling rule, and vertex colours in mesh PLYs."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg

sys.path.insert(0, os.path.join(ROOT, "tests"))
import _metrics_ref as MR  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "metrics_small.npz"))
SHAPES = [tuple(int(v) for v in s) for s in GOLD["shapes"]]
KINDS = [str(k) for k in GOLD["kinds"]]


def pair8(kind, H, W):
    """The uint8 pair of the golden: `self` and `inverse` derive from the smooth image."""
    if kind in ("smooth", "flat"):
        return GOLD[f"{kind}_{H}x{W}/x"], GOLD[f"{kind}_{H}x{W}/y"]
    x = GOLD[f"smooth_{H}x{W}/x"]
    return (x, x) if kind == "self" else (x, (255 - x).astype(np.uint8))


def pair64(kind, H, W):
    x, y = pair8(kind, H, W)
    return x.astype(np.float64) / 255, y.astype(np.float64) / 255


def test_golden_covers_the_cases():
    assert SHAPES == [(12, 43), (33, 70), (161, 163), (176, 162)] and KINDS == ["smooth", "flat", "self", "inverse"]
    for H, W in SHAPES:
        assert bool(GOLD[f"flat_{H}x{W}/clip"]) and not bool(GOLD[f"smooth_{H}x{W}/clip"])
        assert GOLD[f"smooth_{H}x{W}/x"].dtype == np.uint8 and GOLD[f"smooth_{H}x{W}/x"].shape == (3, H, W)


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_psnr_and_ssim_equal_the_reference_in_fp64(kind, H, W):
    x, y = pair64(kind, H, W)
    key = f"{kind}_{H}x{W}"
    assert abs(MR.ssim(x, y) - float(GOLD[key + "/ssim64"])) <= 1e-12
    ref = float(GOLD[key + "/psnr64"])
    if np.isinf(ref):
        assert MR.psnr(x, y) == ref
    else:
        assert abs(MR.psnr(x, y) - ref) <= 1e-12 * max(1.0, abs(ref))
    assert float(GOLD[key + "/ssim_fp32_err"]) == abs(float(GOLD[key + "/ssim32"]) - float(GOLD[key + "/ssim64"]))


@pytest.mark.parametrize("H,W", [s for s in SHAPES if min(s) > 160])
def test_ms_ssim_restatement(H, W):
    x, y = pair64("smooth", H, W)
    assert MR.ms_ssim(x, x) == 1.0
    for kind in KINDS:
        a, b = pair64(kind, H, W)
        assert MR.ms_ssim(a, b) == float(GOLD[f"{kind}_{H}x{W}/msssim64"])
    assert MR.ms_ssim(*pair64("inverse", H, W)) == 0.0  # every cs is negative: the relu engages
    m32 = MR.ms_ssim(x.astype(np.float32), y.astype(np.float32))
    assert m32.dtype == np.float32
    assert abs(np.float64(m32) - MR.ms_ssim(x, y)) == float(GOLD[f"smooth_{H}x{W}/msssim_fp32_err"])


def test_ms_ssim_refuses_small_images():
    x = np.zeros((3, 160, 200))
    with pytest.raises(ValueError):
        MR.ms_ssim(x, x)


def test_pooled_sizes():
    assert MR.pooled_sizes(161) == [161, 81, 41, 21, 11]
    assert MR.pooled_sizes(176) == [176, 88, 44, 22, 11]
    z = np.arange(3 * 5 * 4, dtype=np.float64).reshape(3, 5, 4)
    p = MR.pool(z)
    assert p.shape == (3, 3, 2)
    # odd height: padded on both ends, divisor 4 -- the first output row sees the pad and one input row; the windows then tile the
    # rows in pairs and the trailing pad row is never reached
    assert np.array_equal(p[:, 0, 0], (z[:, 0, 0] + z[:, 0, 1]) / 4)
    assert np.array_equal(p[:, 1, 1], (z[:, 1, 2] + z[:, 1, 3] + z[:, 2, 2] + z[:, 2, 3]) / 4)
    assert np.array_equal(p[:, 2, 0], (z[:, 3, 0] + z[:, 3, 1] + z[:, 4, 0] + z[:, 4, 1]) / 4)
    import torch
    for h, w in ((5, 4), (7, 9), (6, 3)):  # torch's avg_pool2d with padding = side % 2 (count_include_pad) is the rule restated
        z = np.random.RandomState(h).rand(2, h, w)
        want = torch.nn.functional.avg_pool2d(torch.tensor(z)[None], kernel_size=2, padding=(h % 2, w % 2))[0].numpy()
        assert np.allclose(MR.pool(z), want, rtol=0, atol=1e-15)
    x = np.random.RandomState(0).rand(1, 161, 176)
    for s_h, s_w in zip(MR.pooled_sizes(161)[1:], MR.pooled_sizes(176)[1:]):
        x = MR.pool(x)
        assert x.shape == (1, s_h, s_w)


@pytest.mark.parametrize("H,W", SHAPES)
def test_level0_ssim_l_is_rgb_ssim_where_nothing_clips(H, W):
    for kind in ("smooth", "self"):
        x, y = pair64(kind, H, W)
        val, clipped = MR.ssim(x, y, return_clipped=True)
        assert not clipped
        _, sl = MR.level_terms(x, y)
        assert abs(sl.mean() - val) <= 1e-14


def _plain_mesh_bytes(verts, faces):
    """The file write_mesh_ply wrote before it knew colours."""
    v = np.ascontiguousarray(verts, dtype="<f4").reshape(-1, 3)
    rec = np.empty(len(faces), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    rec["n"], rec["idx"] = 3, faces
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y",
            "property float z", f"element face {len(faces)}", "property list uchar int vertex_indices", "end_header"]
    return ("\n".join(head) + "\n").encode("ascii") + v.tobytes() + rec.tobytes()


def test_mesh_ply_vertex_colours_round_trip(tmp_path):
    io = pkg("ply_io")
    rng = np.random.RandomState(3)
    verts = rng.randn(7, 3).astype(np.float32)
    faces = rng.randint(0, 7, (5, 3)).astype(np.int32)
    colors = rng.uniform(-0.2, 1.2, (7, 3)).astype(np.float32)
    colors[0] = (0.0, 1.0, 0.5)
    path = str(tmp_path / "c.ply")
    io.write_mesh_ply(path, verts, faces, vertex_colors=colors)
    v, f, c = io.read_mesh_ply(path, return_colors=True)
    assert np.array_equal(v, verts) and np.array_equal(f, faces)
    want = np.clip(colors * 255, 0, 255).astype(np.uint8)
    assert c.dtype == np.uint8 and np.array_equal(c[:, :3], want) and (c[:, 3] == 255).all()
    assert tuple(c[0]) == (0, 255, 127, 255)
    assert len(io.read_mesh_ply(path)) == 2 and np.array_equal(io.read_mesh_ply(path)[0], verts)
    head = open(path, "rb").read().split(b"end_header")[0].decode()
    assert "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face" in head
    with pytest.raises(ValueError):
        io.write_mesh_ply(path, verts, faces, vertex_colors=colors[:3])


def test_mesh_ply_without_colours_is_unchanged(tmp_path):
    io = pkg("ply_io")
    rng = np.random.RandomState(4)
    verts = rng.randn(6, 3).astype(np.float32)
    faces = rng.randint(0, 6, (4, 3)).astype(np.int32)
    path = str(tmp_path / "p.ply")
    io.write_mesh_ply(path, verts, faces)
    assert open(path, "rb").read() == _plain_mesh_bytes(verts, faces)
    v, f, c = io.read_mesh_ply(path, return_colors=True)
    assert c is None and np.array_equal(v, verts) and np.array_equal(f, faces)
