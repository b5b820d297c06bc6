"""LPIPS without a GPU: the weight loader of lpips.py, the fp64 reference's own checks (tests/_lpips_ref.py) and the C ABI's argument
validation."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _lpips_ref as R
from conftest import ROOT, pkg

SLICES = {"alex": (1, 2, 3, 4, 5), "vgg": (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)}  # the lpips package's slice of each convolution


@pytest.fixture(scope="module", params=["alex", "vgg"])
def weights(request):
    net = request.param
    return net, R.seeded_weights(net, 3)


def layout_b(net, sd):
    """The same tensors as a full lpips.LPIPS state dict."""
    out = {"scaling_layer.shift": torch.zeros(1, 3, 1, 1), "scaling_layer.scale": torch.ones(1, 3, 1, 1)}
    for i, n in enumerate(R.NETS[net][1]):
        for part in ("weight", "bias"):
            out[f"net.slice{SLICES[net][i]}.{n}.{part}"] = sd[f"features.{n}.{part}"]
    for k in range(5):
        out[f"lin{k}.model.1.weight"] = out[f"lins.{k}.model.1.weight"] = sd[f"lin{k}.model.1.weight"]
    return out


def same(p, q):
    return all(len(p[k]) == len(q[k]) and all(np.array_equal(a, b) for a, b in zip(p[k], q[k])) for k in ("conv_w", "conv_b", "lin"))


def test_three_layouts_pack_identically(weights, tmp_path):
    LP = pkg("lpips")
    net, sd = weights
    a = LP.pack(net, dict(sd, **{"classifier.1.weight": torch.zeros(4, 4)}))
    assert same(a, LP.pack(net, layout_b(net, sd)))
    np.savez(tmp_path / "w.npz", **LP.canonical(net, sd))
    assert same(a, LP.pack(net, str(tmp_path / "w.npz")))
    for i, (ci, co, ks) in enumerate(LP.CONVS[net]):
        K = ks * ks * ci
        w = sd[f"features.{R.NETS[net][1][i]}.weight"].numpy()
        assert a["conv_w"][i].shape == ((K + 15) // 16 * 16, co) and a["conv_w"][i].dtype == np.float32
        assert not a["conv_w"][i][K:].any()
        for ky, kx, c in ((0, 0, 0), (ks - 1, 1, ci - 1), (1, ks - 1, ci // 2)):  # row (ky k + kx) C_in + c = weight[:, c, ky, kx]
            assert np.array_equal(a["conv_w"][i][(ky * ks + kx) * ci + c], w[:, c, ky, kx])
    assert [v.shape for v in a["lin"]] == [(LP.CONVS[net][t][1],) for t in LP.TAPS[net]]


def test_loader_names_every_offending_key(weights):
    LP = pkg("lpips")
    net, sd = weights
    first, last = R.NETS[net][1][0], R.NETS[net][1][-1]
    bad = dict(sd)
    del bad[f"features.{last}.bias"], bad["lin2.model.1.weight"]
    bad["features.99.weight"] = torch.zeros(1)
    bad[f"features.{first}.weight"] = sd[f"features.{first}.weight"][:, :, :-1]
    with pytest.raises(ValueError) as e:
        LP.pack(net, bad)
    msg = str(e.value)
    assert f"missing: features.{last}.bias, lin2.model.1.weight" in msg and "unexpected: features.99.weight" in msg
    assert re.search(rf"wrong shape: features\.{first}\.weight \(64, 3, \d+, \d+\) \(expected \(64, 3, \d+, \d+\)\)", msg)
    with pytest.raises(ValueError):
        LP.pack("squeeze", sd)
    with pytest.raises(ValueError) as e:  # the other network's file
        LP.pack("alex" if net == "vgg" else "vgg", sd)
    assert "missing" in str(e.value) or "wrong shape" in str(e.value)


def test_convert_round_trip(tmp_path):
    LP = pkg("lpips")
    sd = R.seeded_weights("alex", 4)
    torch.save({k: v for k, v in sd.items() if k.startswith("features.")}, tmp_path / "backbone.pth")
    torch.save({k: v for k, v in sd.items() if k.startswith("lin")}, tmp_path / "lin.pth")
    p = subprocess.run([sys.executable, "-m", "dgmesh_amd.lpips", "convert", "--net", "alex", "--backbone", str(tmp_path / "backbone.pth"),
                        "--lin", str(tmp_path / "lin.pth"), "--out", str(tmp_path / "alex.npz")], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:]
    assert same(LP.pack("alex", sd), LP.pack("alex", str(tmp_path / "alex.npz")))
    assert same(LP.pack("alex", sd), LP.pack("alex", [str(tmp_path / "backbone.pth"), str(tmp_path / "lin.pth")]))
    with np.load(tmp_path / "alex.npz") as z:
        assert sorted(z.files) == sorted([f"conv{i}.{p}" for i in range(5) for p in ("weight", "bias")] + [f"lin{k}.weight" for k in range(5)])


@pytest.mark.parametrize("net,side", [("alex", 40), ("vgg", 24)])
def test_reference_zero_on_itself_and_symmetric(net, side):
    sd = R.seeded_weights(net, 5, width=0.25)
    imgs, gt = R.make_images(side, side + 3)
    assert not R.lpips_ref(net, sd, gt[None], gt).any()
    ab, ba = R.lpips_ref(net, sd, imgs[3:], gt), R.lpips_ref(net, sd, gt[None], imgs[3])
    assert (ab > 0).all() and torch.equal(ab, ba)


def test_reference_tap_term_by_hand():
    """One 1x1-spatial tap with two channels."""
    a, b, w = (3.0, 4.0), (1.0, 0.0), (0.25, 2.0)
    na, nb = np.sqrt(a[0] ** 2 + a[1] ** 2) + 1e-10, np.sqrt(b[0] ** 2 + b[1] ** 2) + 1e-10
    want = w[0] * (a[0] / na - b[0] / nb) ** 2 + w[1] * (a[1] / na - b[1] / nb) ** 2
    t = lambda v: torch.tensor(v, dtype=torch.float64).reshape(1, 2, 1, 1)
    got = R.tap_term(t(a), t(b), torch.tensor(w, dtype=torch.float64))
    assert got.shape == (1,) and abs(float(got[0]) - want) <= 1e-15
    assert abs(want - (0.25 * 0.16 + 2.0 * 0.64)) < 1e-9  # (0.6 - 1)^2, (0.8 - 0)^2


def test_c_abi_refuses_bad_arguments_without_a_gpu():
    L = pkg("_lib")
    lib = L.lib()
    assert {"dgm_lpips", "dgm_lpips_workspace_bytes"} <= set(L.SYMBOLS) and L.ABI_VERSION == 5 and lib.dgm_abi_version() == 5
    header = open(os.path.join(ROOT, "include", "dgmesh_hip.h")).read()
    assert "size_t dgm_lpips_workspace_bytes(int net, int B, int H, int W);" in header and "int dgm_lpips(int net," in header
    ws = lib.dgm_lpips_workspace_bytes
    assert ws(0, 1, 30, 100) == 0 and ws(0, 1, 100, 30) == 0 and ws(1, 1, 15, 100) == 0 and ws(1, 1, 100, 15) == 0
    assert ws(0, 1, 31, 31) > 0 and ws(1, 1, 16, 16) > 0 and ws(0, 3, 176, 162) > ws(0, 1, 176, 162)
    assert ws(-1, 1, 64, 64) == 0 and ws(2, 1, 64, 64) == 0 and ws(0, 0, 64, 64) == 0 and ws(1, -1, 64, 64) == 0
    ptrs = lambda n, v: (ctypes.c_void_p * n)(*[v] * n)
    one = ctypes.c_void_p(256)  # never dereferenced: every call below is refused before any device work
    good = dict(net=0, w=ptrs(5, 256), b=ptrs(5, 256), lin=ptrs(5, 256), images=one, gt=one, B=1, H=64, W=64, ws=one, out=one)
    for change in (dict(images=None), dict(gt=None), dict(ws=None), dict(out=None), dict(w=None), dict(b=None), dict(lin=None),
                   dict(w=ptrs(5, None)), dict(lin=ptrs(5, None)), dict(net=2), dict(B=0), dict(H=30), dict(net=1, W=15,
                                                                                                           w=ptrs(13, 256), b=ptrs(13, 256))):
        a = dict(good, **change)
        st = lib.dgm_lpips(a["net"], a["w"], a["b"], a["lin"], a["images"], a["gt"], a["B"], a["H"], a["W"], a["ws"], a["out"], None)
        assert st != 0 and b"lpips: " in lib.dgm_last_error(), change


def test_wrapper_has_no_cpu_path():
    LP = pkg("lpips")
    with pytest.raises(RuntimeError):
        LP.LPIPS("alex", {}, device="cpu")
    with pytest.raises(RuntimeError):
        LP._checked(torch.zeros(3, 40, 40), torch.zeros(3, 40, 40), "alex")
