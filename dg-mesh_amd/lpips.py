"""LPIPS 0.1 on the device: the AlexNet and VGG-16 feature stacks of csrc/lpips.hip (dgm_lpips, include/dgmesh_hip.h) behind the two
numbers LPIPS_A and LPIPS_V of the reference's testing() (R/train.py:559-761, R/utils/metric_utils.py:23, R/ = dgmesh/).

The project ships no weights and depends on neither the `lpips` package nor torchvision: a user brings the files they already have.
The loader takes
  (a) a torchvision `alexnet` / `vgg16` state dict (`features.{N}.weight/bias`; classifier keys are ignored) together with the lpips
      package's linear-layer file (`lin{0..4}.model.1.weight`, shape (1, C, 1, 1)) -- as one merged dict, or as a list of paths / dicts;
  (b) a full `lpips.LPIPS(...).state_dict()` (`net.slice{k}.{N}.weight/bias`, `lin{k}.model.1.weight`; `scaling_layer.*` and the
      `lins.*` aliases are ignored);
  (c) one .npz in this project's naming (`conv{i}.weight`, `conv{i}.bias`, `lin{k}.weight`), written by
      `python -m dgmesh_amd.lpips convert --net alex --backbone A.pth --lin B.pth --out alex.npz`.
.pth files are read with torch.load(..., weights_only=True).  A missing key, an extra convolution key or a wrong shape is a
ValueError that names every offending key."""
import argparse
import ctypes
import sys

import numpy as np
import torch

from . import _lib

NETS = ("alex", "vgg")
# (C_in, C_out, kernel) per convolution; TAPS[net][k] = index of the convolution whose ReLU output is tap k
CONVS = {
    "alex": ((3, 64, 11), (64, 192, 5), (192, 384, 3), (384, 256, 3), (256, 256, 3)),
    "vgg": ((3, 64, 3), (64, 64, 3), (64, 128, 3), (128, 128, 3), (128, 256, 3), (256, 256, 3), (256, 256, 3), (256, 512, 3),
            (512, 512, 3), (512, 512, 3), (512, 512, 3), (512, 512, 3), (512, 512, 3)),
}
TAPS = {"alex": (0, 1, 2, 3, 4), "vgg": (1, 3, 6, 9, 12)}
# index of each convolution in torchvision's `features` Sequential
FEATURES = {"alex": (0, 3, 6, 8, 10), "vgg": (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)}
MIN_SIDE = {"alex": 31, "vgg": 16}
K_STEP = 16  # the convolution kernel's K step: packed weights have their rows padded to a multiple of it
COLUMNS = ("tap0", "tap1", "tap2", "tap3", "tap4", "lpips")


def _check_net(net):
    if net not in NETS:
        raise ValueError(f"lpips: net must be one of {NETS}, got {net!r}")


def _numpy(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def _read(weights):
    """A path (.npz, or a .pth read with weights_only=True), a dict, or a list of those merged -> {key: numpy array}."""
    if isinstance(weights, (list, tuple)):
        out = {}
        for w in weights:
            out.update(_read(w))
        return out
    if isinstance(weights, dict):
        return {k: _numpy(v) for k, v in weights.items()}
    path = str(weights)
    if path.endswith(".npz"):
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    return {k: _numpy(v) for k, v in torch.load(path, map_location="cpu", weights_only=True).items()}


def _names(net, layout):
    """{project name: the layout's name} for every tensor of the network."""
    convs = range(len(CONVS[net]))
    if layout == "c":
        src = {i: f"conv{i}" for i in convs}
    elif layout == "a":
        src = {i: f"features.{FEATURES[net][i]}" for i in convs}
    else:  # (b): slice k + 1 holds the convolutions after tap k - 1 up to tap k
        src = {i: f"net.slice{min(k for k in range(5) if TAPS[net][k] >= i) + 1}.{FEATURES[net][i]}" for i in convs}
    names = {}
    for i in convs:
        names[f"conv{i}.weight"] = src[i] + ".weight"
        names[f"conv{i}.bias"] = src[i] + ".bias"
    for k in range(5):
        names[f"lin{k}.weight"] = f"lin{k}.weight" if layout == "c" else f"lin{k}.model.1.weight"
    return names


def canonical(net, weights):
    """The tensors of `weights` (any of the three layouts) under the project's names, float32: conv{i}.weight (C_out, C_in, k, k),
    conv{i}.bias (C_out), lin{k}.weight (C_k).  ValueError naming every missing key, extra convolution key and wrong shape."""
    _check_net(net)
    flat = _read(weights)
    layout = "b" if any(k.startswith("net.slice") for k in flat) else "a" if any(k.startswith("features.") for k in flat) else "c"
    names = _names(net, layout)
    shapes = {}
    for i, (ci, co, ks) in enumerate(CONVS[net]):
        shapes[f"conv{i}.weight"], shapes[f"conv{i}.bias"] = (co, ci, ks, ks), (co,)
    for k in range(5):
        shapes[f"lin{k}.weight"] = (CONVS[net][TAPS[net][k]][1],)
    wanted = set(names.values())
    missing = sorted(v for v in wanted if v not in flat)
    ignored = ("classifier.", "scaling_layer.", "lins.", "avgpool.")
    extra = sorted(k for k in flat if k not in wanted and not k.startswith(ignored))
    out, wrong = {}, []
    for name, key in names.items():
        if key not in flat:
            continue
        a = np.asarray(flat[key])
        want = shapes[name]
        if name.startswith("lin") and a.shape == (1, want[0], 1, 1):
            a = a.reshape(want)
        if a.shape != want:
            wrong.append(f"{key} {tuple(a.shape)} (expected {want})")
            continue
        out[name] = np.ascontiguousarray(a, dtype=np.float32)
    if missing or extra or wrong:
        parts = [f"{what}: {', '.join(keys)}" for what, keys in (("missing", missing), ("unexpected", extra), ("wrong shape", wrong)) if keys]
        raise ValueError(f"lpips {net} weights: " + "; ".join(parts))
    return out


def pack(net, weights):
    """canonical() in the layout the kernels read: {"conv_w": [(Kp, C_out)], "conv_b": [(C_out,)], "lin": [(C_k,)]} float32 numpy
    arrays; row (ky * k + kx) * C_in + c of conv_w[i] is weight[:, c, ky, kx], and the rows from k * k * C_in up to Kp (the next
    multiple of 16) are zero."""
    w = canonical(net, weights)
    conv_w = []
    for i, (ci, co, ks) in enumerate(CONVS[net]):
        K = ks * ks * ci
        p = np.zeros(((K + K_STEP - 1) // K_STEP * K_STEP, co), np.float32)
        p[:K] = w[f"conv{i}.weight"].transpose(2, 3, 1, 0).reshape(K, co)
        conv_w.append(p)
    return {"conv_w": conv_w, "conv_b": [w[f"conv{i}.bias"] for i in range(len(CONVS[net]))], "lin": [w[f"lin{k}.weight"] for k in range(5)]}


def _checked(images, gt, net):
    if not (torch.is_tensor(images) and torch.is_tensor(gt) and images.is_cuda and gt.is_cuda):
        raise RuntimeError("lpips needs CUDA/HIP tensors (dg-mesh_amd has no CPU path for its kernels)")
    if images.dtype != torch.float32 or gt.dtype != torch.float32:
        raise RuntimeError("lpips needs float32 tensors")
    if images.dim() == 3:
        images = images[None]
    if images.dim() != 4 or gt.dim() != 3 or images.shape[1:] != gt.shape or images.device != gt.device or gt.shape[0] != 3:
        raise ValueError(f"lpips: images {tuple(images.shape)} must be (3, H, W) or (B, 3, H, W) matching gt {tuple(gt.shape)} "
                         "on the same device")
    H, W = gt.shape[1:]
    if min(H, W) < MIN_SIDE[net]:
        raise ValueError(f"lpips: the {net} stack needs min(H, W) >= {MIN_SIDE[net]}, got {H}x{W}")
    return images.contiguous(), gt.contiguous()


class LPIPS:
    """LPIPS(net, weights, device): net "alex" or "vgg", weights as described in the module's docstring.  The weights are packed and
    copied to `device` once."""

    def __init__(self, net, weights, device="cuda"):
        _check_net(net)
        self.net, self.device = net, torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("lpips needs a CUDA/HIP device (dg-mesh_amd has no CPU path for its kernels)")
        packed = pack(net, weights)
        self._tensors = {k: [torch.from_numpy(a).to(self.device) for a in v] for k, v in packed.items()}
        ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        self._ptrs = tuple(ptrs(self._tensors[k]) for k in ("conv_w", "conv_b", "lin"))

    def _into(self, images, gt, out):
        """images (B, 3, H, W), gt (3, H, W) as _checked returns them; out: contiguous (B, 6) float64 view, written in place."""
        L = _lib.lib()
        if images.device != self._tensors["lin"][0].device:
            raise ValueError(f"lpips: the images are on {images.device}, the weights on {self._tensors['lin'][0].device}")
        B, _, H, W = images.shape
        code = NETS.index(self.net)
        ws = torch.empty(L.dgm_lpips_workspace_bytes(code, B, H, W), dtype=torch.uint8, device=images.device)
        with _lib.device_guard(images.device):
            _lib.check(L.dgm_lpips(code, *self._ptrs, ctypes.c_void_p(images.data_ptr()), ctypes.c_void_p(gt.data_ptr()), B, H, W,
                                   ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(out.data_ptr()), _lib.stream_ptr()))

    def __call__(self, images, gt):
        """`images` ((3, H, W) or (B, 3, H, W)) against ONE target `gt` (3, H, W), fp32 CUDA/HIP tensors in [0, 1] ->
        {"lpips": (B,) float64 device tensor, "layers": (B, 5) the five tap terms it is the sum of}.  Nothing is read back; the
        results are bit-reproducible and independent of B."""
        images, gt = _checked(images, gt, self.net)
        out = torch.empty((images.shape[0], 6), dtype=torch.float64, device=images.device)
        self._into(images, gt, out)
        return {"lpips": out[:, 5], "layers": out[:, :5]}


def convert(net, backbone, lin, out):
    """Write the .npz of layout (c) from a torchvision state dict file and the lpips package's linear-layer file."""
    np.savez(out, **canonical(net, [backbone, lin]))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m dgmesh_amd.lpips")
    sub = ap.add_subparsers(dest="command", required=True)
    cv = sub.add_parser("convert", help="merge a torchvision state dict and the lpips linear-layer file into one .npz")
    cv.add_argument("--net", required=True, choices=NETS)
    cv.add_argument("--backbone", required=True)
    cv.add_argument("--lin", required=True)
    cv.add_argument("--out", required=True)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    convert(a.net, a.backbone, a.lin, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
