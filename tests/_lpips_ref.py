"""LPIPS 0.1 restated with torch.nn.functional on the CPU (fp64 by default), from the definition in include/dgmesh_hip.h -- written
from that definition, not from any package -- and seeded weights for it.

  x -> ((2x - 1) - shift) / scale, shift = (-0.030, -0.088, -0.188), scale = (0.458, 0.448, 0.450)
  alex: conv 3->64 k11 s4 p2 (tap), maxpool 3/2, conv 64->192 k5 p2 (tap), maxpool 3/2, conv 192->384 k3 p1 (tap),
        conv 384->256 k3 p1 (tap), conv 256->256 k3 p1 (tap)
  vgg : k3 p1 throughout: 64, 64 (tap), maxpool 2/2, 128, 128 (tap), maxpool, 256 x3 (tap), maxpool, 512 x3 (tap), maxpool, 512 x3 (tap)
  every convolution is followed by bias and ReLU; the max-pools floor their output size
  tap term = mean over pixels of sum_c w_c (a_c / (|a|_2 + 1e-10) - b_c / (|b|_2 + 1e-10))^2; LPIPS = the sum of the five

Three reference-only variants, each a detail an implementation can get wrong: eps_inside (the 1e-10 under the square root),
ceil_mode (pools that round their output size up) and normalize=False (no 2x - 1)."""
import math

import torch
import torch.nn.functional as F

SHIFT, SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)
# (C_out, kernel, stride, padding, pool window in front or 0, is a tap) per convolution, and its index in torchvision's `features`
NETS = {
    "alex": (((64, 11, 4, 2, 0, True), (192, 5, 1, 2, 3, True), (384, 3, 1, 1, 3, True), (256, 3, 1, 1, 0, True), (256, 3, 1, 1, 0, True)),
             (0, 3, 6, 8, 10)),
    "vgg": (tuple((c, 3, 1, 1, p, t) for c, p, t in (
        (64, 0, False), (64, 0, True), (128, 2, False), (128, 0, True), (256, 2, False), (256, 0, False), (256, 0, True),
        (512, 2, False), (512, 0, False), (512, 0, True), (512, 2, False), (512, 0, False), (512, 0, True))),
        (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)),
}


def seeded_weights(net, seed, width=1.0):
    """State-dict layout (a): features.{N}.weight/bias (He-normal weights, N(0, 0.1) biases) and lin{k}.model.1.weight
    (1, C, 1, 1), uniform in [0, 1) -- the published ones are non-negative.  width scales every channel count but the input's."""
    g = torch.Generator().manual_seed(seed)
    layers, index = NETS[net]
    sd, cin, k = {}, 3, 0
    for (cout, ks, _, _, _, tap), n in zip(layers, index):
        cout = max(1, int(cout * width))
        sd[f"features.{n}.weight"] = torch.randn((cout, cin, ks, ks), generator=g) * math.sqrt(2.0 / (cin * ks * ks))
        sd[f"features.{n}.bias"] = torch.randn((cout,), generator=g) * 0.1
        if tap:
            sd[f"lin{k}.model.1.weight"] = torch.rand((1, cout, 1, 1), generator=g)
            k += 1
        cin = cout
    return sd


def features(net, sd, x, ceil_mode=False):
    """The five taps of x (n, 3, H, W), already scaled, in x's dtype."""
    layers, index = NETS[net]
    taps = []
    for (_, ks, stride, pad, pool, tap), n in zip(layers, index):
        if pool:
            x = F.max_pool2d(x, pool, 2, ceil_mode=ceil_mode)
        x = F.relu(F.conv2d(x, sd[f"features.{n}.weight"].to(x.dtype), sd[f"features.{n}.bias"].to(x.dtype), stride=stride, padding=pad))
        if tap:
            taps.append(x)
    return taps


def tap_term(a, b, w, eps_inside=False):
    """a (n, C, h, w) against b (1, C, h, w), w (C,) -> (n,)"""
    if eps_inside:
        unit = lambda t: t / torch.sqrt((t * t).sum(1, keepdim=True) + 1e-10)
    else:
        unit = lambda t: t / (torch.sqrt((t * t).sum(1, keepdim=True)) + 1e-10)
    d = (unit(a) - unit(b)) ** 2
    return (d * w.reshape(1, -1, 1, 1)).sum(1).mean((1, 2))


def lpips_ref(net, sd, images, gt, dtype=torch.float64, eps_inside=False, ceil_mode=False, normalize=True):
    """images (B, 3, H, W), gt (3, H, W) in [0, 1] -> (B, 6) tensor of `dtype`: the five tap terms and their sum."""
    x = torch.cat((images, gt[None])).detach().cpu().to(dtype)
    if normalize:
        x = 2 * x - 1
    x = (x - torch.tensor(SHIFT, dtype=dtype).reshape(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dtype).reshape(1, 3, 1, 1)
    taps = features(net, sd, x, ceil_mode)
    terms = [tap_term(t[:-1], t[-1:], sd[f"lin{k}.model.1.weight"].to(dtype).reshape(-1), eps_inside) for k, t in enumerate(taps)]
    terms = torch.stack(terms, 1)
    return torch.cat((terms, terms.sum(1, keepdim=True)), 1)


def make_images(H, W, seed=0):
    """A smooth random target and four images: the target plus noise at three amplitudes, and one independent smooth image."""
    g = torch.Generator().manual_seed(seed)
    smooth = lambda: F.interpolate(torch.rand((1, 3, H // 8 + 2, W // 8 + 2), generator=g), size=(H, W), mode="bicubic",
                                   align_corners=False)[0].clamp(0.0, 1.0)
    gt = smooth()
    noisy = [(gt + amp * torch.randn((3, H, W), generator=g)).clamp(0.0, 1.0) for amp in NOISE]
    return torch.stack(noisy + [smooth()]).float().contiguous(), gt.float().contiguous()


NOISE = (0.1, 0.2, 0.4)
