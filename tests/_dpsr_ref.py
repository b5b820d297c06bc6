"""Float64 torch restatement of the reference's DPSR (R/ = the reference's dgmesh/), the comparison for the HIP kernels of
csrc/dpsr.hip and the DPSR module of dg-mesh_amd/dpsr.py.  Autograd supplies every adjoint; runs on the CPU or on the device.

    fftfreqs              R/nvdiffrast_utils/dpsr_utils.py:25-45
    spec_gaussian_filter  R/nvdiffrast_utils/dpsr_utils.py:56-62
    grid_interp           R/nvdiffrast_utils/dpsr_utils.py:69-118
    point_rasterize       R/nvdiffrast_utils/dpsr_utils.py:143-198 (with scatter_to_grid :120-141)
    dpsr (forward)        R/nvdiffrast_utils/dpsr.py:28-69

The cell indices and the cell positions are the reference's fp32 values (cube = float32(1 / res), q = p / cube, floor(q),
fmod(ceil(q), res), position = index * cube); the weights |p - position| / cube and everything after them are float64.  One
difference of domain: where q rounds up to res (p one ulp below 1 on some grids) the reference indexes out of range; here the
low index wraps like the high one (the periodic grid the kernels implement).

Every function that does arithmetic takes a `dtype` (default float64): float32 gives a single-precision run of the same
arithmetic on the same cells, the yardstick of tests/test_mesh_chain.py."""
import numpy as np
import torch


def fftfreqs(res, device=None, dtype=torch.float64):
    """(R, R, R//2+1, 3) integer frequencies: fftfreq on dims 0, 1 and rfftfreq on dim 2 (dpsr_utils.py:25-45)."""
    f = [torch.tensor(np.fft.fftfreq(res, d=1 / res), dtype=dtype, device=device) for _ in range(2)]
    f.append(torch.tensor(np.fft.rfftfreq(res, d=1 / res), dtype=dtype, device=device))
    return torch.stack(torch.meshgrid(*f, indexing="ij"), -1)


def spectral(ras_s, res, sig):
    """Phi = sum_d -i omega_d G Nhat_d / (Lap + 1e-6), Phi(0) = 0 (dpsr.py:41-54).  ras_s: (3, R, R, R//2+1) complex128, or
    complex64 for the float32 run."""
    omega = fftfreqs(res, ras_s.device, ras_s.real.dtype)
    dis = torch.sqrt((omega ** 2).sum(-1))
    G = torch.exp(-0.5 * (sig * 2 * dis / res) ** 2)                       # spec_gaussian_filter (dpsr_utils.py:56-62)
    omega = omega * (2 * np.pi)
    lap = -(omega ** 2).sum(-1)
    div = sum(-1j * ras_s[d] * G * omega[..., d] for d in range(3))
    dc = torch.ones_like(lap)
    dc[0, 0, 0] = 0.0
    return div / (lap + 1e-6) * dc


def corners(V, res, dtype=torch.float64, cells=None):
    """Reference cell arithmetic (dpsr_utils.py:160-181) for (n, 3) points -> flat indices (n, 8) int64, weights (n, 8).
    Corner k takes bit (2 - d) of k as its side along dim d (the com_ order).  The weights are `dtype` and differentiable in V.
    cells: the (n, 3) float32 points whose cells are used (default: V rounded to float32) -- a caller that perturbs V, or holds
    the device's own float32 points, keeps the cell choice fixed with it."""
    V = V.to(dtype)
    p32 = (V if cells is None else cells).detach().to(torch.float32)
    cube = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(res), dtype=torch.float32)
    cube = cube.to(V.device)
    q = p32 / cube
    size = torch.tensor(float(res), dtype=torch.float32, device=V.device)
    ind0 = torch.floor(q)
    ind1 = torch.fmod(torch.ceil(q), size)
    x0 = (ind0 * cube).to(dtype)                                          # cell positions: fp32 as in the reference
    x1 = ((ind0 + 1) * cube).to(dtype)
    ind0 = torch.fmod(ind0, size).long()
    ind1 = ind1.long()
    if bool((ind0 < 0).any()) or bool((ind1 < 0).any()):
        raise ValueError("dpsr restatement: points must lie in [0, 1)")
    c = cube.to(dtype)
    a0 = torch.abs(V - x1) / c                                             # weight of the low corner: distance to the high one
    a1 = torch.abs(V - x0) / c
    idx, w = [], []
    for k in range(8):
        b = [(k >> 2) & 1, (k >> 1) & 1, k & 1]
        ii = [ind1[:, d] if b[d] else ind0[:, d] for d in range(3)]
        ww = [a1[:, d] if b[d] else a0[:, d] for d in range(3)]
        idx.append((ii[0] * res + ii[1]) * res + ii[2])
        w.append(ww[0] * ww[1] * ww[2])
    return torch.stack(idx, 1), torch.stack(w, 1)


def point_rasterize(V, N, res, dtype=torch.float64, cells=None):
    """(n, 3) points, (n, 3) values -> (3, R, R, R) `dtype` (dpsr_utils.py:143-198, one batch)."""
    idx, w = corners(V, res, dtype, cells)
    N = N.to(dtype)
    cells = res ** 3
    out = []
    for f in range(3):
        g = torch.zeros(cells, dtype=dtype, device=V.device)
        out.append(g.index_add(0, idx.reshape(-1), (w * N[:, f:f + 1]).reshape(-1)))
    return torch.stack(out, 0).reshape(3, res, res, res)


def grid_interp(phi, V, dtype=torch.float64, cells=None):
    """phi (R, R, R), points (n, 3) -> (n,) trilinear values (dpsr_utils.py:69-118, one feature)."""
    idx, w = corners(V, phi.shape[0], dtype, cells)
    return (phi.reshape(-1)[idx] * w).sum(1)


def dpsr(V, N, res, sig, shift=True, scale=True, dtype=torch.float64, cells=None):
    """DPSR.forward for one cloud (dpsr.py:40-69): splat, rfftn, spectral solve, irfftn, shift by the mean at the points, scale.
    dtype: float64, or float32 for a single-precision run of the same arithmetic; cells: see corners()."""
    ras_p = point_rasterize(V, N, res, dtype, cells)
    ras_s = torch.fft.rfftn(ras_p, dim=(1, 2, 3))
    phi = torch.fft.irfftn(spectral(ras_s, res, sig), s=(res, res, res), dim=(0, 1, 2))
    if shift or scale:
        if shift:
            phi = phi - grid_interp(phi, V, dtype, cells).mean()
        fv0 = phi[0, 0, 0]
        if scale:
            phi = -phi / torch.abs(fv0) * 0.5
    return phi


def noisy_sphere(n, seed, radius=0.3):
    """An oriented noisy sphere in (0, 1)^3: (n, 3) float32 points and (n, 3) float32 outward normals."""
    rng = np.random.RandomState(seed)
    d = rng.randn(n, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    V = 0.5 + radius * d * (1 + 0.02 * rng.randn(n, 1))
    N = d + 0.05 * rng.randn(n, 3)
    return V.astype(np.float32), N.astype(np.float32)
