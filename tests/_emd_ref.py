"""Dense NumPy restatement of the reference's approximate EMD: approxmatchkernel followed by matchcostkernel
(R/metrics/pytorch_structural_losses/src/approxmatch.cu:3-182 and 184-224, R/ = the reference's dgmesh/), written from that file.
Test infrastructure only: it forms the n x m matrices the product never does.

dtype=np.float64 is the reference the kernel is held to; dtype=np.float32 is the same code in the kernel's own precision (numpy's
exp and pairwise sums instead of the fast exponential and the kernel's summation order), which shows how much of the kernel's
distance to fp64 the number format alone explains."""
import numpy as np


def pair_d2(xyz1, xyz2, dtype):
    """(n, m) squared distances, (dx*dx + dy*dy) + dz*dz as approxmatch.cu:54 orders it."""
    a = np.asarray(xyz1, dtype)[:, None, :]
    b = np.asarray(xyz2, dtype)[None, :, :]
    d = b - a
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def approx_match_cost(xyz1, xyz2, dtype=np.float64):
    """xyz1 (n, 3), xyz2 (m, 3) -> (cost, (sum remainL, sum remainR)) as Python floats."""
    dt = np.dtype(dtype).type
    n, m = len(xyz1), len(xyz2)
    d2 = pair_d2(xyz1, xyz2, dtype)
    dist = np.sqrt(d2)                                   # :207
    # :5-12 -- INTEGER division: n = 3, m = 2 gives multiR = 1
    multiL, multiR = (1, n // m) if n >= m else (m // n, 1)
    remainL = np.full(n, multiL, dtype)                  # :18-19
    remainR = np.full(m, multiR, dtype)                  # :20-21
    eps = dt(1e-9)
    cost = dt(0)
    for j in range(7, -2, -1):                           # :24, j = 7 .. -1; the j == -2 branch of :26 is never reached
        level = dt(-(4.0 ** j))                          # :25
        W = np.exp(level * d2)                           # :54-55
        ratioL = remainL / (eps + W @ remainR)           # :37, :56, :61
        sumr = remainR * (W.T @ ratioL)                  # :100-101, :106
        ratioR = np.minimum(remainR / (sumr + eps), dt(1)) * remainR   # :107-108
        remainR = np.maximum(dt(0), remainR - sumr)      # :109
        w = (W * ratioL[:, None]) * ratioR[None, :]      # :154 (ratioL[k] only for k < n: the read past n at :148 is not restated)
        cost = cost + (w * dist).sum(dtype=dtype)        # :155 accumulated over levels, :208
        remainL = np.maximum(dt(0), remainL - w.sum(axis=1, dtype=dtype))   # :156, :162
    return float(cost), (float(remainL.sum(dtype=np.float64)), float(remainR.sum(dtype=np.float64)))


def sphere_cloud(count, radius=1.0, center=(0.0, 0.0, 0.0), seed=0):
    """`count` seeded points on a sphere, float32."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((count, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * radius + np.asarray(center)).astype(np.float32)


def chamfer_sides(a, b):
    """fp64 brute force: (min over b of d2 for each a, min over a of d2 for each b)."""
    d2 = pair_d2(a, b, np.float64)
    return d2.min(axis=1), d2.min(axis=0)
