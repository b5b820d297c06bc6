"""Differentiable marching cubes with the call shape of diso.DiffMC (the reference's mesh extraction, R/utils/renderer.py:171,
R/scene/gaussian_model_dpsr_dynamic_anchor.py:703, :831-856; R/ = the reference's dgmesh/):

    DiffMC(dtype=torch.float32)(grid, deform=None, isovalue=0.0, normalize=True) -> verts (V, 3) float32, faces (F, 3) int32

The count, emit and backward passes are HIP kernels of libdgmesh_hip (csrc/marching_cubes.hip) behind torch.autograd.Function,
differentiable w.r.t. `grid` and `deform`.  float32, CUDA/HIP tensors only -- no CPU fallback.

Conventions chosen here (diso is not vendored, so they are this project's, not checked against diso's):
  * grid (X, Y, Z), x = dim 0; point (i, j, k) sits at (i, j, k), plus deform[i, j, k] (shape (X, Y, Z, 3)) when given;
  * a point is inside iff f < isovalue (NaN: outside); the vertex on a crossed edge a->b is p_a + t (p_b - p_a) with
    t = (iso - fa) / (fb - fa); `normalize` divides each coordinate by (dim - 1) of its axis, mapping the grid onto [0, 1]^3;
  * faces are wound so that (v1 - v0) x (v2 - v0) points from f < iso towards f >= iso; ambiguous faces keep inside corners
    separate, so the mesh of a field that is outside on the grid's boundary is closed;
  * vertices are ordered by (owning grid point, axis), faces by (cell, case-table order): the output is identical run to run.
One host synchronisation per forward: the 8-byte read-back of {V, F} that sizes the outputs.
"""

import torch
import torch.nn as nn

from . import _lib


def _st():
    return _lib.stream_ptr()


def _check(grid, deform):
    if not grid.is_cuda or (deform is not None and not deform.is_cuda):
        raise RuntimeError("DiffMC: grid / deform must be CUDA/HIP tensors (dg-mesh_amd has no CPU path)")
    if grid.dtype != torch.float32 or (deform is not None and deform.dtype != torch.float32):
        raise RuntimeError("DiffMC: float32 only")
    if grid.dim() != 3 or min(grid.shape) < 2:
        raise RuntimeError(f"DiffMC: grid must be (X, Y, Z) with every dimension >= 2, got {tuple(grid.shape)}")
    if deform is not None and (tuple(deform.shape) != tuple(grid.shape) + (3,) or deform.device != grid.device):
        raise RuntimeError(f"DiffMC: deform must be (X, Y, Z, 3) on the grid's device, got {tuple(deform.shape)}")


class _MarchingCubes(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid, deform, iso, normalize):
        L = _lib.lib()
        grid = grid.contiguous()
        deform = deform.contiguous() if deform is not None else None
        X, Y, Z = (int(s) for s in grid.shape)
        nbytes = int(L.dgm_mc_scratch_bytes(X, Y, Z))
        if nbytes == 0:
            raise RuntimeError(f"DiffMC: grid {(X, Y, Z)} is too large (5 * X * Y * Z must fit in int32)")
        dev = grid.device
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        with _lib.device_guard(dev):
            _lib.check(L.dgm_mc_count(X, Y, Z, _lib.vp(grid), float(iso), _lib.vp(scratch), _lib.vp(counts), _st()))
            V, F = counts.tolist()  # the one host synchronisation: the output sizes
            verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
            faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
            _lib.check(L.dgm_mc_emit(X, Y, Z, _lib.vp(grid), _lib.vp(deform), float(iso), int(bool(normalize)), _lib.vp(scratch), V, F,
                                     _lib.vp(verts), _lib.vp(faces), _st()))
        ctx.save_for_backward(grid, deform, scratch)
        ctx.iso, ctx.normalize, ctx.V = float(iso), bool(normalize), V
        ctx.mark_non_differentiable(faces)
        return verts, faces

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dverts, _dfaces):
        grid, deform, scratch = ctx.saved_tensors
        X, Y, Z = (int(s) for s in grid.shape)
        dverts = dverts.contiguous().float() if dverts is not None else torch.zeros((ctx.V, 3), device=grid.device)
        dgrid = torch.empty_like(grid)
        ddeform = torch.empty_like(deform) if deform is not None else None
        with _lib.device_guard(grid.device):
            _lib.check(_lib.lib().dgm_mc_backward(X, Y, Z, _lib.vp(grid), _lib.vp(deform), ctx.iso, int(ctx.normalize), _lib.vp(scratch), ctx.V,
                                                  _lib.vp(dverts), _lib.vp(dgrid), _lib.vp(ddeform), _st()))
        return dgrid, ddeform, None, None


def marching_cubes(grid, deform=None, isovalue=0.0, normalize=True):
    """verts (V, 3) float32, faces (F, 3) int32 of the surface f = isovalue (module docstring for the conventions)."""
    _check(grid, deform)
    return _MarchingCubes.apply(grid, deform, isovalue, normalize)


class DiffMC(nn.Module):
    """diso.DiffMC's interface: DiffMC(dtype=torch.float32)(grid, deform=None, isovalue=0.0, normalize=True) -> (verts, faces)."""

    def __init__(self, dtype=torch.float32):
        super().__init__()
        if dtype != torch.float32:
            raise RuntimeError("DiffMC: float32 only")
        self.dtype = dtype

    def forward(self, grid, deform=None, isovalue=0.0, normalize=True):
        return marching_cubes(grid, deform, isovalue, normalize)
