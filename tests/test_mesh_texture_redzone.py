"""Red-zone tests of texture sampling and the texture atlas (csrc/mesh_texture.hip), run as tests/test_redzone.py runs the other kernels:
its run_case puts every input at its exact size between guard zones, hands out every tensor the wrappers allocate at exactly the
requested size, and asserts that all guards are intact, that the outputs equal those of a plain run byte for byte and that they do not
depend on what the buffers held before.  The kernels take no scratch, so there is no size function to cover.

texture: forward and backward; n ragged against the wave (64) and the workgroup (256), the 1 x 1 texture, C = 4 both 16-byte aligned
(the 16-byte path) and 4 bytes off (the scalar path); uv with NaN, +-inf and +-1e30 rows and values far outside [0, 1].
dtex is summed with fp32 atomics: with dout >= 0 every term of a texel's sum has one sign, so two runs differ by at most
2 (m + 3) 2^-24 of the texel's own value, m <= 4 n terms (_texture_ref.dtex_bound); every other output is compared byte for byte."""
import numpy as np
import pytest
import torch

import _edges_ref as E
from conftest import pkg
from test_redzone import dev, run_case

pytestmark = pytest.mark.gpu

SAMPLES = [1, 63, 65, 257]  # the wave 64, TX_THREADS 256
TEXTURES = [(1, 1, 3), (5, 7, 3), (9, 8, 4), (1, 1, 4)]
MODES = [("linear", "wrap"), ("linear", "clamp"), ("linear", "zero"), ("nearest", "wrap"), ("nearest", "clamp"), ("nearest", "zero")]


def texture_inputs(n, Ht, Wt, C):
    rng = np.random.default_rng(n * 131 + Ht * 17 + Wt + C)
    uv = rng.uniform(-3.0, 4.0, (1, n, 2)).astype(np.float32)
    bad = np.array([(np.nan, 0.3), (0.3, np.inf), (-np.inf, 0.5), (1e30, -1e30), (-1e30, 0.25), (3e38, 3e38), (0.0, 1.0)], np.float32)
    if n > 1:
        uv[0, :min(n, len(bad))] = bad[:n]
    return {"tex": dev(rng.standard_normal((1, Ht, Wt, C)).astype(np.float32)), "uv": dev(uv),
            "dout": dev(rng.uniform(0.5, 1.5, (1, n, C)).astype(np.float32))}


@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("Ht,Wt,C", TEXTURES)
@pytest.mark.parametrize("n", SAMPLES)
def test_texture(n, Ht, Wt, C, offset):
    MR = pkg("mesh_raster")

    def run(i):
        outs = []
        for filter_mode, boundary_mode in MODES:
            tex, uv = i["tex"].detach().requires_grad_(True), i["uv"].detach().requires_grad_(True)
            out = MR.texture(tex, uv, filter_mode=filter_mode, boundary_mode=boundary_mode)
            outs += [out.detach()] + list(torch.autograd.grad(out, [tex, uv], grad_outputs=i["dout"]))
        return outs

    tol_dtex = 2 * (4 * n + 3) * 2.0 ** -24
    run_case(run, texture_inputs(n, Ht, Wt, C), tols={3 * k + 1: tol_dtex for k in range(len(MODES))}, offset=offset)


@pytest.mark.parametrize("F,size,cell", [(1, 4, 4), (2, 5, 5), (7, 23, 11), (65, 25, 4), (320, 72, 5), (320, 65, 5)])  # 25 = 6 cells + 1 texel
def test_atlas(F, size, cell):
    MT = pkg("mesh_texture")
    verts, faces = E.icosphere(2)
    faces = faces[:F].copy()
    if F > 2:
        faces[1, 0], faces[F - 1, 2] = -1, len(verts)  # indices outside [0, V): dropped before any use
    attr = np.random.default_rng(F).standard_normal((len(verts), 3)).astype(np.float32)
    attr[5, 1] = np.nan
    atlas = MT.Atlas(size, cell, size // cell, F)
    assert (size // cell) ** 2 >= (F + 1) // 2
    run_case(lambda i: [MT.atlas_uv(atlas, i["attr"].device)] + list(MT.atlas_interpolate(atlas, i["attr"], i["faces"])),
             {"attr": dev(attr), "faces": dev(faces)})


def test_bake_allocates_nothing_it_overruns():
    """bake end to end between guards: positions, ownership, the gathered points, the texture."""
    MT = pkg("mesh_texture")
    verts, faces = E.icosphere(1)
    run_case(lambda i: list(MT.bake(i["verts"], i["faces"], lambda p: p * 0.4 + 0.5, cell=5, chunk=257)[:2]),
             {"verts": dev(verts), "faces": dev(faces)})
