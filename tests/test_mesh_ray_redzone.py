"""Red-zone tests of ray casting (csrc/mesh_ray.hip), run as tests/test_redzone.py runs the other kernels: its run_case puts every input
at its exact size between guard zones, hands out every tensor the wrappers allocate -- the structure at exactly dgm_ray_accel_bytes and
the build's scratch at exactly dgm_ray_build_scratch_bytes -- at exactly the requested size, and asserts that all guards are intact,
that the outputs equal those of a plain run byte for byte, that they do not depend on what the buffers held before (the structure's
padding behind F and the scratch included), and that the scratch and the structure may start off the 256-byte grid.  Sizes (N, F):
ragged against the wave (64), the workgroup and the chunk (256) and the sort's tile (2048 keys).  A passing case enters the two size
functions into test_redzone's record of covered size functions, which that file's last test reads."""
import numpy as np
import pytest

from _ray_ref import soup
from conftest import pkg
from test_redzone import L, dev, run_case

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (65, 130), (257, 255), (300, 513), (4097, 257)]  # RC_THREADS = RC_CHUNK 256


def scene(N, F):
    """Random triples over a few vertices, some indices outside [0, V) (never hit) and a NaN vertex; rays around them, one of them
    without a direction and one with a NaN."""
    rng = np.random.default_rng(N * 7919 + F)
    verts, faces = soup(F, seed=N * 31 + F)
    origins, dirs = rng.standard_normal((N, 3)).astype(np.float32), rng.standard_normal((N, 3)).astype(np.float32)
    dirs[N // 2] = 0
    origins[N // 3, 1] = np.nan
    return origins, dirs, verts, faces


@pytest.mark.parametrize("N,F", SIZES)
def test_ray_cast_and_occluded(N, F):
    M = pkg("mesh_ray")
    origins, dirs, verts, faces = scene(N, F)

    def call(i):
        mesh = M.RayMesh(i["verts"], i["faces"])  # the build: the structure and its scratch come from the guarded allocator
        args = (i["origins"], i["dirs"], i["verts"], i["faces"], 0.05, 3.0)
        out = list(M.ray_cast(*args, accel=mesh)) + [M.occluded(*args, accel=mesh)]
        out += list(M.ray_cast(*args, accel=None)) + [M.occluded(*args, accel=None)]
        assert all(bool((out[k] == out[4 + k]).all()) for k in range(4))  # both paths, one answer (+inf == +inf)
        return out + [mesh.accel]  # the structure itself: every byte written, the same from run to run

    run_case(call, {"origins": dev(origins), "dirs": dev(dirs), "verts": dev(verts), "faces": dev(faces)},
             [("dgm_ray_accel_bytes", L().dgm_ray_accel_bytes(F)), ("dgm_ray_build_scratch_bytes", L().dgm_ray_build_scratch_bytes(F))])
