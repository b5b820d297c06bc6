"""Red-zone tests of the winding number (csrc/mesh_inside.hip), run as tests/test_redzone.py runs the other kernels: its run_case
puts every input at its exact size between guard zones, hands out every tensor the wrappers allocate -- the scratch at exactly
dgm_wind_scratch_bytes -- at exactly the requested size, and asserts that all guards are intact, that the outputs equal those of a
plain run byte for byte, that they do not depend on what the buffers held before, and that the scratch may start off the 256-byte
grid.  Sizes (N, F): ragged against the wave (64), the workgroup and the chunk (256) and the slice (16384 faces: one slice writes w
directly, two go through the slice sums in scratch).  A passing case enters dgm_wind_scratch_bytes into test_redzone's record of
covered size functions, which that file's last test reads."""
import numpy as np
import pytest

from conftest import pkg
from test_redzone import L, dev, run_case

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (65, 130), (257, 255), (300, 16385), (4097, 257)]  # WN_THREADS = WN_CHUNK 256, WN_SLICE 16384


def scene(N, F):
    """Random triples over a few vertices, some indices outside [0, V) (dropped before any use) and a NaN vertex; queries around them."""
    rng = np.random.default_rng(N * 7919 + F)
    V = max(3, min(F, 1000))
    verts = rng.standard_normal((V, 3)).astype(np.float32)
    faces = rng.integers(0, V, (F, 3)).astype(np.int32)
    faces[::11, 0], faces[5::13, 2] = -1, V
    if V > 3:
        verts[V // 2, 1] = np.nan
    return rng.standard_normal((N, 3)).astype(np.float32), verts, faces


@pytest.mark.parametrize("N,F", SIZES)
def test_winding_number(N, F):
    M = pkg("mesh_inside")
    points, verts, faces = scene(N, F)
    assert M.batch_rows(F) >= N  # one launch: the scratch is the size function's at (N, F)
    run_case(lambda i: [M.winding_number(i["points"], i["verts"], i["faces"]), M.contains(i["points"], i["verts"], i["faces"], absolute=True)],
             {"points": dev(points), "verts": dev(verts), "faces": dev(faces)}, [("dgm_wind_scratch_bytes", L().dgm_wind_scratch_bytes(N, F))])
