"""Red-zone tests of mesh repair (csrc/mesh_repair.hip), run as tests/test_redzone.py runs the other kernels: its run_case puts every
input at its exact size between guard zones, hands out every tensor the wrappers allocate -- the scratch at exactly
dgm_mesh_orient_scratch_bytes, dgm_mesh_fill_scratch_bytes and dgm_mesh_edges_scratch_bytes -- at exactly the requested size, and
asserts that all guards are intact, that the outputs equal those of a plain run byte for byte, that they do not depend on what the
buffers held before, and that the scratch may start off the 256-byte grid.  Sizes: those of tests/test_mesh_edges_redzone.py, V and F
ragged against the wave (64), the workgroup (256) and the scan tile (4096).  A passing case enters the two new size functions into
test_redzone's record of covered size functions, which that file's last test reads."""
import numpy as np
import pytest

import _edges_ref as E
from conftest import pkg
from test_mesh_edges_redzone import SIZES
from test_redzone import L, dev, run_case

pytestmark = pytest.mark.gpu

RESERVED = 15  # vertices at the end that the random faces leave alone


def mesh(V, F):
    """Random triples: non-manifold edges, same-direction pairs, chains on the boundary and a few indices outside [0, V) (dropped
    before any use).  From V = 65 on, the last faces are two lone triangles (rims of 3) and a wheel of 8 spokes (a rim of 8, filled
    around a centroid) on the last 15 vertices, so that every path of the fill runs."""
    rng = np.random.default_rng(V * 7919 + F)
    verts = rng.standard_normal((V, 3)).astype(np.float32)
    holes = V >= 65
    faces = rng.integers(0, V - RESERVED if holes else V, (F, 3)).astype(np.int32)
    faces[::11, 0], faces[5::13, 2] = -1, V
    if holes:
        t, hub = V - RESERVED, V - 9
        rim = hub + 1 + np.arange(8)
        faces[-10:] = np.concatenate([[[t, t + 1, t + 2], [t + 3, t + 4, t + 5]], np.stack([np.full(8, hub), rim, np.roll(rim, -1)], 1)])
    return verts, faces


def sizes(V, F, faces, fill=True):
    B = E.edge_table(faces, V)["info"]["boundary_edges"]
    out = [("dgm_mesh_edges_scratch_bytes", L().dgm_mesh_edges_scratch_bytes(V, F)),
           ("dgm_mesh_orient_scratch_bytes", L().dgm_mesh_orient_scratch_bytes(V, F))]
    return out + ([("dgm_mesh_fill_scratch_bytes", L().dgm_mesh_fill_scratch_bytes(V, B))] if fill else [])


@pytest.mark.parametrize("outward", [True, False])
@pytest.mark.parametrize("V,F", SIZES)
def test_orient(V, F, outward):
    M = pkg("mesh_repair")
    verts, faces = mesh(V, F)

    def call(i):
        f, flipped, _ = M.orient_faces(i["verts"], i["faces"], outward=outward)
        return [f, flipped]

    run_case(call, {"verts": dev(verts), "faces": dev(faces)}, sizes(V, F, faces, fill=False))


@pytest.mark.parametrize("orient", [True, False])
@pytest.mark.parametrize("V,F", SIZES)
def test_repair(V, F, orient):
    M = pkg("mesh_repair")
    verts, faces = mesh(V, F)

    def call(i):
        v, f, info = M.repair_mesh(i["verts"], i["faces"], orient=orient, max_hole_edges=8)
        assert info["holes_filled"] >= (3 if V >= 65 else 0) and info["verts_added"] >= (1 if V >= 65 else 0)
        return [v, f]

    want = [s for s in sizes(V, F, faces) if orient or s[0] != "dgm_mesh_orient_scratch_bytes"]
    run_case(call, {"verts": dev(verts), "faces": dev(faces)}, want)
