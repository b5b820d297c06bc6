"""Red-zone tests of the edge table and the smoothing step (csrc/mesh_edges.hip), run as tests/test_redzone.py runs the other kernels:
its run_case puts every input at its exact size between guard zones, hands out every tensor the wrappers allocate -- the scratch at
exactly dgm_mesh_edges_scratch_bytes -- at exactly the requested size, and asserts that all guards are intact, that the outputs equal
those of a plain run byte for byte, that they do not depend on what the buffers held before, and that the scratch may start off the
256-byte grid.  Sizes: V, F and E ragged against the wave (64), the workgroup (256) and the scan tile (4096).  A passing case enters
dgm_mesh_edges_scratch_bytes into test_redzone's record of covered size functions, which that file's last test reads."""
import numpy as np
import pytest

from conftest import pkg
from test_redzone import L, dev, run_case

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 1), (65, 130), (257, 63), (4097, 8195), (4095, 8193)]  # SCAN_TILE 4096, ME_THREADS 256


def mesh(V, F):
    """Random triples: long lists and non-manifold edges, a few indices outside [0, V) (dropped before any use), E ragged."""
    rng = np.random.default_rng(V * 7919 + F)
    verts = rng.standard_normal((V, 3)).astype(np.float32)
    faces = rng.integers(0, V, (F, 3)).astype(np.int32)
    faces[::11, 0], faces[5::13, 2] = -1, V
    return verts, faces


def sizes(V, F):
    return [("dgm_mesh_edges_scratch_bytes", L().dgm_mesh_edges_scratch_bytes(V, F))]


@pytest.mark.parametrize("V,F", SIZES)
def test_edge_table(V, F):
    T = pkg("mesh_topology")
    _, faces = mesh(V, F)

    def call(i):
        table = T.EdgeTable("mesh_edges", i["faces"], V)
        t = table.emit(edges=True, faces=True, adjacency=True, kind=True)
        assert table.E % 64 != 0 or (table.E == 0 and F == 1)  # ragged (the one face of F = 1 has an index of -1: no edge at all)
        return [t["edges"], t["edge_faces"], t["edge_count"], t["adj"], t["adj_kind"], table.adj_offset, table.vert_flag]

    run_case(call, {"faces": dev(faces)}, sizes(V, F))


@pytest.mark.parametrize("boundary", ["fixed", "curve", "free"])
@pytest.mark.parametrize("V,F", SIZES[2:])
def test_smooth(V, F, boundary):
    S = pkg("mesh_smooth")
    verts, faces = mesh(V, F)
    run_case(lambda i: [S.smooth_mesh(i["verts"], i["faces"], iterations=2, boundary=boundary)], {"verts": dev(verts), "faces": dev(faces)},
             sizes(V, F))
