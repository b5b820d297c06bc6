"""The tiled u32 scan of csrc/mesh_scan.hpp with more tiles than one round of its tile-offset phase takes: launch_scan_blocks walks
the tile totals 1024 at a time, a tile is 4096 integers, so 4096 * 1024 + 1 elements put one tile into its second round.  Both users
below are all integers; the expected values are written in closed form in numpy."""
import numpy as np
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROUND = 4096 * 1024  # elements behind which the tile offsets carry over from one round of launch_scan_blocks to the next


def _classify_closed_form(face_of, F):
    """include/dgmesh_hip.h, dgm_anchor_classify."""
    fo = np.asarray(face_of, np.int64)
    valid = (fo >= 0) & (fo < F)
    counts = np.bincount(fo[valid], minlength=F)
    offsets = np.cumsum(counts) - counts
    lists = np.concatenate([np.flatnonzero(counts == 1), np.flatnonzero(counts > 1), np.flatnonzero(counts == 0)])
    order = np.flatnonzero(valid)
    order = order[np.argsort(fo[order], kind="stable")]  # ascending face, ascending index within a face
    members = np.full(fo.size, -1, np.int64)
    members[:order.size] = order
    rank = np.full(fo.size, -1, np.int64)
    rank[order] = np.arange(order.size) - offsets[fo[order]]
    totals = (int((counts == 1).sum()), int((counts > 1).sum()), int((counts == 0).sum()), int(valid.sum()))
    return {"counts": counts, "offsets": offsets, "lists": lists, "members": members, "rank": rank, "totals": totals}


@pytest.mark.parametrize("F", [ROUND + 1, ROUND + 2])
def test_classify_past_one_round_of_tile_offsets(F):
    """dgm_anchor_classify (the three-component scan) with face_of = [0, 0, F - 1, 4096 * 1024, -1].
    With F = 4096 * 1024 + 1 the faces F - 1 and 4096 * 1024 are the same face: it has two Gaussians, like face 0, and the totals are
    (0, 2, F - 2, 4).  With F = 4096 * 1024 + 2 they are two faces and the counts are 2 at face 0 and 1 at each of them, the totals
    (2, 1, F - 3, 4) and the lists [4096 * 1024, F - 1, 0, then every other face ascending]; these are asserted literally."""
    face_of = [0, 0, F - 1, ROUND, -1]
    want = _classify_closed_form(face_of, F)
    got = pkg("anchor").classify(torch.tensor(face_of, dtype=torch.int32, device=DEV), F)
    print("F", F, "totals", got["totals"], "expected", want["totals"])
    assert got["totals"] == want["totals"]
    for k in ("counts", "offsets", "lists", "members", "rank"):
        assert np.array_equal(got[k].cpu().numpy().astype(np.int64), want[k]), k
    if F == ROUND + 2:
        assert got["totals"] == (2, 1, F - 3, 4)
        counts = got["counts"].cpu().numpy()
        assert counts[0] == 2 and counts[ROUND] == 1 and counts[F - 1] == 1 and int(counts.sum(dtype=np.int64)) == 4
        lists = got["lists"].cpu().numpy()
        assert lists[:3].tolist() == [ROUND, F - 1, 0] and np.array_equal(lists[3:], np.arange(1, ROUND))
        assert got["members"].tolist() == [0, 1, 3, 2, -1] and got["rank"].tolist() == [0, 1, 0, 0, -1]


def test_mesh_edges_past_one_round_of_tile_offsets():
    """mesh_edges (three one-component scans over the vertices) with V = 4096 * 1024 + 1 and the faces (0, 1, 2), (V - 3, V - 2, V - 1):
    six boundary edges, two neighbours at six vertices and none elsewhere."""
    V = ROUND + 1
    a, b, c = V - 3, V - 2, V - 1
    faces = torch.tensor([[0, 1, 2], [a, b, c]], dtype=torch.int32, device=DEV)
    table = pkg("mesh_topology").EdgeTable("mesh_edges", faces, V)
    t = table.emit(edges=True, faces=True, adjacency=True, kind=True)
    print("info", table.info)
    assert table.info == {"edges": 6, "boundary_edges": 6, "nonmanifold_edges": 0, "misoriented_edges": 0, "regular_edges": 0,
                          "verts_used": 6, "faces_valid": 2, "adjacency": 12}
    assert t["edges"].tolist() == [[0, 1], [0, 2], [1, 2], [a, b], [a, c], [b, c]]
    assert t["edge_count"].tolist() == [[1, 0], [0, 1], [1, 0]] * 2
    assert t["edge_faces"].tolist() == [[0, -1], [-1, 0], [0, -1], [1, -1], [-1, 1], [1, -1]]
    used = np.array([0, 1, 2, a, b, c])
    degree = np.zeros(V, np.int64)
    degree[used] = 2
    adj_offset = np.zeros(V + 1, np.int64)
    adj_offset[1:] = np.cumsum(degree)
    assert np.array_equal(table.adj_offset.cpu().numpy().astype(np.int64), adj_offset)
    assert t["adj"].tolist() == [1, 2, 0, 2, 0, 1, b, c, a, c, a, b]
    assert t["adj_kind"].tolist() == [1] * 12  # every edge is a boundary edge
    vert_flag = np.zeros(V, np.uint8)
    vert_flag[used] = 3  # used, and on a boundary edge
    assert np.array_equal(table.vert_flag.cpu().numpy(), vert_flag)
