"""GPU tests of the edge table and the topology report (dg-mesh_amd/mesh_topology.py, csrc/mesh_edges.hip) against the numpy reference
tests/_edges_ref.py.  edges, edge_faces, edge_count, adj_offset, adj, adj_kind, vert_flag and every count are compared byte for byte
(everything is integers); every case runs twice and the two runs are compared byte for byte.  Only the report's edge lengths are
floats: fp32 torch reductions, compared with the fp64 lengths within (4 + ceil(log2 E)) fp32 ulp of the longest edge: a length
takes roundings in the differences, the squares, their two sums and the root, under 4 ulp together, and the mean's sum one more per
level of a pairwise tree over E numbers.  That bound holds torch's reductions, not a kernel of this project."""
import numpy as np
import pytest
import torch

import _edges_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu


def T():
    return pkg("mesh_topology")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
    assert a.tobytes() == b.tobytes(), f"{what}: {int((a.view(np.uint8) != b.view(np.uint8)).sum())} bytes differ"


def device_table(faces, V):
    table = T().EdgeTable("mesh_edges", dev(faces), V)
    out = {k: host(v) for k, v in table.emit(edges=True, faces=True, adjacency=True, kind=True).items()}
    out.update(adj_offset=host(table.adj_offset), vert_flag=host(table.vert_flag), info=table.info)
    return out


def check(verts, faces):
    """The device's tables and report against the reference, twice; -> the reference's table and report."""
    verts, faces = np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    V = len(verts)
    ref, ref_report = R.edge_table(faces, V), R.report(verts, faces)
    first = None
    for run in range(2):
        got = device_table(faces, V)
        assert got["info"] == ref["info"], f"counts (run {run}): {got['info']} against {ref['info']}"
        for k in ("edges", "edge_faces", "edge_count", "adj_offset", "adj", "adj_kind", "vert_flag"):
            same(got[k], ref[k], f"{k} (run {run})")
        rep = T().topology_report(dev(verts), dev(faces))
        lengths = rep.pop("edge_length")
        assert rep == ref_report, f"report (run {run}): {rep} against {ref_report}"
        if ref["info"]["edges"] and np.isfinite(verts[np.unique(ref["edges"])]).all():
            ln = R.edge_lengths(verts, ref["edges"])
            tol = (4.0 + np.ceil(np.log2(len(ln)))) * float(np.spacing(np.float32(ln.max())))
            for k, want in (("min", ln.min()), ("mean", ln.mean()), ("max", ln.max())):
                print(f"edge length {k}: device {lengths[k]!r}, fp64 {float(want)!r}, bound {tol:.3e}")
                assert abs(lengths[k] - float(want)) <= tol, k
        elif not ref["info"]["edges"]:
            assert lengths == {"min": None, "mean": None, "max": None}
        if first is None:
            first = got
        else:
            for k in got:
                if k != "info":
                    same(got[k], first[k], f"{k}: run 1 against run 0")
    # the public functions hand out the same tables
    e, ef, ec, (off, adj) = T().mesh_edges(dev(faces), V, return_faces=True, return_adjacency=True)
    for k, t in (("edges", e), ("edge_faces", ef), ("edge_count", ec), ("adj_offset", off), ("adj", adj)):
        same(host(t), ref[k], f"mesh_edges: {k}")
    same(host(T().mesh_edges(dev(faces), V)), ref["edges"], "mesh_edges alone")
    same(host(T().vertex_flags(dev(faces), V)), ref["vert_flag"], "vertex_flags")
    return ref, ref_report


BUILDERS = {"tetrahedron": R.tetrahedron, "icosphere": lambda: R.icosphere(3), "grid_patch": lambda: R.grid_patch(7, 11),
            "torus": R.torus, "bow_tie": R.bow_tie, "fan": R.fan, "same_winding_pair": R.same_winding_pair,
            "salted": lambda: R.salted()[:2], "random_soup": R.random_soup}


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_tables_equal_the_reference(name):
    verts, faces = BUILDERS[name]()
    ref, rep = check(verts, faces)
    print(f"{name}: V {len(verts)} F {len(faces)} E {ref['info']['edges']} longest list {int(np.diff(ref['adj_offset']).max())} report {rep}")


def test_wheel_hub_has_more_neighbours_than_a_workgroup_has_threads():
    verts, faces = R.wheel(600)
    ref, rep = check(verts, faces)
    assert np.diff(ref["adj_offset"])[0] == 600 and rep["boundary_edges"] == 600
    rng = np.random.default_rng(5)
    check(verts, faces[rng.permutation(len(faces))])  # the faces in another order: another arrival order at the hub's list


def test_marching_cubes_sphere_is_watertight():
    n = 24
    i = torch.arange(n, dtype=torch.float32, device="cuda")
    x, y, z = torch.meshgrid(i, i, i, indexing="ij")
    c = (n - 1) / 2.0
    field = torch.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - 0.37 * n
    verts, faces = pkg("marching_cubes").marching_cubes(field.contiguous())
    ref, rep = check(host(verts), host(faces))
    print(f"marching cubes at {n}^3: {rep}")
    assert rep["watertight"] and rep["genus"] == 0 and rep["components"] == 1 and rep["verts_used"] == len(verts)


@pytest.mark.parametrize("case", ["no_vertices", "no_faces", "all_faces_invalid", "faces_without_vertices"])
def test_empty_meshes(case):
    verts, faces = {"no_vertices": (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)),
                    "no_faces": (np.ones((5, 3), np.float32), np.zeros((0, 3), np.int32)),
                    "all_faces_invalid": (np.ones((5, 3), np.float32), np.array([[0, 0, 1], [-1, 2, 3], [1, 2, 5], [4, 4, 4]], np.int32)),
                    "faces_without_vertices": (np.zeros((0, 3), np.float32), np.array([[0, 1, 2]], np.int32))}[case]
    ref, rep = check(verts, faces)
    assert ref["info"]["edges"] == 0 and ref["edges"].shape == (0, 2) and not rep["watertight"] and rep["components"] == 0
    assert (ref["vert_flag"] == 0).all() and (ref["adj_offset"] == 0).all()


def test_argument_errors():
    f = torch.zeros((2, 3), dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="int32"):
        T().mesh_edges(f.long(), 4)
    with pytest.raises(ValueError, match=r"\(F, 3\)"):
        T().mesh_edges(f.reshape(3, 2), 4)
    with pytest.raises(ValueError, match="num_verts"):
        T().mesh_edges(f, -1)
    with pytest.raises(RuntimeError, match="float32"):
        T().topology_report(torch.zeros((4, 3), dtype=torch.float64, device="cuda"), f)
