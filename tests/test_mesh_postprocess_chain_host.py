"""CPU test of tests/_chain_fixture.py: the cases of tests/test_mesh_postprocess_chain.py are what they claim.  The numpy references
of every stage run in the production order on chain_field; the conditions below are what makes the intermediate meshes worth a test
(edges that three or more faces share, misoriented edges, rims that touch, more than one scan tile of faces).  They are conditions, not
measurements: if another numpy changes the noise and one fails, another seed is chosen, the condition stays."""
import numpy as np

import _chain_fixture as C


def test_field_is_the_stated_one():
    n = C.N
    field = C.chain_field(n, C.SEED)
    assert field.shape == (n, n, n) and field.dtype == np.float32
    assert np.array_equal(field, C.chain_field(n, C.SEED)) and not np.array_equal(field, C.chain_field(n, C.SEED + 1))
    quiet = field - (0.25 * np.random.default_rng(C.SEED).standard_normal((n, n, n))).astype(np.float32)
    c = (n - 1) / 2.0
    at = lambda x, y, z: float(quiet[int(round(x)), int(round(y)), int(round(z))])
    assert at(c - 0.22 * n, c, c) < -0.15 * n and at(c + 0.2 * n, c, c) < -0.15 * n  # inside the two blobs
    assert at(c, c + 0.33 * n, c) < 0 and at(c, c, n - 1) < -0.2 * n and at(0, 0, 0) > 0  # the floater, the cut sphere, a far corner
    assert at(c, c, c - 0.3 * n) < 0 < at(c, c, c - 0.3 * n - 2)  # the sheet is thinner than two voxels
    v = C.to_unit_box(np.array([[0, 0, 0], [n - 1, n - 1, n - 1], [c, c, c]], np.float32), n)
    assert v.dtype == np.float32 and np.array_equal(v, np.float32([[-(n - 1) / n] * 3, [(n - 1) / n] * 3, [0, 0, 0]]))


def test_cases_are_what_they_claim():
    chains = {case: C.reference_chain(case) for case in C.CASES}
    for case, chain in chains.items():
        assert tuple(st["name"] for st in chain) == C.STAGES
        print(case)
        for st in chain:
            print("  " + C.describe(st))
    assert any("target_faces" in kw for kw in C.CASES.values()) and {"grid10", "grid16"} <= set(C.CASES)
    mc = chains["grid10"][0]
    assert len(mc["faces"]) > 4096  # more than one scan tile
    assert mc["edges"]["nonmanifold_edges"] == 0 and mc["edges"]["boundary_edges"] > 0
    for case, (_, clean, smooth, simplify, repair) in chains.items():
        assert 0 < len(clean["faces"]) < len(mc["faces"]) and clean["repair"]["components"] < mc["repair"]["components"], case  # floaters went
        assert np.array_equal(smooth["faces"], clean["faces"]) and (smooth["verts"] != clean["verts"]).any(), case
        assert 0 < len(simplify["faces"]) < 2000 and simplify["edges"]["nonmanifold_edges"] > 0, case
        rep = simplify["repair"]  # what repair reports on the clustered mesh
        assert rep["components"] > 1 and rep["holes_filled"] >= 1 and rep["edges_on_open_chains"] > 0, case
        assert repair["edges"]["misoriented_edges"] == 0, case
        assert len(repair["verts"]) == len(simplify["verts"]) + rep["verts_added"] and rep["verts_added"] >= 1, case  # an added rim vertex
        assert len(repair["faces"]) == len(simplify["faces"]) + rep["faces_added"], case
        assert repair["edges"]["nonmanifold_edges"] > 0 and repair["edges"]["boundary_edges"] == rep["edges_on_open_chains"], case
    assert any(ch[3]["edges"]["misoriented_edges"] > 0 for ch in chains.values())
    assert any(ch[3]["repair"]["faces_flipped"] > 0 for ch in chains.values())
    tried = chains["target1200"][3]["grids_tried"]
    assert len(tried) > 1 and len(chains["target1200"][3]["faces"]) <= C.CASES["target1200"]["target_faces"]  # the bisection ran
