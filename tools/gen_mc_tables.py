"""Generate the marching-cubes case table dg-mesh_amd/csrc/mc_tables.hpp.

    python tools/gen_mc_tables.py            # rewrite the header
    python tools/gen_mc_tables.py --check    # exit 1 if the committed header differs from what this script writes

The table is derived, not typed in:
  * corner c of a cell sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) (x = grid dim 0); case = sum of (inside(c) << c), a corner
    being inside iff f < iso;
  * edge e = 4 * axis + m runs along `axis` from corner a (axis bit 0) to corner b (axis bit 1); m holds the coordinates of the two
    other axes in increasing axis order (bit 0 the lower axis).  The cell's edge e is owned by grid point cell + offset(a);
  * on each of the 6 cube faces, walked counter-clockwise as seen from outside the cube, every crossing where the walk enters the
    inside (an "entry") is joined to the next crossing where it leaves (an "exit"): each inside corner of an ambiguous face is cut off
    on its own ("inside corners are kept separate").  The rule reads only the face's 4 signs, so the two cells sharing a face cut it
    identically and the mesh is closed;
  * the face segments chain into closed polygons (each crossed edge ends one segment and starts another); every polygon is fanned
    from the first vertex whose diagonals all run through the cell's interior (no diagonal joins two vertices of one cube face, where
    the neighbouring cell could draw the same pair), and every triangle is wound so that (v1 - v0) x (v2 - v0) points from the
    inside (f < iso) to the outside.
The script checks both properties on every case and reports the largest triangle count, which sizes the kernel's per-cell work.
"""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "dg-mesh_amd", "csrc", "mc_tables.hpp")


def corner_pos(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def _others(axis):
    return [d for d in range(3) if d != axis]


def edges():
    """[(a, b)] for e = 0..11."""
    out = []
    for axis in range(3):
        o1, o2 = _others(axis)
        for m in range(4):
            p = [0, 0, 0]
            p[o1], p[o2] = m & 1, m >> 1
            a = p[0] | (p[1] << 1) | (p[2] << 2)
            out.append((a, a | (1 << axis)))
    return out


EDGES = edges()
EDGE_OF = {frozenset(ab): e for e, ab in enumerate(EDGES)}


def _sub(p, q):
    return [p[i] - q[i] for i in range(3)]


def _cross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def _dot(u, v):
    return sum(u[i] * v[i] for i in range(3))


def faces():
    """The 6 cube faces as corner cycles, counter-clockwise seen from outside the cube."""
    out = []
    for axis in range(3):
        u, v = _others(axis)
        for side in range(2):
            cyc = []
            for cu, cv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = [0, 0, 0]
                p[axis], p[u], p[v] = side, cu, cv
                cyc.append(p[0] | (p[1] << 1) | (p[2] << 2))
            P = [corner_pos(c) for c in cyc]
            n = _cross(_sub(P[1], P[0]), _sub(P[2], P[1]))
            outward = [0, 0, 0]
            outward[axis] = 2 * side - 1
            if _dot(n, outward) < 0:
                cyc.reverse()
            out.append(cyc)
    return out


FACES = faces()


def edge_faces(e):
    """Indices (into FACES) of the two cube faces edge e lies on."""
    a, b = EDGES[e]
    return [f for f, cyc in enumerate(FACES) if a in cyc and b in cyc]


def polygons(case):
    inside = [(case >> c) & 1 for c in range(8)]
    nxt = {}
    for cyc in FACES:
        cross = []  # (position along the walk, kind, edge)
        for k in range(4):
            a, b = cyc[k], cyc[(k + 1) % 4]
            if inside[a] != inside[b]:
                cross.append((k, "X" if inside[a] else "E", EDGE_OF[frozenset((a, b))]))
        for i, (_, kind, e) in enumerate(cross):
            if kind != "E":
                continue
            for j in range(1, len(cross)):  # the next exit along the walk
                _, kind2, e2 = cross[(i + j) % len(cross)]
                if kind2 == "X":
                    assert e2 not in nxt
                    nxt[e2] = e  # directed segment exit -> entry
                    break
    heads = sorted(nxt.values())
    assert heads == sorted(nxt), f"case {case}: open chain"
    polys, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        poly, e = [], start
        while e not in seen:
            seen.add(e)
            poly.append(e)
            e = nxt[e]
        assert e == start
        polys.append(poly)
    return polys


def fan(poly):
    """Triangles of a polygon fanned from the first vertex whose diagonals all cross the cell's interior."""
    n = len(poly)
    for r in range(n):
        p = poly[r:] + poly[:r]
        if all(not set(edge_faces(p[0])) & set(edge_faces(p[i])) for i in range(2, n - 1)):
            return [(p[0], p[i], p[i + 1]) for i in range(1, n - 1)]
    raise AssertionError(f"polygon {poly}: no fan vertex with interior diagonals")


def _mid(e):
    a, b = EDGES[e]
    return [(corner_pos(a)[i] + corner_pos(b)[i]) / 2 for i in range(3)]


def _normal(tri):
    p0, p1, p2 = (_mid(e) for e in tri)
    return _cross(_sub(p1, p0), _sub(p2, p0))


def raw_table():
    return [[t for poly in polygons(case) for t in fan(poly)] for case in range(256)]


def table():
    """Triangles (edge triples) of every case, wound inside -> outside."""
    tab = raw_table()
    # The walk puts the inside on the left of every segment seen from outside the cube, so one winding holds for every case;
    # which one is read off the single-corner cases: the normal must point away from the inside corner.
    signs = set()
    for c in range(8):
        (tri,) = tab[1 << c]
        away = _sub([0.5, 0.5, 0.5], corner_pos(c))
        signs.add(_dot(_normal(tri), away) > 0)
    assert len(signs) == 1, "inconsistent winding"
    if not signs.pop():
        tab = [[(t[0], t[2], t[1]) for t in tris] for tris in tab]
    for case, tris in enumerate(tab):  # every triangle of the single-polygon cases points from the inside corners outwards
        inside = [c for c in range(8) if (case >> c) & 1]
        if len(polygons(case)) == 1 and 0 < len(inside) < 8:
            ci = [sum(corner_pos(c)[i] for c in inside) / len(inside) for i in range(3)]
            co = [sum(corner_pos(c)[i] for c in range(8) if c not in inside) / (8 - len(inside)) for i in range(3)]
            assert sum(_dot(_normal(t), _sub(co, ci)) for t in tris) > 0, f"case {case}: winding"
    return tab


def render(tab):
    max_tris = max(len(t) for t in tab)
    L = []
    L.append("// Marching-cubes case table -- GENERATED by tools/gen_mc_tables.py; do not edit (the tests regenerate and compare it).")
    L.append("//")
    L.append("// Corner c of cell (i, j, k) is grid point (i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1)); x = grid dim 0.")
    L.append("// case = sum over corners of (inside(c) << c), inside iff f < iso (NaN: outside).")
    L.append("// Edge e = 4 * axis + m runs along `axis` from corner a (axis bit clear) to corner b = a | (1 << axis); m holds the")
    L.append("// coordinates of the two other axes, the lower axis in bit 0.  The cell's edge e is the `axis` edge owned by grid point")
    L.append("// cell + offset(a).  dgm_mc_edge_corner_a[e] gives a.")
    L.append("// Ambiguous faces keep inside corners separate; every triangle (e0, e1, e2) is wound so that (v1 - v0) x (v2 - v0) points")
    L.append("// from f < iso towards f >= iso.")
    L.append(f"// Largest triangle count of a case: {max_tris}.")
    L.append("#ifndef DGM_MC_TABLES_HPP")
    L.append("#define DGM_MC_TABLES_HPP")
    L.append("")
    L.append("#include <stdint.h>")
    L.append("")
    L.append(f"#define DGM_MC_MAX_TRIS {max_tris}")
    L.append("")
    L.append("#ifdef __HIPCC__")
    L.append("#define DGM_MC_TABLE __constant__")
    L.append("#else")
    L.append("#define DGM_MC_TABLE")
    L.append("#endif")
    L.append("")
    L.append("DGM_MC_TABLE const uint8_t dgm_mc_edge_corner_a[12] = {" + ", ".join(str(a) for a, _ in EDGES) + "};")
    L.append("")
    L.append("DGM_MC_TABLE const uint8_t dgm_mc_tri_count[256] = {")
    for r in range(0, 256, 32):
        L.append("    " + ", ".join(str(len(tab[c])) for c in range(r, r + 32)) + ",")
    L.append("};")
    L.append("")
    L.append(f"DGM_MC_TABLE const int8_t dgm_mc_tri_table[256][{3 * max_tris}] = {{")
    for c in range(256):
        flat = [e for t in tab[c] for e in t]
        flat += [-1] * (3 * max_tris - len(flat))
        L.append("    {" + ", ".join(str(e) for e in flat) + "},")
    L.append("};")
    L.append("")
    L.append("#endif  // DGM_MC_TABLES_HPP")
    return "\n".join(L) + "\n"


def main(argv):
    tab = table()
    text = render(tab)
    print(f"largest triangle count per case: {max(len(t) for t in tab)}; triangles over all cases: {sum(map(len, tab))}")
    if "--check" in argv:
        with open(OUT) as fh:
            same = fh.read() == text
        print("mc_tables.hpp is " + ("up to date" if same else "STALE"))
        return 0 if same else 1
    with open(OUT, "w") as fh:
        fh.write(text)
    print(f"wrote {os.path.relpath(OUT, ROOT)}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
