"""numpy restatement of the edge table, the topology report and the smoothing step (dg-mesh_amd/mesh_topology.py, mesh_smooth.py,
csrc/mesh_edges.hip; the definitions are in include/dgmesh_hip.h), and the small meshes the tests run on.  No torch, nothing from
the reference project.  The edge table is np.unique over sorted pairs, edge_faces / edge_count a plain loop over the faces, adjacency
sorted lists; the smoothing step adds the neighbours one after the other in fp64 in ascending order (never np.sum, which adds
pairwise), divides once and rounds to fp32 once."""
import numpy as np

KIND_REGULAR, KIND_BOUNDARY, KIND_NONMANIFOLD, KIND_MISORIENTED = 0, 1, 2, 3
BOUNDARIES = ("fixed", "curve", "free")


# ---- topology ----------------------------------------------------------------------------------------------------------------------
def valid_faces(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    inside = ((f >= 0) & (f < V)).all(1)
    return inside & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def kind_of(c0, c1):
    s = c0 + c1
    return KIND_BOUNDARY if s == 1 else KIND_NONMANIFOLD if s >= 3 else KIND_REGULAR if (c0, c1) == (1, 1) else KIND_MISORIENTED


def edge_table(faces, V):
    """{"edges", "edge_faces", "edge_count": (E, 2) int32; "adj_offset" (V + 1,), "adj" (2E,) int32; "adj_kind" (2E,), "vert_flag" (V,)
    uint8; "kind" (E,); "info": the eight counts of dgm_mesh_edges_count as a dict}."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(faces, V)
    fv = faces[ok]
    half = np.concatenate([fv[:, [0, 1]], fv[:, [1, 2]], fv[:, [2, 0]]]) if len(fv) else np.zeros((0, 2), np.int64)
    edges = np.unique(np.sort(half, 1), axis=0).reshape(-1, 2) if len(half) else half
    E = len(edges)
    index = {(int(u), int(v)): i for i, (u, v) in enumerate(edges)}
    edge_faces = np.full((E, 2), -1, np.int64)
    edge_count = np.zeros((E, 2), np.int64)
    for f in np.nonzero(ok)[0]:  # ascending: the first face met per direction is the smallest
        a, b, c = (int(x) for x in faces[f])
        for p, q in ((a, b), (b, c), (c, a)):
            e, col = index[(min(p, q), max(p, q))], 0 if p < q else 1
            if edge_count[e, col] == 0:
                edge_faces[e, col] = f
            edge_count[e, col] += 1
    kind = np.array([kind_of(int(c0), int(c1)) for c0, c1 in edge_count], np.int64).reshape(-1)
    lists = [[] for _ in range(V)]
    for (u, v), k in zip(edges, kind):
        lists[u].append((int(v), int(k)))
        lists[v].append((int(u), int(k)))
    lists = [sorted(l) for l in lists]
    adj_offset = np.zeros(V + 1, np.int64)
    adj_offset[1:] = np.cumsum([len(l) for l in lists])
    adj = np.array([n for l in lists for n, _ in l], np.int64)
    adj_kind = np.array([k for l in lists for _, k in l], np.int64)
    used = np.zeros(V, bool)
    used[fv.reshape(-1)] = True
    vert_flag = used.astype(np.int64)
    for v, l in enumerate(lists):
        for _, k in l:
            vert_flag[v] |= 2 if k == KIND_BOUNDARY else 0 if k == KIND_REGULAR else 4
    info = {"edges": E, "boundary_edges": int((kind == KIND_BOUNDARY).sum()), "nonmanifold_edges": int((kind == KIND_NONMANIFOLD).sum()),
            "misoriented_edges": int((kind == KIND_MISORIENTED).sum()), "regular_edges": int((kind == KIND_REGULAR).sum()),
            "verts_used": int(used.sum()), "faces_valid": int(ok.sum()), "adjacency": 2 * E}
    return {"edges": edges.astype(np.int32), "edge_faces": edge_faces.astype(np.int32), "edge_count": edge_count.astype(np.int32),
            "adj_offset": adj_offset.astype(np.int32), "adj": adj.astype(np.int32), "adj_kind": adj_kind.astype(np.uint8),
            "vert_flag": vert_flag.astype(np.uint8), "kind": kind, "info": info}


def components(faces, V):
    """The connected components (through shared vertices of valid faces) that have a used vertex."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    fv = faces[valid_faces(faces, V)]
    parent = np.arange(V)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in fv:
        ra, rb, rc = find(a), find(b), find(c)
        r = min(ra, rb, rc)
        parent[ra] = parent[rb] = parent[rc] = r
    return len({find(int(v)) for v in np.unique(fv)})


def report(verts, faces):
    """mesh_topology.topology_report without "edge_length" (fp32 sums on the device are not restated bit for bit; the tests compare it
    against edge_lengths below with a tolerance)."""
    V = len(verts)
    t = edge_table(faces, V)
    i = t["info"]
    rep = {"verts": V, "faces": len(np.asarray(faces).reshape(-1, 3))}
    rep.update({k: i[k] for k in ("verts_used", "faces_valid", "edges", "boundary_edges", "nonmanifold_edges", "misoriented_edges")})
    rep["components"] = components(faces, V)
    rep["euler"] = rep["verts_used"] - rep["edges"] + rep["faces_valid"]
    rep["watertight"] = rep["boundary_edges"] == 0 and rep["nonmanifold_edges"] == 0 and rep["misoriented_edges"] == 0 and rep["faces_valid"] > 0
    rep["genus"] = None
    if rep["watertight"]:
        rep["genus"] = rep["components"] - rep["euler"] // 2 if rep["euler"] % 2 == 0 else rep["components"] - rep["euler"] / 2
    return rep


def edge_lengths(verts, edges):
    v = np.asarray(verts, np.float64)
    return np.linalg.norm(v[edges[:, 0]] - v[edges[:, 1]], axis=1)


# ---- smoothing ---------------------------------------------------------------------------------------------------------------------
def smooth_step(verts, table, factor, boundary):
    """One step (include/dgmesh_hip.h, SMOOTHING STEP): verts (V, 3) float32 -> (V, 3) float32."""
    verts = np.asarray(verts, np.float32)
    V = len(verts)
    off, adj, adj_kind, flag = table["adj_offset"].astype(np.int64), table["adj"].astype(np.int64), table["adj_kind"], table["vert_flag"]
    rim = (flag & 2) != 0
    x = verts.astype(np.float64)
    s = np.zeros((V, 3), np.float64)
    n = np.zeros(V, np.int64)
    taken = np.ones(len(adj), bool)
    if boundary == "curve":  # a rim vertex keeps the neighbours it is joined to by a boundary edge
        owner = np.repeat(np.arange(V), np.diff(off))
        taken = ~rim[owner] | (adj_kind == KIND_BOUNDARY)
    deg = np.diff(off)
    with np.errstate(all="ignore"):
        for j in range(int(deg.max()) if V else 0):  # the j-th neighbour of every vertex that has one: ascending order per vertex
            rows = np.nonzero(deg > j)[0]
            at = off[rows] + j
            rows, at = rows[taken[at]], at[taken[at]]
            s[rows] = s[rows] + x[adj[at]]
            n[rows] += 1
        move = np.isfinite(verts).all(1) & (n > 0)
        if boundary == "fixed":
            move &= ~rim
        m = s / np.maximum(n, 1).astype(np.float64)[:, None]
        out = (x + np.float64(factor) * (m - x)).astype(np.float32)
    out[~move] = verts[~move]
    return out


def smooth(verts, faces, iterations=10, lam=0.5, mu=-0.53, method="taubin", boundary="fixed"):
    v = np.asarray(verts, np.float32).copy()
    table = edge_table(faces, len(v))
    for f in ([lam, mu] * iterations if method == "taubin" else [lam] * iterations):
        v = smooth_step(v, table, f, boundary)
    return v


def enclosed_volume(verts, faces):
    p = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("fi,fi->f", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def tetrahedron():
    verts = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32)
    faces = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)  # consistently wound
    return verts, faces


def icosphere(subdivisions):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def noisy_icosphere(subdivisions=3, sigma=0.02, seed=0):
    verts, faces = icosphere(subdivisions)
    r = 1.0 + sigma * np.random.default_rng(seed).standard_normal(len(verts))
    return (verts.astype(np.float64) * r[:, None]).astype(np.float32), faces


def grid_patch(n, m, seed=None):
    """n x m vertices in the plane z = 0 (vertex i * m + j at (j, i, 0)), two triangles per cell; with a seed the interior is lifted
    out of the plane by noise and the rim moved inside the plane."""
    jj, ii = np.meshgrid(np.arange(m), np.arange(n))
    verts = np.stack([jj.ravel(), ii.ravel(), np.zeros(n * m)], 1).astype(np.float64)
    if seed is not None:
        rng = np.random.default_rng(seed)
        verts[:, :2] += 0.2 * rng.standard_normal((n * m, 2))
        inner = ((ii > 0) & (ii < n - 1) & (jj > 0) & (jj < m - 1)).ravel()
        verts[inner, 2] = 0.3 * rng.standard_normal(int(inner.sum()))
    faces = []
    for i in range(n - 1):
        for j in range(m - 1):
            a, b, c, d = i * m + j, i * m + j + 1, (i + 1) * m + j, (i + 1) * m + j + 1
            faces += [(a, b, d), (a, d, c)]
    return verts.astype(np.float32), np.asarray(faces, np.int32)


def grid_rim(n, m):
    jj, ii = np.meshgrid(np.arange(m), np.arange(n))
    return ((ii == 0) | (ii == n - 1) | (jj == 0) | (jj == m - 1)).ravel()


def torus(n=12, m=8, R=2.0, r=0.7):
    verts, faces = [], []
    for i in range(n):
        for j in range(m):
            u, w = 2 * np.pi * i / n, 2 * np.pi * j / m
            verts.append(((R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)))
            a, b, c, d = i * m + j, ((i + 1) % n) * m + j, i * m + (j + 1) % m, ((i + 1) % n) * m + (j + 1) % m
            faces += [(a, b, d), (a, d, c)]
    return np.asarray(verts, np.float32), np.asarray(faces, np.int32)


def bow_tie():
    """Two triangles that share one vertex: every edge is a boundary edge, one component."""
    verts = np.array([[0, 0, 0], [-1, 1, 0], [-1, -1, 0], [1, -1, 0], [1, 1, 0]], np.float32)
    return verts, np.array([[0, 1, 2], [0, 3, 4]], np.int32)


def fan():
    """Three faces on the edge (0, 1)."""
    verts = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0], [-1, 1, 0], [-1, -1, 0]], np.float32)
    return verts, np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]], np.int32)


def same_winding_pair():
    """Two faces that traverse their shared edge 0->1 in the same direction."""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0]], np.float32)
    return verts, np.array([[0, 1, 2], [0, 1, 3]], np.int32)


def wheel(spokes=600):
    """A hub (vertex 0) with `spokes` rim vertices and as many faces: the hub has more neighbours than a workgroup has threads."""
    a = 2 * np.pi * np.arange(spokes) / spokes
    verts = np.concatenate([[[0, 0, 0.5]], np.stack([np.cos(a), np.sin(a), np.zeros(spokes)], 1)]).astype(np.float32)
    k = np.arange(spokes)
    return verts, np.stack([np.zeros(spokes, np.int64), 1 + k, 1 + (k + 1) % spokes], 1).astype(np.int32)


def salted(seed=3):
    """The noisy icosphere of subdivision 1 with unused vertices appended, one of them NaN, invalid faces mixed in (index -1, index
    V, a repeated corner; two of them on vertices nothing else uses) and one used vertex made NaN.  -> verts, faces, a dict of the
    vertex sets the tests name."""
    verts, faces = noisy_icosphere(1, 0.05, seed)
    n0 = len(verts)
    extra = np.array([[5, 5, 5], [np.nan, 1, 2], [7, 7, 7], [8, 8, 8], [9, 9, 9]], np.float32)  # n0 .. n0 + 4
    verts = np.concatenate([verts, extra])
    V = len(verts)
    bad = np.array([[-1, 0, 1], [0, 1, V], [2, 2, 3], [n0 + 2, n0 + 3, n0 + 3], [n0 + 2, n0 + 4, V + 7], [4, 4, 4]], np.int32)
    faces = np.concatenate([faces[:10], bad[:3], faces[10:], bad[3:]]).astype(np.int32)
    nan_vertex = 7
    verts[nan_vertex, 1] = np.nan
    return verts, faces, {"unused": np.arange(n0, V), "nan": nan_vertex}


def random_soup(V=500, F=3000, seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((V, 3)).astype(np.float32), rng.integers(0, V, (F, 3)).astype(np.int32)
