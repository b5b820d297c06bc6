"""The MLP backward pass's launch plan (csrc/mlp.hip: p4_plan, bwd_plan, group_split) restated in plain Python.

It exists to CHOOSE batch sizes and to LABEL test cases (tests/test_mlp_plan_boundaries.py), never to compute anything a test
compares: which N sits on which side of every line where the host code cuts a batch differently.  Two checks keep it honest: the
partial-tile blocks dgm_mlp_describe_workspace reports are `chunks` tiles long (host), and the stage timer sees paired launches
exactly where `n_dw > 0` (device).

The plan's classes, nt = ceil(N / 32) tiles on `cus` compute units (DESIGN 4.1b has the table for 256):
  A  nt < cus            one tile per chunk, chunks = gx = nt
  B  nt = cus            one tile per chunk, chunks = CUs exactly
  C  cus < nt < 4 gx     unpaired, 2 .. 4 tiles per chunk, ragged last chunk (everything above cus where nothing pairs: < 64 CUs)
  D  nt = 4 gx           the first paired and grouped size, every weight-gradient workgroup of a paired launch full
  E  nt > 4 gx           paired, the last weight-gradient workgroups short of tiles or without any
"""
import collections

TILE = 32             # rows of a plane-format tile
PAIR_MIN_GX = 64      # bwd_plan: no paired launch on fewer workgroups
PAIR_MIN_TILES = 4    # ... or on fewer than this many tiles per workgroup
PAIR_SHARE = (128, 256)  # P4_PAIR_SHARE_NUM / P4_PAIR_SHARE_DEN: the weight gradient's share of a paired launch's workgroups

Plan = collections.namedtuple("Plan", "nt gx tiles_per_chunk chunks n_dw tpc_pair chunks_pair chunked n_wg")


def _ceil_div(a, b):
    return (a + b - 1) // b


def plan(N, cus=256):
    nt = _ceil_div(N, TILE)
    tiles_per_chunk = max(_ceil_div(nt, cus), 1)
    chunks = _ceil_div(nt, tiles_per_chunk)
    gx = min(nt, cus)
    n_dw = 0
    if gx >= PAIR_MIN_GX and nt >= PAIR_MIN_TILES * gx:
        n_dw = min(gx * PAIR_SHARE[0] // PAIR_SHARE[1], gx - 1, chunks)
    tpc_pair = _ceil_div(nt, n_dw) if n_dw > 0 else 0
    chunks_pair = _ceil_div(nt, tpc_pair) if n_dw > 0 else 0
    pair_grid = n_dw + max(gx - n_dw, 1)
    chunked = int(pair_grid - n_dw == n_dw and n_dw % 8 == 0)
    n_wg = (n_dw // 2) & ~7
    if n_wg < 8 or 4 * n_wg > gx:
        n_wg = 0
    return Plan(nt, gx, tiles_per_chunk, chunks, n_dw, tpc_pair, chunks_pair, chunked, n_wg)


def plan_class(N, cus=256):
    p = plan(N, cus)
    if p.n_dw > 0:
        return "D" if p.nt == PAIR_MIN_TILES * p.gx else "E"
    return "A" if p.nt < cus else ("B" if p.nt == cus else "C")


def classes(cus):
    """The classes that exist at this CU count."""
    return "ABCDE" if cus >= PAIR_MIN_GX else "ABC"


def _key(nt, cus):
    """What a boundary is a change of: the class, the tiles per chunk, and whether there are enough workgroups to pair at all."""
    N = nt * TILE
    p = plan(N, cus)
    return plan_class(N, cus), p.tiles_per_chunk, p.gx >= PAIR_MIN_GX


def boundaries(cus):
    """Tile counts nt such that the plan of nt + 1 tiles differs in kind from the plan of nt tiles, up to the first size of class E
    (the last class: beyond it only tiles_per_chunk grows, every `cus` tiles, as it does inside class C), or up to four tiles per
    chunk where nothing pairs.  nt = 1 is one: the first size with a second workgroup."""
    last = PAIR_MIN_TILES * cus
    return [1] + [nt for nt in range(2, last + 1) if _key(nt, cus) != _key(nt + 1, cus)]


def sweep(cus=256):
    """Per boundary the largest N before it (a multiple of 32: a full last tile) and the smallest N after it (a one-row last tile);
    per class that is a single tile count (B, D) therefore both of its ends; and the two ends of the ragged single tile, 1 and 31."""
    sizes = {1, TILE - 1}
    for nt in boundaries(cus):
        sizes |= {nt * TILE, nt * TILE + 1}
    return sorted(sizes)


def label(N, cus=256):
    p = plan(N, cus)
    s = f"{plan_class(N, cus)}: {p.nt} tiles, {p.chunks} chunks of {p.tiles_per_chunk}"
    if p.n_dw > 0:
        s += f"; paired: {p.chunks_pair} of {p.n_dw} chunks of {p.tpc_pair}, n_wg {p.n_wg}, chunked {p.chunked}"
    return s
