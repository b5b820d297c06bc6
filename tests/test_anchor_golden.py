"""Ties the float64 restatement of Gaussian-mesh anchoring (tests/_anchor_ref.py) to the REFERENCE's own anchor_mesh,
average_and_prune, densify_from_face and optimizer surgery, executed from their source text by
tests/golden/make_anchor_golden.py into tests/golden/anchor_small.npz, fed the reference's recorded draws.  Integer outcomes
(which rows survive, in which order, how many are appended) must match exactly; the Adam moments are gathered or zero and must
match exactly; values within 16 fp32 ulps of max(1, |value|) (the reference's fp32 arithmetic against float64).  CPU only."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from _anchor_ref import NAMES, PolyField, anchor_ref

GOLD = os.path.join(ROOT, "tests", "golden", "anchor_small.npz")
EPS32 = 2.0 ** -24


@pytest.mark.parametrize("tag", ["c0", "c1"])
def test_restatement_matches_the_reference_golden(tag):
    d = np.load(GOLD)
    scale, radius, t, topn, bs, increase_bs, _ = d[f"{tag}/args"].tolist()
    topn, bs, increase_bs = int(topn), int(bs), int(increase_bs)
    state = {}
    for k in NAMES:
        state[k] = torch.tensor(d[f"{tag}/in/p/{k}"])
        state[k + "/m"] = torch.tensor(d[f"{tag}/in/m/{k}"])
        state[k + "/v"] = torch.tensor(d[f"{tag}/in/v/{k}"])
    fld = lambda name: PolyField(*[torch.tensor(d[f"{tag}/{name}/{i}"]) for i in range(4)])
    draws = {"perm_n1": torch.tensor(d[f"{tag}/perm_n1"])[:bs], "perm_0_1": torch.tensor(d[f"{tag}/perm_0_1"])[:increase_bs],
             "angle": torch.tensor(d[f"{tag}/angle"])}
    max_d2 = float(torch.tensor([scale], dtype=torch.float32) * radius)   # (the reference's fp32 bound on squared distances)
    out, info = anchor_ref(state, torch.tensor(d[f"{tag}/verts"]), torch.tensor(d[f"{tag}/faces"]), fld("deform"), fld("back"),
                           torch.tensor([t]), max_d2, topn, bs, increase_bs, draws)
    # the case covers every class, invalid Gaussians, n-1 faces with >= 3 members and degenerate faces
    fo = info["face_of"]
    cnt = torch.bincount(fo[fo >= 0], minlength=d[f"{tag}/faces"].shape[0])
    print(tag, "n11", info["n11"], "nn1", info["nn1"], "n01", info["n01"], "invalid", int((fo < 0).sum()),
          "selected n-1 faces with >= 3 members", int((cnt[info["sel_n1"]] >= 3).sum()))
    assert info["n11"] > 0 and info["nn1"] > 0 and info["n01"] > 0 and int((fo < 0).sum()) > 0
    assert int((cnt[info["sel_n1"]] >= 3).sum()) > 0
    worst = 0.0
    for k in NAMES:
        ref = torch.tensor(d[f"{tag}/out/p/{k}"]).double()
        assert out[k].shape == ref.shape, (k, out[k].shape, ref.shape)
        err = float((out[k] - ref).abs().max())
        bound = 16 * EPS32 * max(1.0, float(ref.abs().max()))
        worst = max(worst, err / bound)
        print(f"{tag} {k}: rows {ref.shape[0]} max err {err:.2e} (bound {bound:.2e})")
        assert err <= bound, k
        for mk in ("m", "v"):
            assert torch.equal(out[f"{k}/{mk}"], torch.tensor(d[f"{tag}/out/{mk}/{k}"]).double()), (k, mk)
    P = out["xyz"].shape[0]
    assert d[f"{tag}/out/accum"].shape == (P, 1) and not d[f"{tag}/out/accum"].any() and not d[f"{tag}/out/max_radii"].any()
    loss = float(info["loss_1_1"] + info["loss_n_1"])
    gl = float(d[f"{tag}/loss"])
    print(f"{tag} loss {loss:.9g} reference {gl:.9g}")
    assert abs(loss - gl) <= 16 * EPS32 * abs(gl)
