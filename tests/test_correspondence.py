"""dg-mesh_amd/correspondence.py on the GPU: transport / correspond against a closed-form rigid motion (stub networks: any object with
.step works), then the two drivers end to end on the small mesh-phase scene of tests/test_visualize.py.

Bounds (eps = 2^-24, S = the largest |coordinate| in play):
  * transport against the closed form in float64: 16 eps S.  to_canonical and advect are each x + (y - x) around a rotation and a
    translation: a difference or sum with the translation, two products and their sum, y - x and x + (y - x) -- seven roundings of at
    most eps S -- plus cos / sin of the fp32 time within an ulp or two: eight per map, two maps (measured on the CPU: 3.4 eps S);
  * a vertex carried from t_a to t_b against the same vertex advected to t_b directly (another eight roundings): distance <= 24 eps S;
  * the kernel against float64 on a different tessellation: the K_MIN / K_CHOSEN bounds of tests/test_surface_host.py in units of
    E(d) (measured on the CPU on this input: 2.1 and 0.12).
Every test prints its figures before it asserts."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import _surface_ref as SR
from conftest import ROOT, pkg

DEV = "cuda"
EPS = 2.0 ** -24
SHIFT = (0.3, -0.2, 0.1)
T_A, T_B = 0.25, 0.7


class Rigid:
    """deform: x -> R_z(2 t) x + t SHIFT, as the offset to x; back=True: its inverse."""

    def __init__(self, back):
        self.back = back

    def step(self, x, t):
        t = t.reshape(-1)[:1]
        c, s = torch.cos(2 * t), torch.sin(2 * t)
        shift = t * torch.tensor(SHIFT, dtype=x.dtype, device=x.device)
        if not self.back:
            y = torch.stack([c * x[:, 0] - s * x[:, 1], s * x[:, 0] + c * x[:, 1], x[:, 2]], 1) + shift
        else:
            z = x - shift
            y = torch.stack([c * z[:, 0] + s * z[:, 1], -s * z[:, 0] + c * z[:, 1], z[:, 2]], 1)
        return (y - x,)


def closed_form(p, t, back):
    p, t = np.asarray(p, np.float64), float(np.float32(t))
    c, s, shift = math.cos(2 * t), math.sin(2 * t), t * np.array(SHIFT)
    if not back:
        return np.stack([c * p[:, 0] - s * p[:, 1], s * p[:, 0] + c * p[:, 1], p[:, 2]], 1) + shift
    z = p - shift
    return np.stack([c * z[:, 0] + s * z[:, 1], -s * z[:, 0] + c * z[:, 1], z[:, 2]], 1)


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


@pytest.fixture(scope="module")
def moving_torus():
    """torus(40, 20) advected to T_A and to T_B by the stub, and torus(36, 18) advected to T_B."""
    C = pkg("correspondence")
    deform, back = Rigid(False), Rigid(True)
    v, f = SR.torus(40, 20)
    v2, f2 = SR.torus(36, 18)
    va, vb, vb2 = C.advect(dev(v), T_A, deform), C.advect(dev(v), T_B, deform), C.advect(dev(v2), T_B, deform)
    return dict(deform=deform, back=back, faces=dev(f), faces2=dev(f2), va=va.contiguous(), vb=vb.contiguous(), vb2=vb2.contiguous(), V=len(v))


@pytest.mark.gpu
def test_transport_equals_the_closed_form(moving_torus):
    C = pkg("correspondence")
    m = moving_torus
    got = C.transport(m["va"], T_A, T_B, m["deform"], m["back"]).cpu().numpy()
    va = m["va"].cpu().numpy()
    ref = closed_form(closed_form(va, T_A, True), T_B, False)
    S = max(np.abs(va).max(), np.abs(ref).max())
    err = np.abs(got - ref).max()
    print(f"transport: max |error| {err / (EPS * S):.2f} eps S (bound 16)")
    assert err <= 16 * EPS * S
    can = C.to_canonical(m["va"], T_A, m["back"]).cpu().numpy()
    assert np.abs(can - SR.torus(40, 20)[0]).max() <= 16 * EPS * S
    assert C.transport(m["va"][:0], T_A, T_B, m["deform"], m["back"]).shape == (0, 3)
    t_dev = torch.tensor([T_A], device=DEV)
    assert torch.equal(C.to_canonical(m["va"], t_dev, m["back"]), C.to_canonical(m["va"], T_A, m["back"]))


@pytest.mark.gpu
def test_correspond_same_connectivity_finds_every_vertex(moving_torus):
    """Every vertex of the torus at T_A, carried to T_B, lies on the torus at T_B at its own vertex: a distance of rounding size, and
    the interpolated one-hot vertex attribute reproduces the identity matrix to 1e-5 (so does the vertex id as a fraction of V; the raw
    id cannot: an off-vertex weight of 1e-6 times an id difference of hundreds)."""
    C = pkg("correspondence")
    m = moving_torus
    V = m["V"]
    r = C.correspond(m["va"], T_A, m["vb"], m["faces"], T_B, m["deform"], m["back"], max_dist=0.05)
    assert set(r) == {"position_free", "face", "bary", "d2", "position"}
    S = float(m["vb"].abs().max())
    dist = float(r["d2"].max().sqrt())
    print(f"same connectivity: found {(r['face'] >= 0).sum().item()} of {V}, max distance {dist / (EPS * S):.2f} eps S (bound 24)")
    assert bool((r["face"] >= 0).all()) and dist <= 24 * EPS * S
    assert float((r["position"] - m["vb"]).abs().max()) <= 24 * EPS * S
    eye = C.interpolate(torch.eye(V, device=DEV), m["faces"], r["face"], r["bary"])
    frac = C.interpolate(torch.arange(V, device=DEV, dtype=torch.float32) / V, m["faces"], r["face"], r["bary"])
    e_eye = float((eye - torch.eye(V, device=DEV)).abs().max())
    e_frac = float((frac - torch.arange(V, device=DEV, dtype=torch.float32) / V).abs().max())
    print(f"identity: one-hot {e_eye:.3e}, id / V {e_frac:.3e} (bound 1e-5)")
    assert e_eye <= 1e-5 and e_frac <= 1e-5


@pytest.mark.gpu
def test_correspond_onto_another_tessellation(moving_torus):
    C = pkg("correspondence")
    m = moving_torus
    V = m["V"]
    r = C.correspond(m["va"], T_A, m["vb2"], m["faces2"], T_B, m["deform"], m["back"])
    free, vb2, f2 = r["position_free"].cpu().numpy(), m["vb2"].cpu().numpy(), m["faces2"].cpu().numpy()
    face, d2 = r["face"].cpu().numpy(), r["d2"].cpu().numpy()
    f64, d64, _ = SR.closest64(free, vb2, f2)
    E = SR.error_unit(vb2, free, np.sqrt(d64))
    D64 = SR.pair_d2(free, vb2, f2, np.float64)
    r_min = np.abs(d2.astype(np.float64) - d64) / E
    r_chosen = (D64[np.arange(V), face] - d64) / E
    print(f"36 x 18: min d2 ratio {r_min.max():.3f} (bound {SR.K_MIN}), chosen-face excess {r_chosen.max():.3f} (bound {SR.K_CHOSEN}); "
          f"distances up to {np.sqrt(d64.max()):.2e}")
    assert (face >= 0).all() and r_min.max() <= SR.K_MIN and r_chosen.max() <= SR.K_CHOSEN
    pos = r["position"].cpu().numpy().astype(np.float64)
    assert np.abs(np.sqrt(((free - pos) ** 2).sum(1)) - np.sqrt(d64)).max() <= 8 * EPS * np.abs(vb2).max()
    # a bound below the tessellation gap (up to 8e-3): the vertices between the other torus's leave unmatched
    tight = C.correspond(m["va"], T_A, m["vb2"], m["faces2"], T_B, m["deform"], m["back"], max_dist=0.002)
    lost = (tight["face"] < 0).cpu().numpy()
    print(f"max_dist 0.002: {lost.sum()} of {V} unmatched")
    assert 0 < lost.sum() < V
    assert np.array_equal(lost, ~(d2 < np.float32(C.max_d2_of(0.002))))
    p = tight["position"].cpu().numpy()
    assert np.isnan(p[lost]).all() and np.isfinite(p[~lost]).all() and np.isinf(tight["d2"].cpu().numpy()[lost]).all()
    assert torch.equal(tight["position"][~torch.as_tensor(lost, device=DEV)], r["position"][~torch.as_tensor(lost, device=DEV)])


class Identity:
    """Both networks of a mesh that does not move: a zero offset."""

    def step(self, x, t):
        return (torch.zeros_like(x),)


@pytest.mark.gpu
@pytest.mark.parametrize("max_dist", [1.0 / 23, math.inf])
def test_correspond_marching_cubes_sphere_onto_itself(max_dist):
    """SR.mc_sphere(1e-6): a marching-cubes mesh whose isosurface grazes six lattice nodes -- 96 faces thinner than 1e-3, 72 thinner
    than 1e-5, edges down to 8e-8.  Under the identity motion every vertex is found on its own mesh, within one voxel and without a
    bound, at a distance of at most 8 eps S, and its barycentrics rebuild it within 8 eps S (the bound of
    tests/test_surface_host.py::test_barycentrics_are_a_point_of_the_face: the roundings of v, w and (1 - v) - w, each eps S)."""
    C = pkg("correspondence")
    verts, faces = SR.mc_sphere(1e-6)
    v, f, still = dev(verts), dev(faces), Identity()
    r = C.correspond(v, T_A, v, f, T_B, still, still, max_dist=max_dist)
    assert torch.equal(r["position_free"], v)
    S = float(np.abs(verts).max())
    dist = float(r["d2"].max().sqrt())
    rebuilt = float((r["position"] - v).double().pow(2).sum(1).sqrt().max())
    face, bary = r["face"].cpu().numpy(), r["bary"].cpu().numpy()
    thin = (SR.thinness(verts, faces)[face[face >= 0]] < 1e-3).sum()
    print(f"mc_sphere(1e-6) onto itself, max_dist {max_dist:.4f}: found {(face >= 0).sum()} of {len(verts)} ({thin} on a face thinner than "
          f"1e-3), max distance {dist / (EPS * S):.2f} eps S, rebuilt within {rebuilt / (EPS * S):.2f} eps S (bounds 8)")
    assert (face >= 0).all() and dist <= 8 * EPS * S and rebuilt <= 8 * EPS * S
    assert bary.min() >= -4 * EPS and bary.max() <= 1 + 4 * EPS


# ---- drivers --------------------------------------------------------------------------------------------------------------------------
N_FRAMES, SIDE, K_TRACKS = 3, 176, 256


@pytest.fixture(scope="module")
def scene():
    """The scene of tests/test_visualize.py: 2 000 Gaussians, DPSR at 48^3, three 176 x 176 cameras, the mesh phase on DiffMC's mesh."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_trainer_dp_gpu import make_mesh_trainer
    T = pkg("trainer")
    base = make_mesh_trainer(0, 1, res=48, P=2000, W=SIDE, H=SIDE, n_frames=3)
    g = base.g
    mesh = T.MeshPhase(*base.mesh.networks(), dpsr=base.mesh.dpsr, n_verts=4000, scale=1.0, device=g.get_xyz.device,
                       mesh_source="diffmc", mesh_losses="render")
    mesh.bind(g)
    return dict(g=g, deform=base.deform, deform_back=base.deform_back, cameras=base.cameras, mesh=mesh)


def _record_psr(mesh):
    """DPSR's splat accumulates with float atomics: every phi the driver computes is kept, in call order, and the independent
    evaluation continues from it (as tests/test_visualize.py does)."""
    fields, orig = [], mesh.psr

    def psr(*a, **k):
        fields.append(orig(*a, **k))
        return fields[-1]

    mesh.psr = psr
    return fields, orig


def _check_report(rep, n, mode):
    C = pkg("correspondence")
    assert set(rep) >= {"frames", "columns", "t_ref", "mode", "palette", "search_dist", "voxel", "grid_res", "n_tracks"}
    assert rep["mode"] == mode and rep["grid_res"] == 48 and len(rep["frames"]) == n and tuple(rep["columns"]) == C.COLUMNS
    assert abs(rep["search_dist"] - 4 * rep["voxel"]) < 1e-12 and rep["voxel"] > 0
    for row in rep["frames"]:
        assert set(row) == {"t"} | set(C.COLUMNS)
        assert 0 < row["n_found"] <= row["n_queries"]
        assert 0 <= row["mean_dist"] <= row["max_dist"] <= rep["search_dist"] * (1 + 1e-6)  # (d2 < fp32(max_dist^2), strict)
        assert abs(row["mean_dist_voxels"] * rep["voxel"] - row["mean_dist"]) < 1e-9


@pytest.mark.gpu
def test_render_correspondence_frames(scene, tmp_path):
    C, V, MRast = pkg("correspondence"), pkg("visualize"), pkg("mesh_raster")
    g, mesh, cams = scene["g"], scene["mesh"], scene["cameras"]
    deform, back = scene["deform"], scene["deform_back"]
    fields, orig = _record_psr(mesh)
    try:
        res = C.render_correspondence(g, deform, back, cams[0], mesh=mesh, total_frames=N_FRAMES, n_tracks=K_TRACKS, out_dir=str(tmp_path))
    finally:
        mesh.psr = orig
    frames = res["frames"]
    assert frames.shape == (N_FRAMES, SIDE, 3 * SIDE, 3) and frames.dtype == np.uint8 and len(fields) == N_FRAMES + 1
    assert res["tracks"].shape == (N_FRAMES, K_TRACKS, 3) and res["tracks"].dtype == np.float32
    _check_report(res["report"], N_FRAMES, "reference")
    assert json.load(open(tmp_path / "correspondence" / "report.json")) == json.loads(json.dumps(res["report"]))
    assert sorted(os.listdir(tmp_path / "images")) == [f"{i:04d}.png" for i in range(N_FRAMES)]
    orbit = V.trajectory_cameras(4.0, 1.0, N_FRAMES, cams[0])
    with torch.no_grad():
        t_ref = torch.zeros(1, device=DEV)
        ref_verts, ref_faces = mesh.surface(g, fields[0])
        voxel = 2.0 * float(g.gaussian_scale.reshape(-1)[0]) / 48
        for i in (0, N_FRAMES - 1):
            cam = orbit[i]
            verts, faces = mesh.surface(g, fields[1 + i])
            verts = verts.contiguous()
            snap = C.correspond(verts, cam.fid, ref_verts.contiguous(), ref_faces, t_ref, deform, back, max_dist=4 * voxel)
            color = C.palette(C.to_canonical(snap["position"], t_ref, back), g.gaussian_center, g.gaussian_scale, "checker", 8)
            panel = MRast.render_mesh(None, verts, faces, color, cam, whitebackground=True)
            mine = V.compose_frame([panel], 1).cpu().numpy()
            found = int((snap["face"] >= 0).sum())
            row = res["report"]["frames"][i]
            print(f"frame {i}: V {verts.shape[0]} F {faces.shape[0]}, found {found}, mean snap {row['mean_dist_voxels']:.3f} voxels, "
                  f"max {row['max_dist_voxels']:.3f}; panel 2 differs in {(mine != frames[i][:, SIDE:2 * SIDE]).sum()} bytes")
            assert np.array_equal(mine, frames[i][:, SIDE:2 * SIDE])
            assert (row["n_queries"], row["n_found"]) == (verts.shape[0], found)
            mean = float(torch.where(snap["face"] >= 0, snap["d2"].double().sqrt(), torch.zeros((), dtype=torch.float64, device=DEV)).sum()) / found
            assert abs(row["mean_dist"] - mean) <= 1e-12 * max(mean, 1e-30)
            # panel 3: dots only, each in the colour of a track or white
            dots = frames[i][:, 2 * SIDE:]
            assert (dots != 255).any(-1).sum() > 20
            assert (frames[i][:, :SIDE] != 255).any(-1).sum() > 200
        # frame 0 is the reference frame itself: every vertex lies on mesh(t_ref) up to the networks' round trip
        assert res["report"]["frames"][0]["n_found"] > 0
    found_tracks = ~np.isnan(res["tracks"]).any(-1)
    print(f"tracks found per frame: {found_tracks.sum(1).tolist()} of {K_TRACKS}")
    assert found_tracks.any()


@pytest.mark.gpu
def test_export_correspondence_files_and_modes(scene, tmp_path):
    C, io = pkg("correspondence"), pkg("ply_io")
    g, mesh = scene["g"], scene["mesh"]
    out = {}
    for mode in ("reference", "canonical"):
        d = tmp_path / mode
        out[mode] = C.export_correspondence(g, scene["deform"], scene["deform_back"], mesh, str(d), frames=2, mode=mode, palette="rgb",
                                            n_tracks=K_TRACKS, seed=3)
        res = out[mode]
        assert res["paths"] == [str(d / "correspondence" / f"frame_{i}.ply") for i in range(2)]
        _check_report(res["report"], 2, mode)
        assert json.load(open(res["report_path"])) == json.loads(json.dumps(res["report"]))
        for i, p in enumerate(res["paths"]):
            v, f, c = io.read_mesh_ply(p, return_colors=True)
            print(f"{mode} {os.path.basename(p)}: V {len(v)} F {len(f)} colours {c[:, :3].min()}..{c[:, :3].max()}")
            assert len(v) == res["report"]["frames"][i]["n_queries"] and len(f) > 0 and c.shape == (len(v), 4) and c.dtype == np.uint8
            assert c[:, :3].max() > 1 and (c[:, 3] == 255).all() and f.min() >= 0 and f.max() < len(v)
        z = np.load(res["tracks_path"])
        assert sorted(z.files) == ["found", "times", "tracks"]
        assert z["tracks"].shape == (2, K_TRACKS, 3) and z["tracks"].dtype == np.float32 and z["found"].shape == (2, K_TRACKS)
        assert np.array_equal(z["found"], ~np.isnan(z["tracks"]).any(-1)) and np.array_equal(z["times"], np.float32([0.0, 0.5]))
        assert z["found"].any()
    # the snap statistics do not depend on the colouring mode (DPSR's atomics move the mesh by rounding only)
    a, b = out["reference"]["report"]["frames"], out["canonical"]["report"]["frames"]
    assert all(abs(x["n_queries"] - y["n_queries"]) <= 0.02 * x["n_queries"] for x, y in zip(a, b))


@pytest.mark.gpu
def test_driver_errors(scene, tmp_path):
    C, T = pkg("correspondence"), pkg("trainer")
    g, cams = scene["g"], scene["cameras"]
    bare = T.MeshPhase(*scene["mesh"].networks(), dpsr=None, n_verts=100, scale=1.0, device=g.get_xyz.device)
    with pytest.raises(RuntimeError, match="MeshPhase with a DPSR module"):
        C.render_correspondence(g, scene["deform"], scene["deform_back"], cams[0], mesh=bare, total_frames=2)
    with pytest.raises(RuntimeError, match="MeshPhase with a DPSR module"):
        C.export_correspondence(g, scene["deform"], scene["deform_back"], bare, str(tmp_path), frames=2)
    with pytest.raises(ValueError, match="total_frames must be >= 1"):
        C.render_correspondence(g, scene["deform"], scene["deform_back"], cams[0], mesh=scene["mesh"], total_frames=0)
    with pytest.raises(ValueError, match="frames must be >= 1"):
        C.export_correspondence(g, scene["deform"], scene["deform_back"], scene["mesh"], str(tmp_path), frames=0)
    with pytest.raises(ValueError, match="mode must be one of"):
        C.render_correspondence(g, scene["deform"], scene["deform_back"], cams[0], mesh=scene["mesh"], total_frames=2, mode="nearest")
    assert not os.path.exists(tmp_path / "correspondence")
