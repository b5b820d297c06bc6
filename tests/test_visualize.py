"""dg-mesh_amd/visualize.py on the GPU: the four kernels of csrc/visualize.hip against the numpy restatement (tests/_visualize_ref.py)
and the drivers end to end on a small mesh-phase scene.

Tolerance rule for the float passes (vertex normals, shade): 4 x the largest deviation of the float32 restatement from the float64
one on the same inputs, computed in the test, floor 1e-6 (_visualize_ref.tolerance).  The kernel orders its sums differently
(atomics) and uses the device's sqrt / pow, hence the factor; the tolerance never comes from the kernel's output.  The splat and
the composition are compared exactly.  Every test prints its figures before it asserts."""
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

import _visualize_ref as VR
from conftest import ROOT, pkg
from test_mesh_raster import _tilt, uv_sphere

DEV = "cuda"


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


@pytest.fixture(scope="module")
def sphere():
    """Tilted uv_sphere(16, 12) in float32, plus one unreferenced vertex, one zero-area face and one face with an index out of range."""
    v, f = uv_sphere(16, 12)
    v = np.vstack([v @ _tilt().T, [[0.3, -0.2, 0.1]]]).astype(np.float32)
    f = np.vstack([f, [[0, 0, 5]], [[1, 2, len(v) + 3]]]).astype(np.int32)
    return v, f


def camera(H, W, **kw):
    syn, S = pkg("synthetic"), pkg("scene")
    cam = syn.make_camera(W, H, **kw)
    return cam, S.TorchCamera(cam, DEV)


# ---- vertex normals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_vertex_normals_against_fp64(sphere):
    """float32 restatement vs float64 on this mesh: 1.1e-7, so the tolerance is its floor, 1e-6.  Kernel vs float64: not measured yet
    (no GPU run has completed)."""
    V = pkg("visualize")
    v, f = sphere
    got = V.vertex_normals(dev(v), dev(f)).cpu().numpy()
    ref = VR.vertex_normals(v, f, np.float64)
    tol, spread = VR.tolerance(VR.vertex_normals(v, f, np.float32), ref)
    err = np.abs(got - ref).max()
    print(f"vertex normals: fp32 restatement vs fp64 {spread:.3e}, tolerance {tol:.3e}, kernel vs fp64 {err:.3e}")
    assert err <= tol
    assert np.array_equal(got[-1], np.zeros(3, np.float32)) and np.array_equal(ref[-1], np.zeros(3))
    empty = V.vertex_normals(dev(v), torch.zeros((0, 3), dtype=torch.int32, device=DEV))
    assert torch.equal(empty, torch.zeros_like(empty))
    with pytest.raises(RuntimeError):
        V.vertex_normals(torch.tensor(v), torch.tensor(f))


# ---- shade ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(67, 45), (45, 67), (1, 1)])
def test_shade_against_fp64(sphere, H, W, monkeypatch):
    """The GPU rast of the sphere feeds the kernel and the restatement; the light is the headlight, computed in each one's own
    precision.  float32 restatement vs float64: 1.1e-7 to 1.9e-7 at the two larger sizes, so the tolerance is its floor, 1e-6.  Kernel
    vs float64: not measured yet (no GPU run has completed)."""
    V, MRast = pkg("visualize"), pkg("mesh_raster")
    v, f = sphere
    cam_np, cam = camera(H, W)
    verts, faces = dev(v), dev(f)
    rast, _ = MRast.rasterize(None, MRast.clip_positions(cam, verts), faces, (H, W))
    bg = (0.25, 1.0, 0.75)
    # vertex_normals sums with float atomics, so two calls may differ in their last bits: the normals of the first call are kept
    # for the second, and the two images are then compared bit for bit
    kept, orig = [], V.vertex_normals
    monkeypatch.setattr(V, "vertex_normals", lambda a, b: kept[0] if kept else kept.append(orig(a, b)) or kept[0])
    img = V.mesh_shape_renderer(verts, faces, cam, rast=rast, background=bg)
    own = V.mesh_shape_renderer(verts, faces, cam, background=bg)
    assert tuple(img.shape) == (H, W, 3) and img.dtype == torch.float32 and torch.equal(img, own)
    rast_np, got = rast[0].cpu().numpy(), img.cpu().numpy()
    out = {}
    for dt in (np.float64, np.float32):
        out[dt] = VR.shade(v, VR.vertex_normals(v, f, dt), f, rast_np, VR.headlight(v, cam_np.camera_center, dt), cam_np.camera_center, dt,
                           background=bg)
    covered = rast_np[..., 3] > 0
    tol, spread = VR.tolerance(out[np.float32], out[np.float64])
    err = np.abs(got - out[np.float64]).max()
    print(f"shade {H}x{W}: {covered.sum()} covered pixels, fp32 restatement vs fp64 {spread:.3e}, tolerance {tol:.3e}, kernel vs fp64 {err:.3e}")
    assert err <= tol
    assert np.array_equal(got[~covered], np.broadcast_to(np.float32(bg), got[~covered].shape))
    if H > 1:
        assert covered.sum() > 100 and (~covered).sum() > 100
        assert got[covered].min() >= 0.5 and got[covered].max() > 0.8  # (ambient; a lit surface)
    none = V.mesh_shape_renderer(verts, torch.zeros((0, 3), dtype=torch.int32, device=DEV), cam, background=bg)
    assert torch.equal(none, torch.tensor(bg, device=DEV).expand(H, W, 3))
    with pytest.raises(TypeError):
        V.mesh_shape_renderer(verts, faces, cam, glossiness=3.0)


@pytest.mark.gpu
def test_shade_on_a_diffmc_sphere_is_lit():
    """DiffMC on a 32^3 sphere SDF, shaded as the drivers shade (no flip): the surface is lit, so DiffMC's winding is outward.
    With the default material the brightest possible value is ambient + k_d + k_s = 0.84, so the 0.9 bound is checked with
    diffuse = 0.5 (a lit centre then saturates towards 1, an unlit one stays at ambient = 0.5); with the defaults the centre must
    reach ambient + 0.99 k_d (the centre normal faces the headlight to within the 32^3 discretisation).  No covered pixel is below
    ambient - 1e-6 (the tolerance floor: the rule only adds non-negative terms to ambient).  flip_normals turns the light off."""
    V, MC = pkg("visualize"), pkg("marching_cubes")
    n = 32
    ax = torch.arange(n, dtype=torch.float32, device=DEV)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    c = (n - 1) / 2
    grid = torch.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - 10.3
    verts, faces = MC.DiffMC()(grid)
    verts = (verts * 2.0 - 1.0).contiguous()
    H = W = 65
    _, cam = camera(H, W)
    strong = V.mesh_shape_renderer(verts, faces, cam, diffuse=0.5)
    plain = V.mesh_shape_renderer(verts, faces, cam)
    flipped = V.mesh_shape_renderer(verts, faces, cam, flip_normals=True)
    covered = (plain != 1.0).any(-1)
    print(f"DiffMC sphere: V {verts.shape[0]} F {faces.shape[0]}, {int(covered.sum())} covered pixels; centre: diffuse 0.5 -> "
          f"{float(strong[H // 2, W // 2, 0]):.6f}, defaults -> {float(plain[H // 2, W // 2, 0]):.6f}, flipped -> "
          f"{float(flipped[H // 2, W // 2, 0]):.6f}; min over covered {float(plain[covered].min()):.6f}")
    assert int(covered.sum()) > 200 and bool(covered[H // 2, W // 2])
    assert float(strong[H // 2, W // 2].min()) > 0.9
    assert float(plain[H // 2, W // 2].min()) > 0.5 + 0.99 * 0.3
    assert float(plain[covered].min()) >= 0.5 - 1e-6 and float(strong[covered].min()) >= 0.5 - 1e-6
    assert abs(float(flipped[H // 2, W // 2, 0]) - 0.5) <= 1e-6


# ---- splat ----------------------------------------------------------------------------------------------------------------------------
def clip_points(sx, sy, zw, w, H, W):
    """float32 clip positions whose screen position is (sx, sy) pixels at depth z/w = zw."""
    sx, sy, zw, w = (np.asarray(a, np.float64) for a in (sx, sy, zw, w))
    return np.stack([(sx / (0.5 * W) - 1.0) * w, (sy / (0.5 * H) - 1.0) * w, zw * w, w], 1).astype(np.float32)


def assert_clear_of_pixel_boundaries(p, H, W):
    """Every finite screen coordinate lies at least 1/64 px from a pixel boundary, so float32 rounding cannot move a point across."""
    sx, sy, _ = VR.screen(p, H, W, np.float64)
    ok = np.isfinite(p).all(1) & (p[:, 3] > 0)
    for s in (sx[ok], sy[ok]):
        assert (np.abs(s - np.round(s)) >= 1.0 / 64).all()


def special_points(H, W):
    sx = [10.5, 10.3, 20.5, 20.5, 30.5, 31.5, 33.5, W + 20.5, 0.5, W - 0.5, 30.5, 0.5, W - 0.25, 40.5, 41.5]
    sy = [10.5, 10.7, 5.5, 5.5, 30.5, 30.5, 30.5, 12.5, 0.5, 7.5, H - 0.5, 20.5, H - 0.25, -1.5, 40.5]
    zw = [0.5, 0.3, 0.4, 0.4, 0.5, 0.5, 0.5, 0.5, 0.6, 0.6, 0.6, 0.6, 0.7, 0.2, -0.3]
    w = [1.0, 2.0, 1.5, 1.5, -1.0, 0.0, 1.0, 1.0, 1.0, 2.0, 0.5, 3.0, 1.0, 1.0, 1.0]
    p = clip_points(sx, sy, zw, w, H, W)
    p[6, 0] = np.nan          # a NaN point
    p = np.vstack([p, [[np.inf, 0.0, 0.5, 1.0]], [[0.1, 0.1, 0.5, np.inf]]]).astype(np.float32)
    assert np.array_equal(p[2], p[3])  # equal depth, same pixel: the lower id wins
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("case,size", [("special", 1), ("special", 3), ("special", 5), ("random", 1), ("random", 3), ("empty", 3)])
def test_splat_equals_the_restatement(case, size):
    V = pkg("visualize")
    H, W = 48, 64
    rng = np.random.RandomState(5)
    if case == "special":
        p = special_points(H, W)
    elif case == "random":
        N = 5000
        frac = lambda: 1.0 / 32 + rng.rand(N) * 15.0 / 16
        p = clip_points(np.floor(rng.uniform(-4, W + 4, N)) + frac(), np.floor(rng.uniform(-4, H + 4, N)) + frac(),
                        np.round(rng.uniform(0.1, 0.9, N), 2), rng.uniform(0.5, 3.0, N), H, W)  # (depths on a coarse grid: ties happen)
    else:
        p = np.zeros((0, 4), np.float32)
    assert_clear_of_pixel_boundaries(p, H, W)
    colors = rng.rand(len(p), 3).astype(np.float32)
    ids_ref = VR.splat_ids(p, H, W, size)
    pos = dev(p)
    for cols, kw in ((None, dict(color=(0.1, 0.2, 0.9), background=(1.0, 0.5, 0.0))), (colors, {})):
        img, ids = V.splat_points(pos, H, W, colors=None if cols is None else dev(cols), size=size, return_ids=True, **kw)
        img2 = V.splat_points(pos[None], H, W, colors=None if cols is None else dev(cols), size=size, **kw)
        assert torch.equal(img, img2)  # two runs are bit-identical
        ids = ids.cpu().numpy()
        print(f"splat {case} size {size}: {(ids_ref >= 0).sum()} covered pixels, {len(np.unique(ids_ref)) - 1} winners, "
              f"{(ids != ids_ref).sum()} id mismatches")
        assert np.array_equal(ids, ids_ref)
        assert np.array_equal(img.cpu().numpy(), VR.splat_image(ids_ref, cols, kw.get("color", (0.0, 0.0, 1.0)), kw.get("background", (1.0, 1.0, 1.0))))
    if case == "special":
        assert ids_ref[10, 10] == 1 and ids_ref[5, 20] == 2 and not np.isin(ids_ref, [4, 5, 6, 7, 15, 16]).any()
        assert ids_ref[0, 0] == 8 and ids_ref[7, W - 1] == 9 and ids_ref[H - 1, 30] == 10 and ids_ref[20, 0] == 11 and ids_ref[H - 1, W - 1] == 12
        assert (ids_ref == 8).sum() == ((size + 1) // 2) ** 2 and (ids_ref == 13).sum() == (size if size >= 5 else 0)
        assert ids_ref[40, 41] == 14  # (a negative z/w orders below the positive ones)
    if case == "empty":
        assert (ids_ref == -1).all()


@pytest.mark.gpu
def test_pointcloud_renderer_and_argument_checks():
    V, MRast = pkg("visualize"), pkg("mesh_raster")
    H, W = 48, 64
    _, cam = camera(H, W)
    pts = dev(np.random.RandomState(1).uniform(-1, 1, (500, 3)).astype(np.float32))
    img = V.pointcloud_renderer(pts, cam)
    ref = V.splat_points(MRast.clip_positions(cam, pts), H, W)
    assert torch.equal(img, ref)
    blue = (img == torch.tensor([0.0, 0.0, 1.0], device=DEV)).all(-1)
    white = (img == 1.0).all(-1)
    assert int(blue.sum()) > 100 and bool((blue | white).all())
    for bad in (0, 2, 17):
        with pytest.raises(ValueError):
            V.splat_points(MRast.clip_positions(cam, pts), H, W, size=bad)
    with pytest.raises(RuntimeError):
        V.splat_points(torch.zeros(4, 4), H, W)


# ---- compose --------------------------------------------------------------------------------------------------------------------------
SPECIAL_VALUES = np.array([0.0, 1.0, 0.999999, 254.5 / 255, -0.5, -1e-9, 1.5, 1e9, np.nan, np.inf, -np.inf, 0.5, 127.5 / 255], np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(10, 14), (64, 48)])
@pytest.mark.parametrize("n", [1, 3, 4])
@pytest.mark.parametrize("d", [1, 2])
def test_compose_bytes_equal_the_restatement(H, W, n, d):
    V = pkg("visualize")
    rng = np.random.RandomState(100 * n + 10 * d + H)
    panels_np, panels = [], []
    for k in range(n):
        a = rng.uniform(-0.2, 1.2, (H, W, 3)).astype(np.float32)  # (H, W, 3) values; the layouts differ below
        a.reshape(-1)[rng.choice(a.size, 4 * len(SPECIAL_VALUES), replace=False)] = np.tile(SPECIAL_VALUES, 4)
        a[0, 0], a[1, 0], a[0, 1], a[1, 1] = SPECIAL_VALUES[3], 1.0, 1.0, 1.0  # a 2x2 block just below 1
        panels_np.append(a)
        if k % 3 == 0:
            panels.append(dev(a))                                            # (H, W, 3)
        elif k % 3 == 1:
            panels.append(dev(np.transpose(a, (2, 0, 1))))                   # (3, H, W), contiguous
        else:
            panels.append(dev(a).permute(2, 0, 1))                           # (3, H, W), a view of (H, W, 3) memory (as render_mesh's)
    got = V.compose_frame(panels, d)
    ref = VR.compose(panels_np, d)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (H // d, n * (W // d), 3) == ref.shape
    diff = (got.cpu().numpy() != ref).sum()
    print(f"compose {H}x{W} n={n} d={d}: {diff} differing bytes of {ref.size}")
    assert diff == 0
    out = torch.zeros((2,) + ref.shape, dtype=torch.uint8, device=DEV)
    assert V.compose_frame(panels, d, out=out[1]) is not None and np.array_equal(out[1].cpu().numpy(), ref) and int(out[0].max()) == 0


@pytest.mark.gpu
def test_compose_argument_errors():
    V = pkg("visualize")
    a, b, odd = torch.rand(3, 10, 14, device=DEV), torch.rand(12, 14, 3, device=DEV), torch.rand(9, 14, 3, device=DEV)
    with pytest.raises(ValueError):
        V.compose_frame([a, b])              # sizes differ
    with pytest.raises(ValueError):
        V.compose_frame([a] * 5)             # more than four
    with pytest.raises(ValueError):
        V.compose_frame([odd], 2)            # odd H at d = 2
    with pytest.raises(ValueError):
        V.compose_frame([])
    with pytest.raises(RuntimeError):
        V.compose_frame([a.cpu()])


# ---- drivers --------------------------------------------------------------------------------------------------------------------------
N_VIEWS, SIDE = 3, 176


@pytest.fixture(scope="module")
def scene():
    """The scene of tests/test_evaluate.py: the mesh trainer of test_trainer_dp_gpu (2 000 Gaussians, DPSR at 48^3, three 176x176
    cameras) with its mesh phase on DiffMC's mesh."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_trainer_dp_gpu import make_mesh_trainer
    T = pkg("trainer")
    base = make_mesh_trainer(0, 1, res=48, P=2000, W=SIDE, H=SIDE, n_frames=N_VIEWS)
    g = base.g
    mesh = T.MeshPhase(*base.mesh.networks(), dpsr=base.mesh.dpsr, n_verts=4000, scale=1.0, device=g.get_xyz.device,
                       mesh_source="diffmc", mesh_losses="render")
    mesh.bind(g)
    return dict(g=g, deform=base.deform, deform_back=base.deform_back, cameras=base.cameras, mesh=mesh)


def _record_psr(mesh):
    """DPSR's splat accumulates with float atomics, so two evaluations of phi differ in their last bits: every phi the driver computes
    is kept, in call order, and the independent evaluation continues from it (as tests/test_evaluate.py does)."""
    fields, orig = [], mesh.psr

    def psr(*a, **k):
        fields.append(orig(*a, **k))
        return fields[-1]

    mesh.psr = psr
    return fields, orig


def decode_png(data):
    """8-bit RGB, non-interlaced PNG -> (H, W, 3) uint8, with the standard library: chunk CRCs checked, all five row filters."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, tag = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        at += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT"))
    stride = 3 * W
    assert len(raw) == H * (stride + 1)
    out, prev = np.zeros((H, stride), np.uint8), np.zeros(stride, np.int64)
    for y in range(H):
        f, line = raw[y * (stride + 1)], np.frombuffer(raw, np.uint8, stride, y * (stride + 1) + 1).astype(np.int64)
        if f in (0, 2):
            cur = (line + (prev if f == 2 else 0)) & 255
        else:
            cur = np.zeros(stride, np.int64)
            for i in range(stride):
                a, b, c = (cur[i - 3] if i >= 3 else 0), prev[i], (prev[i - 3] if i >= 3 else 0)
                if f == 1:
                    pred = a
                elif f == 3:
                    pred = (a + b) // 2
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[i] = (line[i] + pred) & 255
        out[y], prev = cur, cur
    return out.reshape(H, W, 3)


@pytest.mark.gpu
def test_render_test_frames(scene, tmp_path):
    V, MRast = pkg("visualize"), pkg("mesh_raster")
    g, mesh, cams = scene["g"], scene["mesh"], scene["cameras"]
    fields, orig = _record_psr(mesh)
    try:
        res = V.render_test(g, scene["deform"], scene["deform_back"], cams, mesh=mesh, out_dir=str(tmp_path))
    finally:
        mesh.psr = orig
    frames = res["frames"]
    h = SIDE // 2
    assert frames.shape == (N_VIEWS, h, 3 * h, 3) and frames.dtype == np.uint8 and len(fields) == N_VIEWS
    assert res["fps"] > 0 and abs(res["fps"] * res["time_per_frame"] - 1.0) < 1e-12
    with torch.no_grad():
        cam = cams[0]
        verts, faces = mesh.surface(g, fields[0])
        t_v = cam.fid.reshape(1, 1).expand(verts.shape[0], -1)
        color = mesh.appearance.step(verts + scene["deform_back"].step(verts, t_v)[0], t_v)
        mi = MRast.render_mesh(None, verts, faces, color, cam, whitebackground=True)
        assert np.array_equal(frames[0][:, h:2 * h], V.compose_frame([mi], 2).cpu().numpy())
        assert np.array_equal(frames[0][:, :h], V.compose_frame([cam.original_image], 2).cpu().numpy())
        # the shape panel: vertex_normals sums with float atomics, so an independent evaluation agrees to a byte's rounding
        shape = V.compose_frame([V.mesh_shape_renderer(verts.contiguous(), faces, cam)], 2).cpu().numpy().astype(np.int64)
        third = frames[0][:, 2 * h:].astype(np.int64)
        print(f"render_test: V {verts.shape[0]} F {faces.shape[0]}; shape panel: {(third != 255).any(-1).sum()} non-white pixels, "
              f"max byte difference to an independent evaluation {np.abs(third - shape).max()}; {res['fps']:.1f} frames/s")
        assert np.abs(third - shape).max() <= 1 and (third != 255).any(-1).sum() > 200
    for idx in range(N_VIEWS):
        data = open(tmp_path / "images" / f"{idx:04d}.png", "rb").read()
        assert np.array_equal(decode_png(data), frames[idx])
    assert sorted(os.listdir(tmp_path / "images")) == [f"{i:04d}.png" for i in range(N_VIEWS)]


@pytest.mark.gpu
def test_render_trajectory_frames(scene):
    V, MRast = pkg("visualize"), pkg("mesh_raster")
    g, cams = scene["g"], scene["cameras"]
    n = 4
    res = V.render_trajectory(g, scene["deform"], scene["deform_back"], cams[0], mesh=scene["mesh"], total_frames=n)
    frames = res["frames"]
    assert frames.shape == (n, SIDE, 3 * SIDE, 3) and frames.dtype == np.uint8
    orbit = V.trajectory_cameras(4.0, 1.0, n, cams[0])
    with torch.no_grad():
        for i, cam in enumerate(orbit):
            assert abs(float(cam.fid) - i / n) < 1e-7 and cam.world_view_transform.is_cuda
            cloud = frames[i][:, 2 * SIDE:]
            blue = (cloud == np.array([0, 0, 255], np.uint8)).all(-1)
            white = (cloud == 255).all(-1)
            xyz = g.get_xyz.detach()
            d_xyz = scene["deform"].step(xyz, cam.fid.reshape(1, 1).expand(xyz.shape[0], -1))[0]
            p = MRast.clip_positions(cam, xyz + d_xyz)[0].double().cpu().numpy()
            p = p[p[:, 3] > 0]
            px = np.floor((p[:, 0] / p[:, 3] + 1) * SIDE / 2).astype(np.int64)
            py = np.floor((p[:, 1] / p[:, 3] + 1) * SIDE / 2).astype(np.int64)
            sil = np.zeros((SIDE, SIDE), bool)
            for dy in range(-3, 4):  # the centres' own silhouette, dilated by 3 px
                for dx in range(-3, 4):
                    x, y = px + dx, py + dy
                    ok = (x >= 0) & (x < SIDE) & (y >= 0) & (y < SIDE)
                    sil[y[ok], x[ok]] = True
            print(f"trajectory frame {i}: {blue.sum()} blue pixels, {(blue & ~sil).sum()} outside the dilated silhouette; "
                  f"mesh panel {(frames[i][:, :SIDE] != 255).any(-1).sum()} / shape panel {(frames[i][:, SIDE:2 * SIDE] != 255).any(-1).sum()} non-white")
            assert blue.sum() > 200 and (blue | white).all() and not (blue & ~sil).any()
            assert (frames[i][:, SIDE:2 * SIDE] != 255).any(-1).sum() > 200
    with pytest.raises(ValueError):
        V.render_trajectory(g, scene["deform"], scene["deform_back"], cams[0], mesh=scene["mesh"], radius=1.0, elevation=1.0)


@pytest.mark.gpu
def test_export_dynamic_mesh(scene, tmp_path):
    V, io = pkg("visualize"), pkg("ply_io")
    paths = V.export_dynamic_mesh(scene["g"], scene["deform"], scene["deform_back"], scene["mesh"], str(tmp_path), frames=3)
    assert paths == [str(tmp_path / "dynamic_mesh" / f"frame_{i}.ply") for i in range(3)]
    for p in paths:
        v, f, c = io.read_mesh_ply(p, return_colors=True)
        print(f"{os.path.basename(p)}: V {len(v)} F {len(f)} colours {c[:, :3].min()}..{c[:, :3].max()}")
        assert len(v) > 0 and len(f) > 0 and c.shape == (len(v), 4) and c.dtype == np.uint8
        assert c[:, :3].max() > 1 and (c[:, 3] == 255).all() and f.min() >= 0 and f.max() < len(v)
