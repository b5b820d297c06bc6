"""A scene on disk in the Blender / D-NeRF layout -- transforms_train.json, transforms_test.json, RGBA PNGs, a `time` per frame --
as the cameras, ground-truth images and initial point cloud that training needs.

  read_blender_scene  <- readNerfSyntheticInfo / readCamerasFromTransforms (R/scene/dataset_readers.py:262-352), getNerfppNorm
                         (:93-114), fetchPly / storePly (:183-208); camera matrices as R/scene/cameras.py:54-71
  Scene               <- R/scene/__init__.py:25-141, cameraList_from_camInfos / camera_to_JSON (R/utils/camera_utils.py:23-95)
(R/ = dgmesh/.)  The images never pass through the host as pixels: png_io.decode_pngs inflates the files on the host and undoes
the PNG filters on the device, image_ingest composites them over the background there (csrc/ingest.hip), and `downsample` and
`resolution` resize them there with Pillow's arithmetic (resample.py, csrc/resample.hip).

The reader only reads PNG headers, so resizing is a stage of Scene._load, in the reference's order: decode; Lanczos on the file's
bytes when `downsample` changes the size (dataset_readers.py:289; RGBA through Pillow's premultiplied path); composite; bicubic
when `resolution` changes the size again (loadCam, R/utils/camera_utils.py:23-46); divide by 255.  CameraInfo.width, height and FoVy
and cameras.json follow the downsampled size, the TorchCameras the final one; FoVs do not depend on `resolution`.

Deviation from the reference: it swaps the two field-of-view names (FovY = fovx; FovX = fovy, dataset_readers.py:304-306), which is
harmless for square images and wrong otherwise.  Here FoVx is the file's camera_angle_x and FoVy follows from the aspect ratio.
Under `resolution` the reference resizes the image and leaves the alpha mask at its old size, so its mask loss cannot run; here the
alpha plane is resampled with the same bicubic filter as a fourth, non-premultiplied channel and the mask always has the image's size.
Nerfies, iPhone and NeuralActor scenes have other readers in the reference; theirs are in captures.py, which Scene asks first
(READERS here keeps a stub per name that raises).  Their cameras carry an intrinsic matrix K and a mask_path: Scene._load decodes
the masks beside the frames (png_io.decode_mask_groups) and composites with image_ingest_masked.
read_blender_scene itself still reads at file size only (downsample=1.0); Scene applies `downsample`."""
import ctypes
import json
import math
import os
import random
import struct
from typing import NamedTuple

import numpy as np

from . import png_io, resample, synthetic

ZNEAR, ZFAR = 0.01, 100.0  # R/scene/cameras.py:54-55
DEFAULT_POINTS = 100_000
C0 = synthetic.C0


def SH2RGB(sh):
    return sh * C0 + 0.5


class CameraInfo(NamedTuple):
    uid: int
    R: np.ndarray          # (3, 3) float64, world-to-camera rotation TRANSPOSED (as the reference keeps it)
    T: np.ndarray          # (3,) float64
    FoVx: float
    FoVy: float
    image_path: str
    image_name: str
    width: int
    height: int
    fid: float
    K: np.ndarray = None   # (3, 3) float64 intrinsics of a real capture, for width x height; None: the FoVs describe the camera
    mask_path: str = None  # the segmentation mask of a real capture's frame


class PointCloud(NamedTuple):
    points: np.ndarray     # (N, 3) float32
    colors: np.ndarray     # (N, 3) in [0, 1]
    normals: np.ndarray    # (N, 3)


class SceneInfo(NamedTuple):
    point_cloud: PointCloud
    train_cameras: list
    test_cameras: list
    cameras_extent: float  # getNerfppNorm's radius
    translate: np.ndarray
    ply_path: str          # None when the default cloud was generated and not written


def world_to_view(R, T):
    """getWorld2View2 (R/utils/graphics_utils.py:42-53) without its translate / scale: (4, 4) float32."""
    Rt = np.zeros((4, 4))
    Rt[:3, :3] = np.asarray(R).T
    Rt[:3, 3] = T
    Rt[3, 3] = 1.0
    # (the reference inverts, moves the camera centre by translate / scale, and inverts back; with neither, the two inversions are kept
    # so that the matrix carries the same float64 rounding before it is cut to float32)
    return np.float32(np.linalg.inv(np.linalg.inv(Rt)))


def make_camera(info):
    """synthetic.Camera of a CameraInfo, built as R/scene/cameras.py:54-71 builds its matrices."""
    wvt = np.ascontiguousarray(world_to_view(info.R, info.T).T)
    if info.K is not None:  # (R/scene/cameras.py:64-67: getProjectionMatrix_from_K when the camera has intrinsics)
        P = synthetic.projection_matrix_from_K(ZNEAR, ZFAR, np.asarray(info.K, np.float64), info.width, info.height)
    else:
        P = synthetic.projection_matrix(ZNEAR, ZFAR, info.FoVx, info.FoVy)
    full = np.ascontiguousarray((wvt @ P.T).astype(np.float32))
    center = np.linalg.inv(wvt.astype(np.float64))[3, :3].astype(np.float32)
    return synthetic.Camera(info.width, info.height, info.FoVx, info.FoVy, wvt, full, center, float(info.fid))


def png_size(path):
    """(W, H) from a PNG's IHDR, without reading the rest of the file."""
    with open(path, "rb") as fh:
        head = fh.read(24)
    if len(head) < 24 or head[:8] != png_io.SIGNATURE or head[12:16] != b"IHDR":
        raise ValueError(f"png_size: {path}: not a PNG file")
    return struct.unpack(">II", head[16:24])


def read_cameras_from_transforms(path, transformsfile, extension=".png"):
    with open(os.path.join(path, transformsfile)) as fh:
        contents = json.load(fh)
    fovx = float(contents["camera_angle_x"])
    infos = []
    for idx, frame in enumerate(contents["frames"]):
        image_path = os.path.join(path, frame["file_path"] + extension)
        c2w = np.array(frame["transform_matrix"], np.float64)
        c2w[:3, 1:3] *= -1  # OpenGL / Blender camera axes (y up, z back) -> COLMAP (y down, z forward)
        w2c = np.linalg.inv(c2w)
        W, H = png_size(image_path)
        fovy = 2 * math.atan(math.tan(fovx / 2) * H / W)  # focal2fov(fov2focal(fovx, W), H)
        infos.append(CameraInfo(idx, np.transpose(w2c[:3, :3]), w2c[:3, 3], fovx, fovy, image_path,
                                os.path.splitext(os.path.basename(image_path))[0], int(W), int(H), float(frame["time"])))
    return infos


def nerfpp_norm(infos):
    """getNerfppNorm: (translate, radius) with radius = 1.1 x the largest distance of a camera centre from their mean."""
    centers = np.stack([np.linalg.inv(world_to_view(c.R, c.T))[:3, 3] for c in infos])
    mean = centers.mean(axis=0)
    return -mean, float(np.linalg.norm(centers - mean, axis=1).max() * 1.1)


def default_point_cloud(seed=0, n=DEFAULT_POINTS):
    """The reference's random start (dataset_readers.py:332-341) from a seeded RandomState, as it comes back from the PLY the
    reference stores it in: float32 positions in [-1.3, 1.3]^3, colours SH2RGB(rand / 255) quantised to bytes."""
    rng = np.random.RandomState(seed)
    xyz = (rng.random_sample((n, 3)) * 2.6 - 1.3).astype(np.float32)
    rgb = (SH2RGB(rng.random_sample((n, 3)) / 255.0) * 255).astype(np.uint8)
    return xyz, rgb


def store_ply(path, xyz, rgb_u8):
    """storePly: x y z nx ny nz (float), red green blue (uchar)."""
    from . import ply_io
    v = np.zeros(len(xyz), dtype=[(k, "f4") for k in ("x", "y", "z", "nx", "ny", "nz")] + [(k, "u1") for k in ("red", "green", "blue")])
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    v["red"], v["green"], v["blue"] = rgb_u8[:, 0], rgb_u8[:, 1], rgb_u8[:, 2]
    ply_io.write_ply(path, [("vertex", v)])


def fetch_ply(path):
    from . import ply_io
    v = ply_io.read_ply(path)["vertex"]
    col = lambda *ks: np.stack([np.asarray(v[k]) for k in ks], axis=1)
    names = v.dtype.names
    normals = col("nx", "ny", "nz").astype(np.float32) if "nx" in names else np.zeros((len(v), 3), np.float32)
    return PointCloud(col("x", "y", "z").astype(np.float32), col("red", "green", "blue") / 255.0, normals)


def read_blender_scene(source_path, white_background=False, eval=False, *, downsample=1.0, model_path=None, seed=0, extension=".png"):
    """SceneInfo of a Blender / D-NeRF directory.  eval=False folds the test frames into the training set.  The point cloud is
    source_path/points3d.ply when present; otherwise the seeded default cloud, written to model_path/input.ply when model_path is
    given (never into the dataset directory).  white_background only matters to the images, which Scene loads."""
    if downsample != 1.0:
        raise NotImplementedError(f"read_blender_scene: downsample={downsample} would resize the images (only 1.0 is built)")
    train = read_cameras_from_transforms(source_path, "transforms_train.json", extension)
    test = read_cameras_from_transforms(source_path, "transforms_test.json", extension)
    if not eval:
        train, test = train + test, []
    translate, radius = nerfpp_norm(train)
    ply_path = os.path.join(source_path, "points3d.ply")
    if os.path.exists(ply_path):
        pcd = fetch_ply(ply_path)
    else:
        xyz, rgb = default_point_cloud(seed)
        ply_path = None
        if model_path is not None:
            ply_path = os.path.join(model_path, "input.ply")
            store_ply(ply_path, xyz, rgb)
        pcd = PointCloud(xyz, rgb / 255.0, np.zeros_like(xyz))
    return SceneInfo(pcd, train, test, radius, translate, ply_path)


def _no_reader(name):
    def reader(*a, **k):
        raise NotImplementedError(f"dataset: the {name} reader is not built (Blender / D-NeRF scenes only)")
    return reader


# data type -> reader(source_path, white_background, eval, ...) -> SceneInfo
READERS = {"Blender": read_blender_scene, "Nerfies": _no_reader("Nerfies"), "iPhone": _no_reader("iPhone"),
           "NeuralActor": _no_reader("NeuralActor")}


def scene_type(args):
    """The key of READERS for a ModelParams-like object: its data_type, or "Blender" when transforms_train.json is there."""
    if getattr(args, "data_type", ""):
        if args.data_type not in READERS:
            raise NotImplementedError(f"dataset: unknown data_type {args.data_type!r} (known: {sorted(READERS)})")
        return args.data_type
    if os.path.exists(os.path.join(args.source_path, "transforms_train.json")):
        return "Blender"
    raise ValueError(f"dataset: {args.source_path}: could not recognise the scene type (no transforms_train.json)")


def image_ingest(pixels, background):
    """dgm_image_ingest: pixels (B, H, W, C) uint8 on the device, C 3 or 4; background: three numbers.  -> original_image
    (B, 3, H, W) fp32 = the bytes the reference composites in fp64 and truncates, over 255; gt_alpha_mask (B, H, W, 1) fp32."""
    import torch

    from . import _lib
    if not (torch.is_tensor(pixels) and pixels.is_cuda and pixels.dtype == torch.uint8 and pixels.dim() == 4 and pixels.shape[3] in (3, 4)):
        raise RuntimeError("image_ingest needs a (B, H, W, 3 or 4) uint8 CUDA/HIP tensor (dg-mesh_amd has no CPU path for its kernels)")
    pixels = pixels.contiguous()
    B, H, W, C = pixels.shape
    image = torch.empty((B, 3, H, W), dtype=torch.float32, device=pixels.device)
    mask = torch.empty((B, H, W, 1), dtype=torch.float32, device=pixels.device)
    bg = (ctypes.c_float * 3)(*[float(v) for v in background])
    with _lib.device_guard(pixels.device):
        _lib.check(_lib.lib().dgm_image_ingest(B, H, W, C, ctypes.c_void_p(pixels.data_ptr()), bg, ctypes.c_void_p(image.data_ptr()),
                                               ctypes.c_void_p(mask.data_ptr()), _lib.stream_ptr()))
    return image, mask


def image_composite_bytes(pixels, background):
    """dgm_image_composite_bytes: image_ingest's composited bytes before the division, (B, H, W, 4) uint8 = (R, G, B over the
    background, the file's alpha; 255 for three-channel files): what a `resolution` resize takes."""
    import torch

    from . import _lib
    if not (torch.is_tensor(pixels) and pixels.is_cuda and pixels.dtype == torch.uint8 and pixels.dim() == 4 and pixels.shape[3] in (3, 4)):
        raise RuntimeError("image_composite_bytes needs a (B, H, W, 3 or 4) uint8 CUDA/HIP tensor (dg-mesh_amd has no CPU path for its kernels)")
    pixels = pixels.contiguous()
    B, H, W, C = pixels.shape
    out = torch.empty((B, H, W, 4), dtype=torch.uint8, device=pixels.device)
    bg = (ctypes.c_float * 3)(*[float(v) for v in background])
    with _lib.device_guard(pixels.device):
        _lib.check(_lib.lib().dgm_image_composite_bytes(B, H, W, C, ctypes.c_void_p(pixels.data_ptr()), bg, ctypes.c_void_p(out.data_ptr()),
                                                        _lib.stream_ptr()))
    return out


def image_ingest_masked(pixels, mask, background, out="planes"):
    """dgm_image_ingest_masked: pixels (B, H, W, 3 or 4) uint8 and mask (B, H, W, 1, 3 or 4) uint8 on the device; m = mask[..., 0] > 0.
    out="planes" -> original_image (B, 3, H, W) fp32 = (m ? byte : 255 background) / 255, gt_alpha_mask (B, H, W, 1) fp32 = m.
    out="bytes"  -> (B, H, W, 4) uint8 = (R, G, B, 255 m): what a `resolution` resize takes."""
    import torch

    from . import _lib
    ok = lambda t, cs: torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 4 and t.shape[3] in cs
    if not (ok(pixels, (3, 4)) and ok(mask, (1, 3, 4))):
        raise RuntimeError("image_ingest_masked needs (B, H, W, 3 or 4) and (B, H, W, 1, 3 or 4) uint8 CUDA/HIP tensors (dg-mesh_amd has no "
                           "CPU path for its kernels)")
    if out not in ("planes", "bytes"):
        raise ValueError(f"image_ingest_masked: out must be 'planes' or 'bytes', got {out!r}")
    if pixels.shape[:3] != mask.shape[:3] or pixels.device != mask.device:
        raise ValueError(f"image_ingest_masked: pixels {tuple(pixels.shape)} and mask {tuple(mask.shape)} differ in batch, size or device")
    pixels, mask = pixels.contiguous(), mask.contiguous()
    B, H, W, C = pixels.shape
    image = alpha = res = None
    if out == "planes":
        image = torch.empty((B, 3, H, W), dtype=torch.float32, device=pixels.device)
        alpha = torch.empty((B, H, W, 1), dtype=torch.float32, device=pixels.device)
    else:
        res = torch.empty((B, H, W, 4), dtype=torch.uint8, device=pixels.device)
    bg = (ctypes.c_float * 3)(*[float(v) for v in background])
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    with _lib.device_guard(pixels.device):
        _lib.check(_lib.lib().dgm_image_ingest_masked(B, H, W, C, ptr(pixels), int(mask.shape[3]), ptr(mask), bg, 1 if res is not None else 0,
                                                      ptr(image), ptr(alpha), ptr(res), _lib.stream_ptr()))
    return (image, alpha) if res is None else res


def downsampled(info, downsample):
    """The CameraInfo after readCamerasFromTransforms' image.resize((int(W / downsample), int(H / downsample))): width, height, and
    FoVy recomputed from the resized size; FoVx stays the file's camera_angle_x."""
    w, h = resample.target_size_downsample(info.width, info.height, downsample)
    if w < 1 or h < 1:
        raise ValueError(f"Scene: downsample={downsample} leaves no pixels of {info.image_path} ({info.width} x {info.height})")
    if (w, h) == (info.width, info.height):
        return info
    return info._replace(width=w, height=h, FoVy=2 * math.atan(math.tan(info.FoVx / 2) * h / w))


def camera_to_json(uid, info):
    """camera_to_JSON (R/utils/camera_utils.py:75-95)."""
    Rt = np.zeros((4, 4))
    Rt[:3, :3] = info.R.transpose()
    Rt[:3, 3] = info.T
    Rt[3, 3] = 1.0
    C2W = np.linalg.inv(Rt)
    focal = lambda fov, pixels: pixels / (2 * math.tan(fov / 2))
    return {"id": uid, "img_name": info.image_name, "width": info.width, "height": info.height, "position": C2W[:3, 3].tolist(),
            "rotation": [row.tolist() for row in C2W[:3, :3]], "fy": focal(info.FoVy, info.height), "fx": focal(info.FoVx, info.width)}


def check_resolution(resolution, infos):
    """Names what loads without resampling: loadCam (R/utils/camera_utils.py:23-46) keeps the file's size for resolution 1, and
    for -1 up to 1600 pixels of width.  (Scene resizes for every other value and does not call this.)"""
    if resolution == 1 or (resolution == -1 and all(c.width <= 1600 for c in infos)):
        return
    raise NotImplementedError(f"Scene: resolution={resolution} would resize the images (only 1, or -1 with widths <= 1600, is built)")


class Scene:
    """R/scene/__init__.py:25-141 for the data types of READERS.  args: a ModelParams-like object (source_path, model_path,
    white_background, eval, data_type, downsample, resolution).  gaussians: a scene.GaussianModel or None."""

    def __init__(self, args, gaussians, load_iteration=None, shuffle=True, device="cuda", seed=0):
        import torch

        from . import scene as S
        self.model_path, self.gaussians, self.loaded_iter = args.model_path, gaussians, None
        if load_iteration:
            if load_iteration == -1:
                load_iteration = max(int(f.split("_")[-1]) for f in os.listdir(os.path.join(self.model_path, "point_cloud")))
            self.loaded_iter = load_iteration
        os.makedirs(self.model_path, exist_ok=True)
        from . import captures
        kind = scene_type(args)
        d = float(getattr(args, "downsample", 1.0))
        if not d > 0:
            raise ValueError(f"Scene: downsample must be positive, got {d}")
        if kind in captures.READERS:
            # the capture readers size their cameras themselves (K follows the image); only Nerfies scenes take `downsample`
            more = {"downsample": d, "nerfies_ratio": float(getattr(args, "nerfies_ratio", 0.5))} if kind == "Nerfies" else {}
            info = captures.READERS[kind](args.source_path, args.white_background, args.eval, model_path=self.model_path, seed=seed, **more)
            d = d if kind == "Nerfies" else 1.0
        else:
            info = READERS[kind](args.source_path, args.white_background, args.eval, downsample=1.0, model_path=self.model_path, seed=seed)
        if d != 1.0 and kind not in captures.READERS:  # (the reader saw the files' sizes; from here on the cameras carry the downsampled ones)
            info = info._replace(train_cameras=[downsampled(c, d) for c in info.train_cameras],
                                 test_cameras=[downsampled(c, d) for c in info.test_cameras])
        self.downsample, self.resolution = d, getattr(args, "resolution", -1)
        if not self.loaded_iter:
            if info.ply_path is not None and os.path.dirname(os.path.abspath(info.ply_path)) != os.path.abspath(self.model_path):
                with open(info.ply_path, "rb") as src, open(os.path.join(self.model_path, "input.ply"), "wb") as dst:
                    dst.write(src.read())
            cams = list(info.test_cameras) + list(info.train_cameras)
            with open(os.path.join(self.model_path, "cameras.json"), "w") as fh:
                json.dump([camera_to_json(i, c) for i, c in enumerate(cams)], fh)
        train, test = list(info.train_cameras), list(info.test_cameras)
        if shuffle:  # the reference's two random.shuffle calls after random.seed(0) (R/utils/general_utils.py:214)
            rng = random.Random(seed)
            rng.shuffle(train)
            rng.shuffle(test)
        self.cameras_extent = info.cameras_extent
        self.scene_info = info
        self.device = torch.device(device)
        background = [1.0, 1.0, 1.0] if args.white_background else [0.0, 0.0, 0.0]
        self.train_cameras = {1.0: self._load(train, background, S)}
        self.test_cameras = {1.0: self._load(test, background, S)}
        if gaussians is not None:
            if self.loaded_iter:
                gaussians.load_ply(os.path.join(self.model_path, "point_cloud", f"iteration_{self.loaded_iter}", "point_cloud.ply"),
                                   og_number_points=len(info.point_cloud.points))
            else:
                pcd = info.point_cloud
                gaussians.create_from_pcd(pcd.points, pcd.colors, pcd.normals if np.any(pcd.normals) else None)

    def _load(self, infos, background, S):
        """TorchCameras of one split; original_image / gt_alpha_mask are views into one batch per image shape.  infos carry the size
        after `downsample`; the stages are those of the module docstring."""
        if not infos:
            return []
        images, masks = [None] * len(infos), [None] * len(infos)
        capture = infos[0].mask_path is not None
        seg, per = self._load_masks(infos) if capture else (None, None)
        for idx, pixels in png_io.decode_png_groups([c.image_path for c in infos], self.device):
            w, h = resample.target_size_downsample(pixels.shape[2], pixels.shape[1], self.downsample)
            if any((infos[i].width, infos[i].height) != (w, h) for i in idx):  # (the sizes the reader took from the headers)
                raise ValueError(f"Scene: {infos[idx[0]].image_path}: size changed while loading")
            if (w, h) != (pixels.shape[2], pixels.shape[1]):
                pixels = resample.resize(pixels, (w, h), "lanczos")
            final = resample.target_size_resolution(w, h, self.resolution)
            if min(final) < 1:
                raise ValueError(f"Scene: resolution={self.resolution} leaves no pixels of a {w} x {h} image")
            if capture:
                import torch
                whole = [b for j, b in seg if j == idx]  # one mask batch for exactly these frames: taken as it is
                mk = whole[0] if whole else torch.stack([per[i][:, :, :1] for i in idx])
                if final == (w, h):
                    im, mk = image_ingest_masked(pixels, mk, background)
                else:
                    im, mk = resample.resize(image_ingest_masked(pixels, mk, background, out="bytes"), final, "bicubic", premultiplied=False,
                                             out="planes")
            elif final == (w, h):
                im, mk = image_ingest(pixels, background)
            else:
                im, mk = resample.resize(image_composite_bytes(pixels, background), final, "bicubic", premultiplied=False, out="planes")
            for k, i in enumerate(idx):
                images[i], masks[i] = im[k], mk[k]
        cams = []
        for i, c in enumerate(infos):
            fw, fh = int(images[i].shape[2]), int(images[i].shape[1])
            if c.K is not None and (fw, fh) != (c.width, c.height):  # (the intrinsics follow the image, so the frustum stays)
                c = c._replace(K=np.diag([fw / c.width, fh / c.height, 1.0]) @ np.asarray(c.K, np.float64))
            c = c._replace(width=fw, height=fh)  # (`resolution` leaves the FoVs alone)
            cam = S.TorchCamera(make_camera(c), self.device)
            cam.original_image, cam.gt_alpha_mask = images[i], masks[i]
            cam.uid, cam.image_name = i, c.image_name
            cams.append(cam)
        return cams

    def _load_masks(self, infos):
        """([(indices, (n, h, w, C) uint8 batch)], {camera index: its (h, w, C) view}) of the cameras' masks at the cameras' size:
        decoded, and under `downsample` resized as Pillow resizes them -- NEAREST for palette and bilevel files, Lanczos for grey and
        colour ones."""
        for c in infos:
            if c.mask_path is None or not os.path.exists(c.mask_path):
                raise ValueError(f"Scene: {c.image_path}: its mask {c.mask_path} is missing")
        out = []
        for idx, batch, kind in png_io.decode_mask_groups([c.mask_path for c in infos], self.device):
            W, H = int(batch.shape[2]), int(batch.shape[1])
            for i in idx:  # (the files' own sizes: two different sizes can meet after `downsample`)
                fw, fh = (int(v) for v in png_size(infos[i].image_path))
                if (fw, fh) != (W, H):
                    raise ValueError(f"Scene: the mask {infos[i].mask_path} is {W} x {H} but its frame {infos[i].image_path} is {fw} x {fh}")
            w, h = resample.target_size_downsample(W, H, self.downsample)
            if (w, h) != (W, H):
                batch = resample.resize_nearest(batch, (w, h)) if kind == "index" else resample.resize(batch, (w, h), "lanczos")
            out.append((idx, batch))
        return out, {i: b[k] for idx, b in out for k, i in enumerate(idx)}

    def save(self, iteration):
        self.gaussians.save_ply(os.path.join(self.model_path, f"point_cloud/iteration_{iteration}", "point_cloud.ply"))

    def getTrainCameras(self, scale=1.0):
        return self.train_cameras[scale]

    def getTestCameras(self, scale=1.0):
        return self.test_cameras[scale]
