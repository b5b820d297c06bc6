"""Real captures on disk -- Nerfies / HyperNeRF, iPhone (DyCheck) and NeuralActor scenes -- as the cameras and point cloud that
dataset.Scene loads: the front end of the reference's `configs/nerfies`, `configs/iphone` and `configs/neural-actor`.

  read_nerfies_scene       <- readNerfiesCameras / readNerfiesInfo (R/scene/dataset_readers.py:545-677)
  read_iphone_scene        <- readiPhoneCameras / readiPhoneInfo (:680-800)
  read_neural_actor_scene  <- readNeuralActorCameras / readNeuralActorInfo (:803-905)
  nerfies_camera           <- camera_nerfies_from_JSON (R/utils/camera_utils.py:98-118)
(R/ = dgmesh/.)  The readers read JSON and PNG headers only.  Every camera carries its intrinsic matrix K, from which
dataset.make_camera builds the off-centre projection (getProjectionMatrix_from_K), and the path of its segmentation mask; Scene
decodes frames and masks on the device and composites "frame where the mask's first channel is set, background elsewhere"
(dataset.image_ingest_masked).  NeuralActor's (v / 255.0) * 255.0 round trip truncates back to v for every byte, so the three layouts
share that one kernel.

Layouts.  Nerfies: scene.json (scale, center), metadata.json (time_id or warp_id per frame), dataset.json (train_ids, val_ids),
camera/<id>.json, rgb/<1/ratio>x/<id>.png, mask-tracking/<1/ratio>x/Annotations/<id>.png; positions are recentred and scaled,
focal length and principal point multiplied by nerfies_ratio.  iPhone: the same files at 1x, no scene.json, warp_id only.
NeuralActor: transforms_{train,test}.json whose frames give file_path (with its extension), time, an OpenCV camera-to-world
transform_matrix and an `intrinsic` matrix; the mask of .../training/... is .../training_mask/Annotations/..., likewise testing;
at most the first 1500 frames of a file are read.

The point cloud is source_path/points3d.ply when present; otherwise points.npy (recentred and scaled for Nerfies), or for
NeuralActor 100 000 seeded points in [-1, 1]^3, with seeded colours as dataset.default_point_cloud draws them, written to
model_path/input.ply when model_path is given -- never into the dataset directory, where the reference writes it.

Deviations from the reference:
  (a) under Nerfies `downsample` the reference keeps the undivided focal length against the smaller image, so its field of view is
      wrong; here fx and cx scale by w' / w and fy and cy by h' / h.
  (b) under `resolution` the reference resizes the image and leaves the mask at its old size; here the mask is resized with the
      image, as for Blender scenes (dataset.py).
  (c) orig_img, the unmasked frame that only the reference's render_test uses for NeuralActor, is not kept.
iPhone and NeuralActor scenes ignore `downsample`, as the reference's readers for them are called without it."""
import json
import math
import os
import struct

import numpy as np

from . import png_io
from .dataset import CameraInfo, PointCloud, SceneInfo, SH2RGB, fetch_ply, nerfpp_norm, store_ply

NEURAL_ACTOR_FRAMES = 1500  # load_num
NEURAL_ACTOR_POINTS = 100_000


def png_header(path):
    """(W, H, bit depth, colour type) from a PNG's IHDR, without reading the rest of the file."""
    with open(path, "rb") as fh:
        head = fh.read(26)
    if len(head) < 26 or head[:8] != png_io.SIGNATURE or head[12:16] != b"IHDR":
        raise ValueError(f"captures: {path}: not a PNG file")
    return struct.unpack(">IIBB", head[16:26])


def focal2fov(focal, pixels):
    return 2 * math.atan(pixels / (2 * focal))


def _json(path):
    with open(path) as fh:
        return json.load(fh)


def nerfies_camera(path, scale):
    """camera_nerfies_from_JSON, the fields the readers use."""
    c = _json(path)
    return {"orientation": np.array(c["orientation"], np.float64), "position": np.array(c["position"], np.float64),
            "focal_length": c["focal_length"] * scale, "principal_point": np.array(c["principal_point"], np.float64) * scale}


def _frame_size(image_path, mask_path):
    if not os.path.exists(image_path):
        raise ValueError(f"captures: the frame {image_path} is missing")
    if not os.path.exists(mask_path):
        raise ValueError(f"captures: {image_path}: its mask {mask_path} is missing")
    W, H = png_header(image_path)[:2]
    return int(W), int(H)


def _nerfies_cameras(path, ratio, time_keys, center, scale, downsample):
    """The cameras of a Nerfies-layout directory, train ids first, then val ids; -> (infos, number of train ids)."""
    meta, ids = _json(os.path.join(path, "metadata.json")), _json(os.path.join(path, "dataset.json"))
    train_ids, all_ids = list(ids["train_ids"]), list(ids["train_ids"]) + list(ids["val_ids"])
    key = next((k for k in time_keys if k in meta[all_ids[0]]), None)
    if key is None:
        raise ValueError(f"captures: {path}/metadata.json: no {' or '.join(time_keys)} for frame {all_ids[0]}")
    times = [meta[i][key] for i in all_ids]
    max_time = max(times)
    level = f"{int(1 / ratio)}x"
    infos = []
    for idx, name in enumerate(all_ids):
        cam = nerfies_camera(os.path.join(path, "camera", f"{name}.json"), ratio)
        position = cam["position"]
        if center is not None:
            position = (position - center) * scale
        R = cam["orientation"].T
        T = -position @ R
        image_path = f"{path}/rgb/{level}/{name}.png"
        mask_path = f"{path}/mask-tracking/{level}/Annotations/{name}.png"
        W, H = _frame_size(image_path, mask_path)
        fx = fy = float(cam["focal_length"])
        cx, cy = (float(v) for v in cam["principal_point"])
        if downsample != 1.0:  # (deviation (a): the intrinsics follow the resized image)
            w, h = int(W / downsample), int(H / downsample)
            if w < 1 or h < 1:
                raise ValueError(f"captures: downsample={downsample} leaves no pixels of {image_path} ({W} x {H})")
            fx, cx, fy, cy = fx * w / W, cx * w / W, fy * h / H, cy * h / H
            W, H = w, h
        K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
        infos.append(CameraInfo(idx, R, T, focal2fov(fx, W), focal2fov(fy, H), image_path, os.path.splitext(os.path.basename(image_path))[0],
                                W, H, times[idx] / max_time, K, mask_path))
    return infos, len(train_ids)


def _point_cloud(path, model_path, seed, make_xyz):
    """points3d.ply when the dataset has one; otherwise make_xyz(rng)'s points with seeded colours, stored as the reference's storePly
    stores them (float32 positions, byte colours) -- under model_path, or not at all."""
    ply_path = os.path.join(path, "points3d.ply")
    if os.path.exists(ply_path):
        return fetch_ply(ply_path), ply_path
    rng = np.random.RandomState(seed)
    xyz = np.asarray(make_xyz(rng), np.float64).astype(np.float32)
    rgb = (SH2RGB(rng.random_sample((len(xyz), 3)) / 255.0) * 255).astype(np.uint8)
    ply_path = None
    if model_path is not None:
        ply_path = os.path.join(model_path, "input.ply")
        store_ply(ply_path, xyz, rgb)
    return PointCloud(xyz, rgb / 255.0, np.zeros_like(xyz)), ply_path


def _scene_info(train, test, eval, pcd, ply_path):
    if not eval:
        train, test = train + test, []
    translate, radius = nerfpp_norm(train)
    return SceneInfo(pcd, train, test, radius, translate, ply_path)


def _points_npy(path):
    file = os.path.join(path, "points.npy")
    if not os.path.exists(file):
        raise ValueError(f"captures: {path} has neither points3d.ply nor points.npy")
    return np.load(file)


def read_nerfies_scene(source_path, white_background=False, eval=False, *, downsample=1.0, nerfies_ratio=0.5, model_path=None, seed=0):
    """SceneInfo of a Nerfies / HyperNeRF directory.  eval=True: the val ids are the test set; otherwise they train too.
    white_background only matters to the images, which Scene loads."""
    scene = _json(os.path.join(source_path, "scene.json"))
    center, scale = np.array(scene["center"], np.float64), float(scene["scale"])
    infos, n_train = _nerfies_cameras(source_path, float(nerfies_ratio), ("time_id", "warp_id"), center, scale, float(downsample))
    pcd, ply_path = _point_cloud(source_path, model_path, seed, lambda rng: (_points_npy(source_path) - center) * scale)
    return _scene_info(infos[:n_train], infos[n_train:], eval, pcd, ply_path)


def read_iphone_scene(source_path, white_background=False, eval=False, *, model_path=None, seed=0):
    """SceneInfo of an iPhone (DyCheck) directory: the Nerfies layout at 1x, positions as they are, times from warp_id."""
    infos, n_train = _nerfies_cameras(source_path, 1.0, ("warp_id",), None, None, 1.0)
    pcd, ply_path = _point_cloud(source_path, model_path, seed, lambda rng: _points_npy(source_path))
    return _scene_info(infos[:n_train], infos[n_train:], eval, pcd, ply_path)


def _neural_actor_cameras(path, transformsfile):
    split = "training" if transformsfile == "transforms_train.json" else "testing"
    infos = []
    for idx, frame in enumerate(_json(os.path.join(path, transformsfile))["frames"][:NEURAL_ACTOR_FRAMES]):
        w2c = np.linalg.inv(np.array(frame["transform_matrix"], np.float64))  # (OpenCV axes already: no y / z flip)
        image_path = os.path.join(path, frame["file_path"])
        mask_path = image_path.replace(f"/{split}/", f"/{split}_mask/Annotations/")
        W, H = _frame_size(image_path, mask_path)
        if png_header(mask_path)[3] not in (2, 6):
            raise ValueError(f"captures: {image_path}: its mask {mask_path} must have three or four channels (its first one is read)")
        K = np.array(frame["intrinsic"], np.float64)[:3, :3]
        infos.append(CameraInfo(idx, np.transpose(w2c[:3, :3]), w2c[:3, 3], focal2fov(K[0, 0], W), focal2fov(K[1, 1], H), image_path,
                                os.path.splitext(os.path.basename(image_path))[0], W, H, float(frame["time"]), K, mask_path))
    return infos


def read_neural_actor_scene(source_path, white_background=False, eval=False, *, model_path=None, seed=0):
    """SceneInfo of a NeuralActor directory.  eval=False folds the test frames into the training set."""
    train = _neural_actor_cameras(source_path, "transforms_train.json")
    test = _neural_actor_cameras(source_path, "transforms_test.json")
    pcd, ply_path = _point_cloud(source_path, model_path, seed, lambda rng: rng.random_sample((NEURAL_ACTOR_POINTS, 3)) * 2.0 - 1.0)
    return _scene_info(train, test, eval, pcd, ply_path)


# data type -> reader(source_path, white_background, eval, ...) -> SceneInfo
READERS = {"Nerfies": read_nerfies_scene, "iPhone": read_iphone_scene, "NeuralActor": read_neural_actor_scene}
