"""Test-side restatement, in numpy, of what the reference does with a real capture: the camera maths of readNerfiesCameras,
readiPhoneCameras and readNeuralActorCameras (dgmesh/scene/dataset_readers.py:545-865) with camera_nerfies_from_JSON
(dgmesh/utils/camera_utils.py:98-118), the matrices a Camera makes of them (dgmesh/scene/cameras.py:54-71, getWorld2View2 and
getProjectionMatrix_from_K of dgmesh/utils/graphics_utils.py), and the masked composite.  Independent of captures.py and dataset.py."""
import math

import numpy as np

ZNEAR, ZFAR = 0.01, 100.0


def nerfies_pose(camera_json, ratio, center=None, scale=None):
    """-> (R, T, K): R = orientation.T, T = -position @ R with the position recentred and scaled first (Nerfies only); one focal
    length and the principal point, both times `ratio`."""
    orientation = np.array(camera_json["orientation"])
    position = np.array(camera_json["position"])
    if center is not None:
        position = position - np.array(center)
        position = position * scale
    focal = camera_json["focal_length"] * ratio
    pp = np.array(camera_json["principal_point"]) * ratio
    R = orientation.T
    T = -position @ R
    return R, T, np.array([[focal, 0, pp[0]], [0, focal, pp[1]], [0, 0, 1]])


def neural_actor_pose(frame):
    c2w = np.array(frame["transform_matrix"])
    w2c = np.linalg.inv(c2w)
    return np.transpose(w2c[:3, :3]), w2c[:3, 3], np.array(frame["intrinsic"])


def focal2fov(focal, pixels):
    return 2 * math.atan(pixels / (2 * focal))


def camera_matrices(R, T, K, W, H):
    """(world_view_transform, full_proj_transform, camera_center) as float32, transposed as the reference keeps them."""
    Rt = np.zeros((4, 4))
    Rt[:3, :3] = R.transpose()
    Rt[:3, 3] = T
    Rt[3, 3] = 1.0
    wvt = np.float32(Rt).T
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    top, bottom = ZNEAR * cy / fy, -ZNEAR * (H - cy) / fy
    right, left = ZNEAR * (W - cx) / fx, -ZNEAR * cx / fx
    P = np.zeros((4, 4), np.float32)
    P[0, 0] = 2.0 * ZNEAR / (right - left)
    P[1, 1] = 2.0 * ZNEAR / (top - bottom)
    P[0, 2] = -(right + left) / (right - left)
    P[1, 2] = (top + bottom) / (top - bottom)
    P[3, 2] = 1.0
    P[2, 2] = ZFAR / (ZFAR - ZNEAR)
    P[2, 3] = -(ZFAR * ZNEAR) / (ZFAR - ZNEAR)
    full = (wvt @ P.T).astype(np.float32)
    return wvt, full, np.linalg.inv(wvt.astype(np.float64))[3, :3].astype(np.float32)


def mask_of(mask_pixels):
    """np.array(Image.open(mask)) -> bool (H, W): the first channel of a colour file (DEVA), the plane itself otherwise (SAM)."""
    m = np.asarray(mask_pixels)
    return m[..., 0] > 0 if m.ndim == 3 else m > 0


def composite_bytes(frame, mask, white_background):
    """readNerfiesCameras / readiPhoneCameras: image[~mask] = 255 or 0 -> (H, W, 3) uint8 (a frame's own alpha is dropped, as
    PILtoTorch's caller takes [:3]), and the bool mask."""
    m = mask if mask.dtype == bool and mask.ndim == 2 else mask_of(mask)
    image = np.array(frame[..., :3], copy=True)
    image[~m] = 255.0 if white_background else 0.0
    return image.astype(np.uint8), m


def composite_bytes_neural_actor(frame, mask, white_background):
    """readNeuralActorCameras: arr = im / 255.0; arr[~mask] = bg; bytes of arr * 255.0, truncated."""
    m = mask if mask.dtype == bool and mask.ndim == 2 else mask_of(mask)
    arr = frame[..., :3] / 255.0
    arr[~m] = np.array([1, 1, 1]) if white_background else np.array([0, 0, 0])
    return np.array(arr * 255.0, dtype=np.byte).view(np.uint8), m


def planes(image_bytes, m):
    """PILtoTorch's byte / 255 in float32 as (3, H, W); the mask as (H, W, 1) float32."""
    image = image_bytes.astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray(image.transpose(2, 0, 1)), m[..., None].astype(np.float32)


def ingest_masked(frame, mask, white_background):
    return planes(*composite_bytes(frame, mask, white_background))


def ingest_masked_bytes(frame, mask, white_background):
    """(H, W, 4) uint8 = (R, G, B, 255 m): what a `resolution` resize takes."""
    image, m = composite_bytes(frame, mask, white_background)
    return np.concatenate([image, (m[..., None] * 255).astype(np.uint8)], axis=2)


def extent(centers):
    """getNerfppNorm's radius: 1.1 x the largest distance of a camera centre from their mean."""
    c = np.asarray(centers, np.float64)
    return float(np.linalg.norm(c - c.mean(axis=0), axis=1).max() * 1.1)
