"""Test-side restatement of how the reference turns a frame's bytes into the tensors it trains on: readCamerasFromTransforms
(dgmesh/scene/dataset_readers.py:291-302) composites in float64 and truncates to a byte, PILtoTorch (dgmesh/utils/general_utils.py:23-29)
divides that byte by 255 in float32."""
import numpy as np


def ingest(pixels, white_background):
    """pixels (H, W, 3 or 4) uint8 -> original_image (3, H, W) float32, gt_alpha_mask (H, W, 1) float32."""
    im_data = np.asarray(pixels)
    if im_data.shape[2] == 3:  # image.convert("RGBA")
        im_data = np.concatenate([im_data, np.full(im_data.shape[:2] + (1,), 255, np.uint8)], axis=2)
    bg = np.array([1, 1, 1]) if white_background else np.array([0, 0, 0])
    norm_data = im_data / 255.0
    alpha_mask = norm_data[..., 3:4]
    arr = norm_data[:, :, :3] * norm_data[:, :, 3:4] + bg * (1 - norm_data[:, :, 3:4])
    q = np.trunc(arr * 255.0).astype(np.int64).astype(np.uint8)
    image = q.astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray(image.transpose(2, 0, 1)), alpha_mask.astype(np.float32)
