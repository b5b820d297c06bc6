"""Small real-capture scenes written to a directory by the tests, one per layout captures.py reads: Nerfies, iPhone and NeuralActor.
The poses are synthetic.make_camera(K=...)'s, with an off-centre principal point, inverted into what each layout stores --
`orientation` / `position` (recentred and scaled back for Nerfies, focal length and principal point divided by the ratio) or
NeuralActor's OpenCV camera-to-world `transform_matrix` and `intrinsic`.  48 x 40 frames, 5 train + 2 val; frame 1 is RGBA, the
others RGB (tests/_scene_fixture.py's shaded disc, encoded by tests/_png_ref.py); the masks are the Pillow-written files of
tests/golden/capture_small.npz, a different PNG flavour per frame; a points.npy."""
import json
import os

import numpy as np

import _png_ref
import _scene_fixture

W, H = 48, 40
N_TRAIN, N_VAL = 5, 2
RATIO = 0.5                        # nerfies_ratio: the frames live under rgb/2x
CENTER, SCALE = [0.3, -0.2, 0.1], 0.25  # scene.json of the Nerfies scene
K_SQUARE = np.array([[60.0, 0.0, W / 2 + 3.5], [0.0, 60.0, H / 2 - 2.25], [0.0, 0.0, 1.0]])  # one focal length: Nerfies, iPhone
K_ACTOR = np.array([[62.0, 0.0, W / 2 - 4.0], [0.0, 58.0, H / 2 + 1.5], [0.0, 0.0, 1.0]])
FLAVOURS = {"Nerfies": ["1", "L", "P3", "P16", "Pbits1", "RGB", "RGBA"], "iPhone": ["P256", "P3", "1", "RGB", "L", "RGBA", "Pbits1"],
            "NeuralActor": ["RGB", "RGBA", "RGBA", "RGB", "RGB", "RGBA", "RGB"]}
TIME_IDS = [0, 3, 4, 7, 10, 2, 8]  # train ids first, then val ids; the largest divides them all


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capture_small.npz"))


def cameras(syn, K, fids):
    return [syn.make_camera(W, H, azimuth=0.9 * k + 0.2, elevation=0.25 + 0.05 * (k % 3), fid=fid, K=K) for k, fid in enumerate(fids)]


def points(n=600):
    return _scene_fixture.ball_points(n)[0].astype(np.float64)


def _frame_file(path, k):
    px = _scene_fixture.frame_pixels(W, H, k, channels=4 if k == 1 else 3)
    types = np.random.RandomState(k).randint(0, 5, H)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(_png_ref.encode_png(px, types, idat_split=1 + k % 3))
    return px


def _mask_file(path, gold, flavour):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(gold[f"scene/{flavour}/png"].tobytes())


def _items(cams, frames, kind):
    """[{camera, frame pixels, mask flavour, split}] in the order the reader returns its cameras."""
    return [dict(cam=c, frame=f, flavour=FLAVOURS[kind][k], split="train" if k < N_TRAIN else "test")
            for k, (c, f) in enumerate(zip(cams, frames))]


def write_nerfies_like(root, syn, kind, time_key="time_id"):
    """kind "Nerfies": scene.json, ratio 0.5, positions stored before recentring; "iPhone": 1x, positions as they are."""
    gold = golden()
    nerfies = kind == "Nerfies"
    ratio, level = (RATIO, "2x") if nerfies else (1.0, "1x")
    fids = [t / max(TIME_IDS) for t in TIME_IDS]
    cams = cameras(syn, K_SQUARE, fids)
    names = [f"frame_{k:03d}" for k in range(N_TRAIN + N_VAL)]
    os.makedirs(os.path.join(root, "camera"), exist_ok=True)
    frames = []
    for k, (cam, name) in enumerate(zip(cams, names)):
        w2c = cam.world_view_transform.T.astype(np.float64)
        position = -np.linalg.inv(w2c[:3, :3]) @ w2c[:3, 3]
        if nerfies:
            position = position / SCALE + np.array(CENTER)
        with open(os.path.join(root, "camera", name + ".json"), "w") as fh:
            json.dump({"orientation": w2c[:3, :3].tolist(), "position": position.tolist(), "focal_length": K_SQUARE[0, 0] / ratio,
                       "principal_point": (K_SQUARE[:2, 2] / ratio).tolist(), "skew": 0.0, "pixel_aspect_ratio": 1.0,
                       "radial_distortion": [0.0, 0.0, 0.0], "tangential_distortion": [0.0, 0.0],
                       "image_size": [int(W / ratio), int(H / ratio)]}, fh)
        frames.append(_frame_file(os.path.join(root, "rgb", level, name + ".png"), k))
        _mask_file(os.path.join(root, "mask-tracking", level, "Annotations", name + ".png"), gold, FLAVOURS[kind][k])
    with open(os.path.join(root, "metadata.json"), "w") as fh:
        json.dump({n: {time_key: t, "camera_id": 0} for n, t in zip(names, TIME_IDS)}, fh)
    with open(os.path.join(root, "dataset.json"), "w") as fh:
        json.dump({"count": len(names), "ids": names, "train_ids": names[:N_TRAIN], "val_ids": names[N_TRAIN:]}, fh)
    pts = points()
    if nerfies:
        with open(os.path.join(root, "scene.json"), "w") as fh:
            json.dump({"scale": SCALE, "center": CENTER, "near": 0.1, "far": 10.0}, fh)
        np.save(os.path.join(root, "points.npy"), pts / SCALE + np.array(CENTER))
    else:
        np.save(os.path.join(root, "points.npy"), pts)
    return _items(cams, frames, kind)


def write_neural_actor(root, syn):
    gold = golden()
    fids = [k / 10.0 for k in range(N_TRAIN + N_VAL)]
    cams = cameras(syn, K_ACTOR, fids)
    frames, lists = [], {"train": [], "test": []}
    for k, cam in enumerate(cams):
        split, folder = ("train", "training") if k < N_TRAIN else ("test", "testing")
        rel = f"{folder}/{k:06d}.png"
        frames.append(_frame_file(os.path.join(root, rel), k))
        _mask_file(os.path.join(root, f"{folder}_mask", "Annotations", f"{k:06d}.png"), gold, FLAVOURS["NeuralActor"][k])
        lists[split].append({"file_path": rel, "time": cam.fid, "intrinsic": K_ACTOR.tolist(),
                             "transform_matrix": np.linalg.inv(cam.world_view_transform.T.astype(np.float64)).tolist()})
    for split, fr in lists.items():
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as fh:
            json.dump({"frames": fr}, fh)
    return _items(cams, frames, "NeuralActor")


def write_scene(root, syn, kind):
    os.makedirs(root, exist_ok=True)
    if kind == "NeuralActor":
        return write_neural_actor(root, syn)
    return write_nerfies_like(root, syn, kind, time_key="time_id" if kind == "Nerfies" else "warp_id")


def listing(root):
    """Every file under root with its size and modification time: what a reader must leave alone."""
    return sorted((os.path.relpath(os.path.join(d, f), root), os.path.getsize(os.path.join(d, f)), os.path.getmtime(os.path.join(d, f)))
                  for d, _, fs in os.walk(root) for f in fs)
