"""Training a scene on disk: training() of R/train.py:50-557 (R/ = dgmesh/) and its command line,

    python -m dgmesh_amd.train --config configs/d-nerf/jumpingjacks.yaml [--key value ...]

The schedule -- warm-up, dynamic Gaussians, normal_initialization at dpsr_iter, mesh co-training, anchoring, densification -- lives
in trainer.Trainer.step; this driver reads the configuration, builds the Scene (dataset.py), the networks and the MeshPhase, runs
the loop, logs the losses without a per-step host wait, writes checkpoints and scores the test views at the end (evaluate.testing).

Configuration: the defaults of ModelParams (below), scene.OptimizationParams, scene.PipelineParams and DRIVER_DEFAULTS; a flat YAML
file over them; `--key value` command-line overrides over that.  An unknown key is an error that lists every unknown key; the keys
of IGNORED_KEYS, which the reference defines and this project has no use for, are dropped with one log line; the reference's
gaussian_center is read as the driver's dpsr_center (TRANSLATED_KEYS).  The merged dict is written to model_path/cfg_args.txt.

Scenes: Blender / D-NeRF directories, and with data_type Nerfies, iPhone or NeuralActor the real captures of captures.py.

LPIPS of the test views (--lpips_alex FILE, --lpips_vgg FILE): weight files in any layout lpips.py reads; the project ships none.
With either, testing() also reports LPIPS_A / LPIPS_V; without, the run is what it was.

Resuming (--start_checkpoint DIR): the Gaussians and every network of the latest iteration found in DIR are loaded and the loop
continues with the iteration after it, so every schedule that is a function of the iteration number picks up where it was.
Optimiser state is not saved, as in the reference, and the order in which frames are drawn starts over (Trainer.step_count counts
the steps of this run: the resumed run replays the first epoch's shuffle instead of continuing the interrupted one).  One GPU: Trainer keeps rank / world, the driver passes 0 / 1."""
import json
import os
import sys

from . import scene as S


class ModelParams:
    """R/arguments/__init__.py:50-92, the fields this project reads, plus dpsr_sig (an optimisation field there)."""
    sh_degree = 3
    source_path = ""
    model_path = ""
    white_background = False
    eval = False
    is_blender = False
    is_6dof = False
    data_type = ""
    downsample = 1.0
    nerfies_ratio = 0.5
    resolution = -1
    prune_threshold = 0.005
    laplacian_loss_weight = 1.0
    # DPSR
    grid_res = 256
    dpsr_sig = 0.5
    gaussian_ratio = 1.5


# the driver's own switches (R/train.py:858-886 argparse flags)
DRIVER_DEFAULTS = {"config": None, "start_checkpoint": None, "log_every": 1000, "save_iterations": None, "checkpoint_iterations": None,
                   "seed": 0, "quiet": False, "lpips_alex": None, "lpips_vgg": None, "dpsr_center": None}
# the reference's gaussian_center is read under the driver's own name: only real captures -- iPhone, NeuralActor -- place the DPSR cube
# by it (R/scene/gaussian_model_dpsr_dynamic_anchor.py:686-689); the other data types measure their Gaussians and never look at it
TRANSLATED_KEYS = {"gaussian_center": ("dpsr_center", "the DPSR cube's centre for iPhone / NeuralActor captures")}
# defined by the reference's parameter groups or command line, unused here
IGNORED_KEYS = ("expname", "images", "data_device", "data_mask", "load2gpu_on_the_fly", "save_wis3d",
                "pretrain_mesh_path", "pretrain_mesh_path_test", "pretrained_type", "first_iter", "ip", "port", "detect_anomaly",
                "test_iterations")
PARAM_CLASSES = (ModelParams, S.OptimizationParams, S.PipelineParams)


def _fields(cls):
    return {k: v for k, v in vars(cls).items() if not k.startswith("_") and not callable(v)}


def default_config():
    cfg = dict(DRIVER_DEFAULTS)
    for cls in PARAM_CLASSES:
        cfg.update(_fields(cls))
    return cfg


def merge_config(*layers, log=print):
    """default_config() with each dict of `layers` merged over it in turn.  ValueError listing every unknown key."""
    cfg = default_config()
    unknown, ignored, translated = [], [], []
    for layer in layers:
        for k, v in (layer or {}).items():
            if k in TRANSLATED_KEYS:
                k = TRANSLATED_KEYS[k][0]
                translated.append(k)
            if k in cfg:
                cfg[k] = v
            elif k in IGNORED_KEYS:
                ignored.append(k)
            else:
                unknown.append(k)
    for k in PATH_KEYS:
        if cfg[k] is not None and not isinstance(cfg[k], str):
            raise ValueError(f"{k}: expected a path, got {cfg[k]!r}")
    for k in LIST_KEYS:
        if cfg[k] is not None:
            cfg[k] = iteration_list(k, cfg[k])
    if cfg["dpsr_center"] is not None:
        cfg["dpsr_center"] = center_triple("dpsr_center", cfg["dpsr_center"])
    if unknown:
        raise ValueError(f"unknown configuration key(s): {', '.join(sorted(set(unknown)))}")
    for old, (new, why) in TRANSLATED_KEYS.items():
        if new in translated:
            log(f"[config] {old} -> {new} ({why})")
    if ignored:
        log(f"[config] ignored (defined by the reference, unused here): {', '.join(sorted(set(ignored)))}")
    return cfg


def load_yaml(path):
    import yaml
    with open(path) as fh:
        data = yaml.safe_load(fh) or {}
    if not isinstance(data, dict) or any(isinstance(v, dict) for v in data.values()):
        raise ValueError(f"{path}: a flat mapping of keys to values is expected")
    return data


PATH_KEYS = ("config", "start_checkpoint", "lpips_alex", "lpips_vgg")  # None by default, strings when given
LIST_KEYS = ("save_iterations", "checkpoint_iterations")      # None by default, lists of iterations when given


def iteration_list(key, value):
    """A LIST_KEYS value from a file or the command line as a sorted list of ints; a single number is a list of one."""
    items = value if isinstance(value, (list, tuple)) else [value]
    if not all(isinstance(i, int) and not isinstance(i, bool) for i in items):
        raise ValueError(f"{key}: expected an iteration number or a list of them, got {value!r}")
    return sorted(set(items))


def center_triple(key, value):
    """Three finite numbers as a list of floats."""
    ok = isinstance(value, (list, tuple)) and len(value) == 3 and all(
        isinstance(v, (int, float)) and not isinstance(v, bool) and v == v and abs(v) != float("inf") for v in value)
    if not ok:
        raise ValueError(f"{key}: expected three numbers [x, y, z], got {value!r}")
    return [float(v) for v in value]


def _coerce(key, text, default):
    """A command-line string as the type of the key's default (None defaults: YAML's own reading of the string)."""
    import yaml
    if isinstance(default, str) or key in PATH_KEYS:
        return text
    value = yaml.safe_load(text)
    if key in LIST_KEYS:
        return iteration_list(key, value)
    if key == "dpsr_center":
        return center_triple(key, value)
    if isinstance(value, str) and isinstance(default, (int, float)) and not isinstance(default, bool):
        try:  # (YAML 1.1 reads 1e-4 as a string)
            value = float(text)
        except ValueError:
            raise ValueError(f"--{key}: expected a number, got {text!r}") from None
    if isinstance(default, bool):
        if not isinstance(value, bool):
            raise ValueError(f"--{key}: expected true or false, got {text!r}")
        return value
    if isinstance(default, float) and isinstance(value, int) and not isinstance(value, bool):
        return float(value)
    if isinstance(default, int) and not isinstance(default, bool) and isinstance(value, float) and value == int(value):
        return int(value)
    return value


def parse_overrides(argv):
    """['--key', 'value', '--flag', ...] -> dict; a key without a value is True; values are typed like the key's default."""
    defaults, out, i = default_config(), {}, 0
    while i < len(argv):
        a = argv[i]
        if not a.startswith("--") or len(a) < 3:
            raise ValueError(f"expected --key, got {a!r}")
        if "=" in a:
            key, text = a[2:].split("=", 1)
            i += 1
        elif i + 1 < len(argv) and not argv[i + 1].startswith("--"):
            key, text = a[2:], argv[i + 1]
            i += 2
        else:
            key, text = a[2:], "true"
            i += 1
        out[key] = _coerce(key, text, defaults.get(key))
    return out


def config_from_argv(argv, log=print):
    over = parse_overrides(argv)
    path = over.get("config")
    return merge_config(load_yaml(path) if path else {}, over, log=log)


def split_config(cfg):
    """-> (ModelParams, OptimizationParams, PipelineParams) objects carrying the merged values as instance attributes."""
    out = []
    for cls in PARAM_CLASSES:
        obj = cls()
        for k in _fields(cls):
            setattr(obj, k, cfg[k])
        out.append(obj)
    return tuple(out)


def latest_iteration(model_path, sub="point_cloud"):
    """searchForMaxIteration (R/utils/system_utils.py:29-31)."""
    return max(int(f.split("_")[-1]) for f in os.listdir(os.path.join(model_path, sub)))


def _loss_logging_trainer():
    from .trainer import Trainer

    class LoggingTrainer(Trainer):
        """Trainer that keeps the latest iteration's loss terms (detached device scalars) for the driver's log."""

        def loss_terms(self, cam, iteration):
            losses, pkg = super().loss_terms(cam, iteration)
            self.last_losses = {k: v.detach() for k, v in losses.items()}
            return losses, pkg

    return LoggingTrainer


def mesh_phase_options(lp, op, seed=0, center=None):
    """The MeshPhase arguments the driver derives from the configuration (the networks, the DPSR module and the device aside).
    real: the reference places the DPSR cube by gaussian_ratio / gaussian_center alone only for the iPhone and NeuralActor data types
    (R/scene/gaussian_model_dpsr_dynamic_anchor.py:686-689) and measures the deformed Gaussians for every other one, whatever
    is_blender says.  center: the configuration's dpsr_center, the cube's centre for those two (None: the origin)."""
    return dict(seed=seed, mesh_source="diffmc", mesh_losses="render", laplacian_loss_weight=lp.laplacian_loss_weight,
                anchor=op.use_anchor > 0, normal_init=True, gaussian_ratio=lp.gaussian_ratio,
                real=getattr(lp, "data_type", "") in ("iPhone", "NeuralActor"), gaussian_center=center)


LOG_COLUMNS = ("loss", "img_loss", "cycle_loss", "mask_loss", "mesh_img_loss", "laplacian_loss", "anchor_loss")


def training(cfg, *, gaussians=None, networks=None, log=print):
    """Train with the merged configuration dict `cfg` (merge_config / config_from_argv).

    gaussians: a prepared scene.GaussianModel to start from instead of the scene's point cloud; networks: prepared (deform,
    deform_back) position networks instead of fresh ones.  The MeshPhase has normal_init=True, anchor=use_anchor > 0, the rendered
    mask / mesh-image losses and a DPSR at grid_res, and exists only when dpsr_iter < iterations.

    -> dict: `log` {iteration: {column: value}} for every iteration (read back every log_every steps), `trainer`, `scene`,
    `gaussians`, `networks` {model_name: model}, `mesh`, `first_iter`, `saved` (iterations written), `test` (evaluate.testing's
    result, or None without test cameras)."""
    import torch

    from . import deform as D
    from . import dpsr as DP
    from .trainer import MeshPhase
    lp, op, pp = split_config(cfg)
    if not lp.model_path:
        raise ValueError("training: model_path is not set")
    dev = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(lp.model_path, exist_ok=True)
    with open(os.path.join(lp.model_path, "cfg_args.txt"), "w") as fh:
        json.dump(cfg, fh, indent=1, sort_keys=True)
    seed = int(cfg["seed"])
    torch.manual_seed(seed)
    start, first_iter = cfg["start_checkpoint"], 0
    if start:
        first_iter = latest_iteration(start)
    given = gaussians is not None
    if not given:
        gaussians = S.GaussianModel(sh_degree=lp.sh_degree, device=dev)
    from .dataset import Scene
    scene = Scene(lp, None if (given or start) else gaussians, device=dev, seed=seed)
    cameras, extent = scene.getTrainCameras(), scene.cameras_extent
    scene.gaussians = gaussians
    impl = "hip"
    if networks is None:
        networks = (D.DeformModelNormal(is_blender=lp.is_blender, is_6dof=lp.is_6dof, model_name="deform", device=dev, trunk_impl=impl),
                    D.DeformModelNormal(is_blender=lp.is_blender, is_6dof=lp.is_6dof, model_name="deform_back", device=dev, trunk_impl=impl))
    deform, deform_back = networks
    mesh = None
    if op.dpsr_iter < op.iterations:
        mesh = MeshPhase(D.DeformModelNormalSep(is_blender=lp.is_blender, is_6dof=lp.is_6dof, model_name="deform_normal", device=dev, trunk_impl=impl),
                         D.DeformModelNormalSep(is_blender=lp.is_blender, is_6dof=lp.is_6dof, model_name="deform_back_normal", device=dev,
                                                trunk_impl=impl),
                         D.AppearanceModel(is_blender=lp.is_blender, device=dev, trunk_impl=impl),
                         dpsr=DP.DPSR(res=(int(lp.grid_res),) * 3, sig=lp.dpsr_sig), device=dev,
                         **mesh_phase_options(lp, op, seed, cfg["dpsr_center"]))
    nets = {m.model_name: m for m in [deform, deform_back] + (mesh.networks() if mesh is not None else [])}
    if start:
        gaussians.load_ply(start, iteration=first_iter)
        for name, m in nets.items():
            if os.path.isdir(os.path.join(start, name)):
                m.load_weights(start, iteration=first_iter)
            else:
                log(f"[resume] {start} has no {name} weights: starting that network afresh")
    if mesh is not None and mesh.normal_init:
        mesh.normal_init_out_dir = lp.model_path
    background = torch.tensor([1.0, 1.0, 1.0] if lp.white_background else [0.0, 0.0, 0.0], dtype=torch.float32, device=dev)
    tr = _loss_logging_trainer()(gaussians, deform, deform_back, cameras, opt=op, pipe=pp, background=background, is_blender=lp.is_blender,
                                 is_6dof=lp.is_6dof, rank=0, world=1, seed=seed, densify=True, cameras_extent=extent,
                                 prune_threshold=lp.prune_threshold, white_background=lp.white_background, mesh=mesh)
    iterations = int(op.iterations)
    every = lambda k: iteration_list(k, cfg[k]) if cfg[k] is not None else sorted(set(list(range(5000, iterations + 1, 5000)) + [iterations]))
    save_at, ckpt_at = every("save_iterations"), every("checkpoint_iterations")
    log_every = max(int(cfg["log_every"]), 1)
    # one row per step of the current window, written on the device, read back once per window
    window = torch.zeros((log_every, len(LOG_COLUMNS)), dtype=torch.float32, device=dev)
    rows, present, history, saved = [], [], {}, []

    def flush():
        if not rows:
            return
        host = window[:len(rows)].cpu().numpy()  # the one read-back of the window
        for k, it in enumerate(rows):
            history[it] = {c: float(host[k, j]) for j, c in enumerate(LOG_COLUMNS) if c in present[k]}
        last = history[rows[-1]]
        log(f"[ITER {rows[-1]}] " + " ".join(f"{c} {v:.6f}" for c, v in last.items()) + f" points {gaussians.get_xyz.shape[0]}")
        rows.clear()
        present.clear()

    def save(it):
        if it in save_at:
            scene.save(it)
        if it in ckpt_at:
            for m in nets.values():
                m.save_weights(lp.model_path, it)
        if it in save_at or it in ckpt_at:
            saved.append(it)
            log(f"[ITER {it}] saved to {lp.model_path}")

    tr.freeze_gc()
    for it in range(first_iter + 1, iterations + 1):
        loss, _ = tr.step(it)
        row = window[len(rows)]
        row[0] = loss
        for j, c in enumerate(LOG_COLUMNS[1:], 1):
            if c in tr.last_losses:
                row[j] = tr.last_losses[c]
        rows.append(it)
        present.append(("loss",) + tuple(tr.last_losses))
        if len(rows) == log_every or it == iterations:
            flush()
        save(it)
    flush()
    test = None
    tests = scene.getTestCameras()
    if tests:
        from .evaluate import testing
        in_mesh = mesh is not None and iterations >= op.dpsr_iter
        from .lpips import LPIPS
        lpips = {net: LPIPS(net, cfg["lpips_" + net], dev) for net in ("alex", "vgg") if cfg["lpips_" + net]}
        test = testing(gaussians, deform, deform_back, tests, pipe=pp, background=background, mesh=mesh if in_mesh else None,
                       is_6dof=lp.is_6dof, white_background=lp.white_background, out_dir=lp.model_path,
                       lpips=lpips or None)
        log(f"[TEST] {len(tests)} views: " + " ".join(f"{k} {v:.4f}" for k, v in test["gaussian"].items())
            + "".join(f" lpips_{net} {v:.4f}" for net, v in (test["lpips"]["gaussian"] if lpips else {}).items()))
    return {"log": history, "trainer": tr, "scene": scene, "gaussians": gaussians, "networks": nets, "mesh": mesh, "first_iter": first_iter,
            "saved": saved, "test": test}


def main(argv=None):
    cfg = config_from_argv(sys.argv[1:] if argv is None else argv)
    quiet = bool(cfg["quiet"])
    training(cfg, log=(lambda *a, **k: None) if quiet else print)
    return 0


if __name__ == "__main__":
    sys.exit(main())
