"""The train driver's configuration (train.py): defaults + flat YAML + command-line overrides, checked against the reference's own
parameter objects for every Blender-layout config it ships (tests/test_reference_configs.reference_params builds those)."""
import glob
import os

import pytest

from conftest import ROOT, pkg
from test_reference_configs import REF, reference_params

# attributes of this project's parameter classes that the reference's groups do not define, and why
PROJECT_ONLY = {"normal_deform_delay": "NORMAL_WARMUP_ITER, a module constant of the reference's train.py (2000), not a parameter"}


def _blender_configs():
    found = sorted(os.path.relpath(p, os.path.join(REF, "configs")) for d in ("d-nerf", "dg-mesh")
                   for p in glob.glob(os.path.join(REF, "configs", d, "*.yaml")))
    return found or ["d-nerf/jumpingjacks.yaml", "dg-mesh/beagle.yaml"]


@pytest.mark.parametrize("config", _blender_configs())
def test_merged_config_equals_the_reference(config):
    T = pkg("train")
    lp, op, pp = reference_params(config)  # (skips when oracle/_ref is not built)
    cfg = T.merge_config(T.load_yaml(os.path.join(REF, "configs", config)), log=lambda *a: None)
    mine = T.split_config(cfg)
    checked = 0
    for obj in mine:
        for name in T._fields(type(obj)):
            if name in PROJECT_ONLY:
                continue
            holders = [g for g in (lp, op, pp) if hasattr(g, name)]
            assert holders, f"{name}: not a parameter of the reference (list it in PROJECT_ONLY with the reason)"
            want, got = getattr(holders[0], name), getattr(obj, name)
            if name == "source_path":  # (the reference's extract() makes it absolute)
                want, got = os.path.basename(want), os.path.basename(got)
            assert got == want, f"{config}: {name} = {got!r}, the reference has {want!r}"
            checked += 1
    assert checked >= 44
    assert mine[1].normal_deform_delay == pkg("trainer").NORMAL_WARMUP_ITER


def test_defaults_equal_the_reference_defaults():
    """No YAML at all: every default of the three classes is the reference's."""
    T = pkg("train")
    from argparse import ArgumentParser
    from test_reference_configs import PYREF, _load_pyc
    if not os.path.exists(os.path.join(PYREF, "arguments.pyc")):
        pytest.skip("oracle/_ref/pyref/arguments.pyc not built")
    R = _load_pyc("ref_arguments_defaults", "arguments.pyc")
    parser = ArgumentParser()
    groups = [R.ModelParams(parser), R.OptimizationParams(parser), R.PipelineParams(parser)]
    args = parser.parse_args([])
    ref = [g.extract(args) for g in groups]
    for cls in T.PARAM_CLASSES:
        for name, got in T._fields(cls).items():
            if name in PROJECT_ONLY:
                continue
            holders = [g for g in ref if hasattr(g, name)]
            assert holders, name
            want = getattr(holders[0], name)
            if name == "source_path":
                continue
            assert got == want, f"default of {name}: {got!r}, the reference has {want!r}"


def test_unknown_keys_are_listed_and_reference_only_keys_ignored():
    T = pkg("train")
    with pytest.raises(ValueError) as e:
        T.merge_config({"iterations": 10, "zeta": 1, "alpha_typo": 2})
    assert "alpha_typo, zeta" in str(e.value)
    lines = []
    cfg = T.merge_config({"expname": "x", "data_device": "cuda", "iterations": 10}, log=lines.append)
    assert cfg["iterations"] == 10 and "expname" not in cfg
    assert len(lines) == 1 and "data_device" in lines[0] and "expname" in lines[0]
    for k in T.IGNORED_KEYS:
        assert k not in T.default_config()


def test_yaml_then_command_line(tmp_path):
    T = pkg("train")
    y = tmp_path / "c.yaml"
    y.write_text("iterations: 300\nwhite_background: True\ndpsr_sig: 3.0\nsource_path: data/x\n")
    cfg = T.config_from_argv(["--config", str(y), "--iterations", "20", "--lambda_dssim=0.3", "--eval", "--model_path", "123",
                              "--grid_res", "48", "--position_lr_init", "1e-4", "--save_iterations", "[5, 20]", "--warm_up", "1000.0"],
                             log=lambda *a: None)
    assert cfg["iterations"] == 20 and isinstance(cfg["iterations"], int)          # the command line wins over the file
    assert cfg["white_background"] is True and cfg["dpsr_sig"] == 3.0 and cfg["source_path"] == "data/x"   # the file over defaults
    assert cfg["lambda_dssim"] == 0.3 and cfg["eval"] is True and cfg["model_path"] == "123" and cfg["grid_res"] == 48
    assert cfg["position_lr_init"] == 1e-4 and isinstance(cfg["position_lr_init"], float)
    assert cfg["save_iterations"] == [5, 20] and cfg["warm_up"] == 1000 and isinstance(cfg["warm_up"], int)
    assert cfg["densify_until_iter"] == pkg("scene").OptimizationParams.densify_until_iter                  # an untouched default
    lp, op, pp = T.split_config(cfg)
    assert isinstance(op, pkg("scene").OptimizationParams) and op.iterations == 20 and lp.grid_res == 48 and pp.debug is False
    assert pkg("scene").OptimizationParams.iterations == 40_000, "split_config must not write to the classes"
    with pytest.raises(ValueError, match="nope"):
        T.config_from_argv(["--nope", "1"])
    with pytest.raises(ValueError):
        T.config_from_argv(["--eval", "maybe"])
    with pytest.raises(ValueError):
        T.config_from_argv(["iterations", "3"])
    nested = tmp_path / "n.yaml"
    nested.write_text("opt:\n  iterations: 3\n")
    with pytest.raises(ValueError, match="flat"):
        T.config_from_argv(["--config", str(nested)])


def test_training_needs_a_model_path():
    T = pkg("train")
    with pytest.raises(ValueError, match="model_path"):
        T.training(T.merge_config({}))


def test_mesh_phase_is_never_a_real_capture_for_the_readers_built():
    """The reference sets `real` by data type (iPhone, NeuralActor), not by is_blender: a Blender-layout scene trained with the
    default is_blender = False still measures its bounding box over the deformed frames."""
    T = pkg("train")
    assert T.ModelParams.is_blender is False
    lp, op, _ = T.split_config(T.merge_config({"source_path": "s", "model_path": "m"}))
    kw = T.mesh_phase_options(lp, op, seed=3)
    assert kw["real"] is False and kw["normal_init"] is True and kw["anchor"] is True and kw["seed"] == 3
    assert (kw["mesh_source"], kw["mesh_losses"], kw["gaussian_ratio"]) == ("diffmc", "render", lp.gaussian_ratio)
    lp.is_blender = True
    assert T.mesh_phase_options(lp, op)["real"] is False
    op.use_anchor = 0.0
    assert T.mesh_phase_options(lp, op)["anchor"] is False
    # a MeshPhase takes exactly these keywords
    ms = pkg("trainer").MeshPhase(None, None, None, dpsr=object(), device="cpu", n_verts=4, **kw)
    assert ms.real is False and ms.normal_init and ms.anchor
    # gaussian_center places the cube of real captures only: accepted from a reference config, not a key of this driver
    lines = []
    cfg = T.merge_config({"gaussian_center": [0.0, 0.0, 1.0]}, log=lines.append)
    assert "gaussian_center" not in cfg and "gaussian_center" in lines[0]


def test_iteration_lists_and_paths_from_the_command_line():
    T = pkg("train")
    q = lambda *a: T.config_from_argv(list(a), log=lambda *x: None)
    assert q("--save_iterations", "5")["save_iterations"] == [5]
    assert q("--checkpoint_iterations=7")["checkpoint_iterations"] == [7]
    assert q("--save_iterations", "[20, 5, 5]")["save_iterations"] == [5, 20]
    assert q("--start_checkpoint", "123")["start_checkpoint"] == "123"
    assert T.merge_config({"save_iterations": 9})["save_iterations"] == [9]          # (a scalar in the YAML file)
    assert q()["save_iterations"] is None and q()["start_checkpoint"] is None
    for bad in ("abc", "[1, x]", "2.5", "true"):
        with pytest.raises(ValueError, match="save_iterations"):
            q("--save_iterations", bad)
    with pytest.raises(ValueError, match="start_checkpoint"):
        T.merge_config({"start_checkpoint": 123})
