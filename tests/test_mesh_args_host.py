"""What the mesh tools share on the host (no GPU): mesh_args' argument check reached through the tools' own entry points, spec_of
through every module's as_spec, and mesh_post.apply's order and pass-through with the four stages replaced by recorders.

A refusal must come before any kernel is reached, so the dtype and shape cases run here too: OnDevice is a host tensor that says
is_cuda, which is all the check asks of a tensor before it looks at dtype and shape."""
import importlib
import itertools

import numpy as np
import pytest
import torch

from conftest import pkg


class OnDevice(torch.Tensor):
    is_cuda = True


def on_device(t):
    return t.as_subclass(OnDevice)


V = on_device(torch.zeros(4, 3))
F = on_device(torch.zeros((2, 3), dtype=torch.int32))
P = on_device(torch.zeros(5, 3))
HOST_V, HOST_F = torch.zeros(4, 3), torch.zeros((2, 3), dtype=torch.int32)


def smooth(verts, faces):
    return pkg("mesh_smooth").smooth_mesh(verts, faces)


def components(faces, num_verts=4):
    return pkg("mesh_clean").connected_components(faces, num_verts)


def cast(origins, dirs, verts=V, faces=F):
    return pkg("mesh_ray").ray_cast(origins, dirs, verts, faces, accel=None)


def winding(points, verts=V, faces=F):
    return pkg("mesh_inside").winding_number(points, verts, faces)


# (the call, the exception, what the message must hold: the module and function, the argument, and what was wrong with it)
REFUSALS = [
    # a host tensor and a numpy array
    (lambda: smooth(HOST_V, HOST_F), RuntimeError, ("mesh_smooth.smooth_mesh", "verts must be a CUDA/HIP tensor", "no CPU path")),
    (lambda: smooth(V, HOST_F), RuntimeError, ("mesh_smooth.smooth_mesh", "faces must be a CUDA/HIP tensor", "no CPU path")),
    (lambda: smooth(np.zeros((4, 3), np.float32), F), RuntimeError, ("mesh_smooth.smooth_mesh", "verts must be a CUDA/HIP tensor")),
    (lambda: components(HOST_F), RuntimeError, ("mesh_clean.connected_components", "faces must be a CUDA/HIP tensor", "no CPU path")),
    (lambda: components(np.zeros((2, 3), np.int32)), RuntimeError, ("mesh_clean.connected_components", "faces must be a CUDA/HIP tensor")),
    (lambda: cast(torch.zeros(5, 3), P), RuntimeError, ("mesh_ray.ray_cast", "origins must be a CUDA/HIP tensor", "no CPU path")),
    (lambda: cast(P, np.zeros((5, 3), np.float32)), RuntimeError, ("mesh_ray.ray_cast", "dirs must be a CUDA/HIP tensor")),
    (lambda: cast(P, P, HOST_V, F), RuntimeError, ("mesh_ray.ray_cast", "verts must be a CUDA/HIP tensor")),
    (lambda: winding(torch.zeros(5, 3)), RuntimeError, ("mesh_inside.winding_number", "points must be a CUDA/HIP tensor", "no CPU path")),
    (lambda: winding(np.zeros((5, 3), np.float32)), RuntimeError, ("mesh_inside.winding_number", "points must be a CUDA/HIP tensor")),
    # a wrong dtype
    (lambda: smooth(V.double(), F), RuntimeError, ("mesh_smooth.smooth_mesh", "verts must be torch.float32, got torch.float64")),
    (lambda: smooth(V, F.long()), RuntimeError, ("mesh_smooth.smooth_mesh", "faces must be torch.int32, got torch.int64")),
    (lambda: components(F.long()), RuntimeError, ("mesh_clean.connected_components", "faces must be torch.int32, got torch.int64")),
    (lambda: cast(P.double(), P), RuntimeError, ("mesh_ray.ray_cast", "origins must be torch.float32, got torch.float64")),
    (lambda: cast(P, P.half()), RuntimeError, ("mesh_ray.ray_cast", "dirs must be torch.float32, got torch.float16")),
    (lambda: cast(P, P, V, F.short()), RuntimeError, ("mesh_ray.ray_cast", "faces must be torch.int32, got torch.int16")),
    (lambda: winding(P.double()), RuntimeError, ("mesh_inside.winding_number", "points must be torch.float32, got torch.float64")),
    (lambda: winding(P, V, F.long()), RuntimeError, ("mesh_inside.winding_number", "faces must be torch.int32, got torch.int64")),
    # a wrong shape
    (lambda: smooth(V[:, :2], F), ValueError, ("mesh_smooth.smooth_mesh", "verts must be (V, 3), got (4, 2)")),
    (lambda: smooth(V, F.reshape(3, 2)), ValueError, ("mesh_smooth.smooth_mesh", "faces must be (F, 3), got (3, 2)")),
    (lambda: components(F.reshape(-1)), ValueError, ("mesh_clean.connected_components", "faces must be (F, 3), got (6,)")),
    (lambda: cast(P[:, :2], P), ValueError, ("mesh_ray.ray_cast", "origins must be (n, 3), got (5, 2)")),
    (lambda: cast(P, P[None]), ValueError, ("mesh_ray.ray_cast", "dirs must be (n, 3), got (1, 5, 3)")),
    (lambda: winding(P.reshape(-1)), ValueError, ("mesh_inside.winding_number", "points must be (n, 3), got (15,)")),
    (lambda: winding(P, V.reshape(3, 4)), ValueError, ("mesh_inside.winding_number", "verts must be (V, 3), got (3, 4)")),
    # a wrong num_verts
    (lambda: components(F, -1), ValueError, ("mesh_clean.connected_components", "num_verts must be >= 0, got -1")),
    (lambda: pkg("mesh_topology").mesh_edges(F, -3), ValueError, ("mesh_topology.mesh_edges", "num_verts must be >= 0, got -3")),
    # labels, and tensors on two devices
    (lambda: pkg("mesh_clean").component_table(V, F, torch.zeros(4, dtype=torch.int32)), RuntimeError,
     ("mesh_clean.component_table", "labels must be a CUDA/HIP tensor")),
    (lambda: pkg("mesh_clean").component_table(V, F, on_device(torch.zeros(3, dtype=torch.int32))), ValueError,
     ("mesh_clean.component_table", "labels must be (4,) int32 on cpu")),
    (lambda: smooth(V, on_device(torch.zeros((2, 3), dtype=torch.int32, device="meta"))), ValueError,
     ("mesh_smooth.smooth_mesh", "verts on cpu, faces on meta")),
    (lambda: winding(on_device(torch.zeros((5, 3), device="meta"))), ValueError, ("mesh_inside.winding_number", "verts on cpu, points on meta")),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_refusals_name_the_module_the_function_and_the_argument(case):
    call, exc, words = REFUSALS[case]
    with pytest.raises(exc) as caught:
        call()
    assert type(caught.value) is exc
    for word in words:
        assert word in str(caught.value), (word, str(caught.value))


def test_the_check_hands_back_detached_contiguous_tensors():
    A = pkg("mesh_args")
    wide = on_device(torch.zeros(4, 6))
    verts, faces = A.mesh("here.fn", wide[:, ::2].requires_grad_(), F, ("points", P))
    assert verts.is_contiguous() and not verts.requires_grad and faces.is_contiguous() and tuple(verts.shape) == (4, 3)
    assert A.faces("here.fn", F, 0).is_contiguous() and A.faces("here.fn", F).dtype == torch.int32
    assert A.need("here.fn", P, "points", torch.float32) is None


SPECS = [("mesh_clean", "clean", "CleanSpec", {"largest": True, "min_faces": 3}),
         ("mesh_smooth", "smooth", "SmoothSpec", {"iterations": 3, "boundary": "curve"}),
         ("mesh_simplify", "simplify", "SimplifySpec", {"grid": 12}),
         ("mesh_repair", "repair", "RepairSpec", {"max_hole_edges": 30, "outward": False}),
         ("mesh_texture", "texture", "TextureSpec", {"cell": 6, "format": "glb", "ao_samples": 4})]


@pytest.mark.parametrize("module, arg, cls, fields", SPECS)
def test_spec_of_through_every_as_spec(module, arg, cls, fields):
    M = pkg(module)
    Spec = getattr(M, cls)
    assert M.as_spec(None) is None
    given = Spec(**fields)
    assert M.as_spec(given) is given
    made = M.as_spec(dict(fields))
    assert type(made) is Spec and made == given and made is not given
    for bad in ("a string", 3, [fields], (fields,)):
        with pytest.raises(TypeError) as caught:
            M.as_spec(bad)
        text = str(caught.value)
        assert text.startswith(f"{module}: {arg} must be None, a {cls} or a dict of its fields") and type(bad).__name__ in text
    with pytest.raises(TypeError):
        M.as_spec({"no_such_field": 1})
    assert pkg("mesh_args").spec_of(module, arg, Spec, fields) == given


# ---- mesh_post.apply with the four stages replaced by recorders -------------------------------------------------------------------------
@pytest.fixture
def recorded(monkeypatch):
    """calls: [(stage, spec, inputs, outputs)] in call order; every recorder hands out new objects, as many as it was given."""
    calls = []
    for stage in pkg("mesh_post").ORDER:
        def apply(spec, *mesh, stage=stage):
            out = tuple(object() for _ in mesh)
            calls.append((stage, spec, mesh, out))
            return out

        monkeypatch.setattr(pkg("mesh_" + stage), "apply", apply)
    return calls


@pytest.mark.parametrize("on", list(itertools.product((False, True), repeat=4)), ids=lambda on: "".join("01"[x] for x in on))
@pytest.mark.parametrize("n_attributes", [0, 2])
def test_apply_calls_the_enabled_stages_in_order(recorded, on, n_attributes):
    MP = pkg("mesh_post")
    assert MP.ORDER == ("clean", "smooth", "simplify", "repair")
    specs = {stage: {"stage": stage} for stage, enabled in zip(MP.ORDER, on) if enabled}
    given = tuple(object() for _ in range(2 + n_attributes))
    # (the keywords in another order than ORDER: the order is apply's, not the caller's)
    out = MP.apply(*given, **{stage: specs.get(stage) for stage in ("repair", "simplify", "clean", "smooth")})
    assert [c[0] for c in recorded] == [stage for stage in MP.ORDER if stage in specs]
    handed = given
    for stage, spec, inputs, outputs in recorded:
        assert spec is specs[stage]
        assert len(inputs) == len(handed) and all(a is b for a, b in zip(inputs, handed))  # threaded from the stage before
        handed = outputs
    assert isinstance(out, tuple) and len(out) == len(given) and all(a is b for a, b in zip(out, handed))
    if not any(on):
        assert all(a is b for a, b in zip(out, given))  # the inputs themselves


def test_apply_imports_only_the_stages_it_runs(recorded, monkeypatch):
    MP = pkg("mesh_post")
    real, asked = importlib.import_module, []

    def import_module(name, package=None):
        asked.append(name)
        return real(name, package)

    monkeypatch.setattr(importlib, "import_module", import_module)
    MP.apply(V, F, None)
    MP.apply(V, F, None, smooth={}, repair={})
    monkeypatch.undo()
    assert asked == [".mesh_smooth", ".mesh_repair"]


def test_the_exports_take_the_four_keywords_and_call_mesh_post():
    import inspect
    for fn in (pkg("trainer").MeshPhase.extract_mesh, pkg("evaluate").testing, pkg("visualize").export_dynamic_mesh,
               pkg("correspondence").export_correspondence):
        names = list(inspect.signature(fn).parameters)
        at = names.index("clean")
        assert names[at:at + 4] == ["clean", "simplify", "smooth", "repair"]
        assert "mesh_post" in fn.__doc__
    assert list(inspect.signature(pkg("mesh_post").apply).parameters) == ["verts", "faces", "attributes", "clean", "smooth", "simplify", "repair"]
