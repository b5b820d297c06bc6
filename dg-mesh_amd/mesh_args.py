"""What the mesh tools (mesh_clean, mesh_smooth, mesh_simplify, mesh_repair, mesh_topology, mesh_inside, mesh_ray, mesh_texture)
share in reading their arguments: the check that a tensor is one the kernels take, and the conversion of a stage's spec.  A new
mesh stage validates through mesh() or faces() and converts its spec through spec_of(); its place in the exports is mesh_post.

The kernels read fp32 vertices and int32 faces through raw device pointers: a tensor on the host, of another dtype or of another
shape is refused here, by name, never converted.  `who` is "module.function", the caller as its user wrote it."""
import torch


def need(who, t, what, dtype, shape_label="(n, 3)"):
    """`t`, the argument called `what`, is a CUDA/HIP tensor of `dtype` with three columns.  RuntimeError: not a device tensor, another
    dtype; ValueError: another shape (`shape_label` is how the message writes the wanted one)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who}: {what} must be a CUDA/HIP tensor (dg-mesh_amd has no CPU path)")
    if t.dtype != dtype:
        raise RuntimeError(f"{who}: {what} must be {dtype}, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{who}: {what} must be {shape_label}, got {tuple(t.shape)}")


def one_device(who, first, *rest):
    """Every (what, tensor) pair of `rest` is on the device of the pair `first`; ValueError names both devices."""
    for what, t in rest:
        if t.device != first[1].device:
            raise ValueError(f"{who}: {first[0]} on {first[1].device}, {what} on {t.device}")


def mesh(who, verts, faces, *more):
    """verts (V, 3) fp32 and faces (F, 3) int32, with every (what, tensor) pair of `more` an (n, 3) fp32 tensor, all on one device
    -> verts and faces detached and contiguous."""
    need(who, verts, "verts", torch.float32, "(V, 3)")
    need(who, faces, "faces", torch.int32, "(F, 3)")
    for what, t in more:
        need(who, t, what, torch.float32)
    one_device(who, ("verts", verts), ("faces", faces), *more)
    return verts.detach().contiguous(), faces.detach().contiguous()


def faces(who, faces, num_verts=None):
    """faces (F, 3) int32 alone, for what needs no coordinates, and num_verts >= 0 when it is given -> faces detached and contiguous."""
    need(who, faces, "faces", torch.int32, "(F, 3)")
    if num_verts is not None and int(num_verts) < 0:
        raise ValueError(f"{who}: num_verts must be >= 0, got {num_verts}")
    return faces.detach().contiguous()


def labels(who, labels, num_verts, device):
    """labels (num_verts,) int32 on `device` (mesh_clean.connected_components' output) -> contiguous."""
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
        raise RuntimeError(f"{who}: labels must be a CUDA/HIP tensor (dg-mesh_amd has no CPU path)")
    if labels.dtype != torch.int32 or tuple(labels.shape) != (num_verts,) or labels.device != device:
        raise ValueError(f"{who}: labels must be ({num_verts},) int32 on {device}")
    return labels.contiguous()


def spec_of(module_name, arg_name, cls, value):
    """None, an instance of the dataclass `cls` or a dict of its fields -> an instance of `cls`, or None ("do nothing")."""
    if value is None or isinstance(value, cls):
        return value
    if isinstance(value, dict):
        return cls(**value)
    raise TypeError(f"{module_name}: {arg_name} must be None, a {cls.__name__} or a dict of its fields, got {type(value).__name__}")
