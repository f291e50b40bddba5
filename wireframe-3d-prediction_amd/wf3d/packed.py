"""Packed point-cloud batches: clouds of different lengths concatenated along the point axis, with their point counts.

    points, point_counts = pack([cloud_0 [N_0, Din], cloud_1 [N_1, Din], ...])     # [sum N_b, Din], [N_0, N_1, ...]
    out = model.forward_packed(points.cuda(), point_counts)

Every cloud runs at its own resolution: outputs and gradients are those of the model on that cloud alone."""
import torch

from .ops import PackedLayout, point_counts_list  # noqa: F401  (the layout object of a packed batch)


def pack(clouds):
    """list of [N_b, Din] tensors (or arrays) -> (points [sum N_b, Din] float32, point_counts: list of ints)."""
    clouds = [torch.as_tensor(c) for c in clouds]
    if not clouds:
        raise ValueError("wf3d.pack: an empty batch")
    for c in clouds:
        if c.dim() != 2 or c.shape[1:] != clouds[0].shape[1:]:
            raise ValueError(f"wf3d.pack: every cloud must be [N_b, Din] with one Din (got {tuple(c.shape)})")
        if c.shape[0] < 1:
            raise ValueError("wf3d.pack: every cloud needs at least one point")
    return torch.cat([c.float() for c in clouds], dim=0).contiguous(), [int(c.shape[0]) for c in clouds]
