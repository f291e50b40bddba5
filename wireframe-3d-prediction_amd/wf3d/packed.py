"""Packed point-cloud batches: clouds of different lengths concatenated along the point axis, with their point counts.

    points, point_counts = pack([cloud_0 [N_0, Din], cloud_1 [N_1, Din], ...])     # [sum N_b, Din], [N_0, N_1, ...]
    out = model.forward_packed(points.cuda(), point_counts)

Every cloud runs at its own resolution: outputs and gradients are those of the model on that cloud alone.

For one graph capture over batches of any lengths, keep static buffers and refill them between replays:

    points_buf = torch.zeros(capacity, Din, device="cuda"); counts_buf = torch.zeros(B, dtype=torch.int64, device="cuda")
    pack_into(points_buf, counts_buf, clouds)
    out = model.forward_packed(points_buf, counts_buf, capacity=capacity)          # counts stay on the device"""
import torch

from .ops import DevicePackedLayout, PackedLayout, point_counts_list  # noqa: F401  (the layouts of a packed batch)


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


def pack_into(points_buf, counts_buf, clouds):
    """Copy a list of [N_b, Din] clouds into the static buffers of a capacity batch: points_buf [capacity, Din] gets the
    clouds in its first rows and zeros behind them, counts_buf (int64 or int32 [B]) their lengths.  The buffers may be on
    the device (two host-to-device copies, nothing is read back).  Raises ValueError, on the host, when the clouds do
    not fit.  Returns the list of counts."""
    if points_buf.dim() != 2 or counts_buf.dim() != 1 or counts_buf.dtype not in (torch.int64, torch.int32):
        raise ValueError("wf3d.pack_into: needs points_buf [capacity, Din] and an int64 or int32 counts_buf [B]")
    if len(clouds) != counts_buf.shape[0]:
        raise ValueError(f"wf3d.pack_into: {len(clouds)} clouds for a counts buffer of {counts_buf.shape[0]}")
    points, counts = pack(clouds)
    capacity, din = points_buf.shape
    if points.shape[1] != din:
        raise ValueError(f"wf3d.pack_into: the clouds have {points.shape[1]} columns, the buffer {din}")
    if points.shape[0] > capacity:
        raise ValueError(f"wf3d.pack_into: the clouds hold {points.shape[0]} points, above the capacity of {capacity} rows")
    staged = torch.zeros(capacity, din, dtype=points_buf.dtype, device=points.device)
    staged[:points.shape[0]] = points
    points_buf.copy_(staged)
    counts_buf.copy_(torch.tensor(counts, dtype=counts_buf.dtype))
    return counts
