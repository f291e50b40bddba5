"""Drop-in `losses.WireframeLoss.WireframeLoss` (reference losses/WireframeLoss.py:6-283) — row f-1,
the caller of the hot path's backward.

Same constructor, same `forward(predictions, targets) -> dict` with the same four keys.  Default
(`assignment="device"`): the B Hungarian cost matrices, the assignment itself (Jonker-Volgenant on the
device, csrc/loss.hip), SmoothL1 / BCE / BCE and their gradients w.r.t. the model outputs are three
kernel launches with no host synchronisation; `total_loss.backward()` hands those gradients to the model.
`assignment="scipy"` keeps the reference's host solver (`linear_sum_assignment`, :236) behind ONE
device->host copy for the batch (the reference syncs per sample).

Differences to know about:
  * target counts larger than min(max_vertices, targets['vertices'].shape[1]) are CLAMPED on the device path
    (the reference's inf-padded cost matrix makes scipy raise there; raising would need a host sync); the
    scipy path raises like the reference.
  * exactly tied assignment costs: the device solver works on the same padded square problem in the same row
    order as scipy, but its tie rule is its own — among the columns of minimal path cost the unassigned one of
    lowest index, else the lowest index — and on tied problems (lattice coordinates, say) it may return another
    optimal matching than scipy.  The rule is pinned: tests/lsa_model.py states the solver in numpy and
    tests/test_loss_assign_forms_gpu.py holds every kernel form to it element for element, tied inputs included.
  * non-finite costs (NaN model outputs after a poisoned optimizer step, say): the device solver reads NaN and
    +inf as FLT_MAX and -inf as -FLT_MAX, so it always terminates and always returns a permutation; the loss
    terms then produce NaN from NaN inputs as torch would, and the step goes on without a host check.  The
    reference and the scipy path raise a ValueError there.
  * a padded edge head (PointCloudToWireframe.set_edge_layout("padded")) predicts [B, V(V-1)/2] with the width
    max_s E_s in predictions["edge_width"] (a device scalar): the edge term runs over min(that width, label width),
    as the reference's over min(pred width, label width), so labels may be allocated at full width V(V-1)/2.
  * `last_assignment`: after every forward, the matching the loss used, as an int32 [B, V] device tensor — prediction
    slot p of sample b is matched to target last_assignment[b, p] iff that value is below the sample's (clamped) count.
    On the device path it is the solver's output itself (no extra launch; unmatched slots hold their dummy column);
    on the scipy path it is built from the match lists with V in the unmatched slots.  wf3d.meter.WireframeMeter
    turns it into batch-wide metrics without a host read.
  * `edge_targets="matched"` (opt-in; the default "positional" is the reference).  The reference compares column k of
    `edge_probs[b]` — the pair (p, q) of predicted SLOTS — with column k of `edge_labels[b]`, the pair (i, j) of
    ground-truth vertices: right only under an identity matching.  "matched" materialises, after the assignment, the
    labels of the pairs of targets that the slots are matched to (ops.edge_labels_matched, one launch; specification
    wf3d.targets.matched_edge_labels) and runs the edge term on them at the prediction's width.  The pair order of the
    prediction row is that of `predictions["edge_counts"]` when the key is there (a padded edge head) and of the target
    counts otherwise (train mode).  `last_edge_labels` keeps the tensor, [B, edge-term width], beside `last_assignment`.
    A pair with an unmatched slot is labelled 0; edges to targets matched by slots at or past the pair count stay
    unsupervised, and existence targets stay positional.
  * `edge_pos_weight=w`, `edge_focal_gamma=g` (opt-in, defaults 1 and 0): the edge element becomes
    -(w t (1-p)^g max(log p, -100) + (1-t) p^g max(log1p(-p), -100)) with its own derivative as the gradient, same
    normaliser.  Columns with p == t in {0, 1} (a ragged batch's padding) contribute exactly 0.  Both `assignment=`
    values take every option; under "scipy" a non-default option runs the terms from `last_assignment` on the device
    entry points.
  * `set_data_parallel()`: with one process per GPU each rank sees a slice of the batch, but the reference's
    normalisers are batch-wide (matched-vertex count, :276-281; B x common edge width, :82-86).  When enabled,
    the three normalisers are exchanged (one tiny all-reduce) and each term is rescaled so that the MEAN over
    ranks of the local losses / gradients equals the single-process loss / gradient of the whole batch."""
import numpy as np
import torch
import torch.nn as nn
from scipy.optimize import linear_sum_assignment

from wf3d import ops


class _TermsFn(torch.autograd.Function):
    """The backward of both forms: forward saved the gradients of the total w.r.t. its first three inputs; every output
    after the total is non-differentiable."""

    @staticmethod
    def backward(ctx, g_total, *_g_rest):
        dv, de, dd = ctx.saved_tensors
        return (dv * g_total, de * g_total, dd * g_total) + (None,) * (len(ctx.needs_input_grad) - 3)


def _edge_terms(verts, exist, edge, tverts, texist, tlabel, col4row, counts, weights, edge_width, edge_opts):
    """The term launch under a device assignment.  edge_opts None: today's launch.  Otherwise (matched, pair_counts,
    pos_weight, focal_gamma): matched labels are materialised first (one launch, label width = prediction width), and a
    non-default weight or gamma takes the balanced entry point.  Returns (losses, dverts, dexist, dedge, labels or None)."""
    matched, pair_counts, pos_weight, gamma = edge_opts or (False, None, 1.0, 0.0)
    labels = ops.edge_labels_matched(tlabel, col4row, counts, edge.shape[1], pair_counts) if matched else None
    tl = labels if matched else tlabel
    if pos_weight == 1.0 and gamma == 0.0:
        out = ops.loss_terms_assigned(verts, exist, edge, tverts, texist, tl, col4row, counts, weights, edge_width=edge_width)
    else:
        out = ops.loss_terms_assigned_bal(verts, exist, edge, tverts, texist, tl, col4row, counts, weights, pos_weight,
                                          gamma, edge_width=edge_width)
    return (*out, labels)


class _LossDevFn(_TermsFn):
    """Fully asynchronous variant: cost matrices, assignment, loss terms and gradients all on the device."""

    @staticmethod
    def forward(ctx, verts, exist, edge, tverts, texist, tlabel, counts, weights, scales=None, edge_width=None,
                edge_opts=None):
        exist_c = exist.contiguous()
        cost = ops.loss_cost_matrix(verts, exist_c, tverts, counts)
        # the square problem, rows in prediction order like scipy: L1 costs have exact ties (2 of 32 random samples
        # at V = 64) and the rectangular shortcut of ops.loss_assign(cost, counts) resolves them differently
        col4row = ops.loss_assign(cost)
        losses, dv, de, dd, labels = _edge_terms(verts, exist_c, edge.contiguous(), tverts, texist, tlabel, col4row, counts,
                                                 weights, edge_width, edge_opts)
        if scales is not None:       # data-parallel renormalisation: (vertex, existence, edge) factors, device scalars
            w = torch.tensor(weights, dtype=torch.float32, device=losses.device)
            losses = torch.cat([losses[:3], (losses[:3] * w * scales).sum().reshape(1)])
            dv, de, dd = dv * scales[0], de * scales[1], dd * scales[2]
        ctx.save_for_backward(dv, de, dd)
        ctx.mark_non_differentiable(losses, col4row, *(() if labels is None else (labels,)))
        # the assignment as solved (WireframeLoss.last_assignment) and the matched labels (last_edge_labels, or None)
        return losses[3].clone(), losses, col4row, labels


class _LossAssignedFn(_TermsFn):
    """The scipy path under a non-default edge option: the terms from its col4row (V in unmatched slots) on the device
    entry points, which hold the matched labels and the balanced element."""

    @staticmethod
    def forward(ctx, verts, exist, edge, tverts, texist, tlabel, col4row, counts, weights, edge_opts):
        losses, dv, de, dd, labels = _edge_terms(verts, exist.contiguous(), edge.contiguous(), tverts, texist, tlabel,
                                                 col4row, counts, weights, None, edge_opts)
        ctx.save_for_backward(dv, de, dd)
        ctx.mark_non_differentiable(losses, *(() if labels is None else (labels,)))
        return losses[3].clone(), losses, labels


class _LossFn(_TermsFn):
    @staticmethod
    def forward(ctx, verts, exist, edge, tverts, texist, tlabel, m_pred, m_tgt, m_off, n_match, weights):
        losses, dv, de, dd = ops.loss_terms(verts, exist.contiguous(), edge.contiguous(), tverts, texist, tlabel,
                                            m_pred, m_tgt, m_off, n_match, weights)
        ctx.save_for_backward(dv, de, dd)
        ctx.mark_non_differentiable(losses)
        return losses[3].clone(), losses


class WireframeLoss(nn.Module):
    def __init__(self, vertex_weight=1.0, edge_weight=1.0, existence_weight=1.0, assignment="device",
                 edge_targets="positional", edge_pos_weight=1.0, edge_focal_gamma=0.0):
        """assignment: "device" (default) = Hungarian matching on the GPU, no host sync at all;
        "scipy" = the reference's scipy.optimize.linear_sum_assignment on the host (one sync).
        edge_targets: "positional" (default, the reference) or "matched"; edge_pos_weight > 0 and edge_focal_gamma >= 0:
        the class-balanced edge element (module docstring).  The defaults are the reference's loss."""
        super().__init__()
        if assignment not in ("device", "scipy"):
            raise ValueError("assignment must be 'device' or 'scipy'")
        if edge_targets not in ("positional", "matched"):
            raise ValueError("edge_targets must be 'positional' or 'matched'")
        if isinstance(edge_pos_weight, bool) or not isinstance(edge_pos_weight, (int, float)) \
                or not (0.0 < edge_pos_weight < float("inf")):
            raise ValueError("edge_pos_weight must be a finite number > 0")
        if isinstance(edge_focal_gamma, bool) or not isinstance(edge_focal_gamma, (int, float)) \
                or not (0.0 <= edge_focal_gamma < float("inf")):
            raise ValueError("edge_focal_gamma must be a finite number >= 0")
        self.assignment = assignment
        self.edge_targets = edge_targets
        self.edge_pos_weight = float(edge_pos_weight)
        self.edge_focal_gamma = float(edge_focal_gamma)
        self.last_edge_labels = None     # fp32 [B, Ep] device tensor of the latest forward under edge_targets="matched"
        self.vertex_weight = vertex_weight
        self.edge_weight = edge_weight
        self.existence_weight = existence_weight
        self.smooth_l1_loss = nn.SmoothL1Loss()      # kept for attribute parity; not called
        self.bce_loss = nn.BCELoss()
        self._dp = (False, None)
        self.last_assignment = None      # int32 [B, V] device tensor of the latest forward (module docstring)

    def set_data_parallel(self, enabled=True, group=None):
        """One process per GPU, batch sharded over ranks: rescale the three terms to the batch-wide normalisers
        (module docstring).  No effect in a single process."""
        self._dp = (bool(enabled), group)
        return self

    def _dp_scales(self, counts, B, V, e_pred, e_tgt, dev):
        """(vertex, existence, edge) factors s with  mean_over_ranks(s * local term) == whole-batch term; None when not DP.
        One all-reduce of a [world, 3] tensor, nothing read back to the host."""
        import torch.distributed as dist
        enabled, group = self._dp
        if not enabled or not (dist.is_available() and dist.is_initialized()):
            return None
        W = dist.get_world_size(group)
        if W == 1:
            return None
        r = dist.get_rank(group)
        if torch.is_tensor(e_pred):       # a padded edge head's device width: min(width, e_tgt) without a host read
            common = e_pred.clamp(max=e_tgt).to(device=dev, dtype=torch.float32).reshape(())
        else:
            common = torch.tensor(float(min(e_pred, e_tgt)), device=dev)
        mine = torch.stack([counts.clamp(max=V).sum().to(torch.float32), torch.tensor(float(B), device=dev), common])
        table = torch.zeros(W, 3, dtype=torch.float32, device=dev)
        table[r] = mine
        dist.all_reduce(table, group=group)
        n_g, b_g, w_g = table[:, 0].sum().clamp_min(1.0), table[:, 1].sum(), table[:, 2].max().clamp_min(1.0)
        return torch.stack([W * mine[0] / n_g, W * mine[1] / b_g, W * mine[1] * mine[2] / (b_g * w_g)])

    def _hungarian_matching(self, predictions, targets):
        """list of (pred_indices, target_indices) numpy arrays per sample (reference :106-237)."""
        pv = predictions["vertices"]
        B, V, _ = pv.shape
        counts = targets["vertex_counts"].to(device=pv.device, dtype=torch.int64).contiguous()
        tv = targets["vertices"].to(device=pv.device, dtype=torch.float32).contiguous()
        cost = ops.loss_cost_matrix(pv.detach(), predictions["existence_probabilities"].detach().contiguous(), tv, counts)
        cost_np = cost.cpu().numpy()                               # the one sync of the loss
        cnt = counts.cpu().tolist()
        out = []
        for b in range(B):
            if cnt[b] > V:
                raise ValueError("target vertex count exceeds max_vertices (the reference's inf-padded matrix is infeasible too)")
            pi, ti = linear_sum_assignment(cost_np[b])
            keep = ti < cnt[b]
            out.append((pi[keep], ti[keep]))
        return out

    def forward(self, predictions, targets):
        pv = predictions["vertices"]
        pe = predictions["existence_probabilities"]
        pp = predictions["edge_probs"]
        dev = pv.device
        B, V = pv.shape[0], pv.shape[1]
        if tuple(pe.shape) != (B, V):
            raise ValueError(f"existence_probabilities must be [B, V] = {(B, V)}, got {tuple(pe.shape)}")
        if tuple(targets["vertex_existence"].shape) != (B, V):
            raise ValueError(f"targets['vertex_existence'] must be [B, V] = {(B, V)}, got {tuple(targets['vertex_existence'].shape)}")
        if targets["vertices"].dim() != 3 or targets["vertices"].shape[0] != B or targets["vertices"].shape[2] != 3:
            raise ValueError("targets['vertices'] must be [B, Vt, 3]")
        tv, te, tl = (targets[k].to(device=dev, dtype=torch.float32).contiguous()
                      for k in ("vertices", "vertex_existence", "edge_labels"))
        # weights in the kernels' (vertex, existence, edge) order
        w = (self.vertex_weight, self.existence_weight, self.edge_weight)
        matched = self.edge_targets == "matched"
        edge_opts = None          # all three edge options at their defaults: exactly the launches of the plain loss
        if matched or self.edge_pos_weight != 1.0 or self.edge_focal_gamma != 0.0:
            # matched labels follow the pair order of the prediction row: a padded edge head says which counts it used
            pc = predictions.get("edge_counts") if matched else None
            pc = pc.to(device=dev, dtype=torch.int64).contiguous() if pc is not None else None
            edge_opts = (matched, pc, self.edge_pos_weight, self.edge_focal_gamma)
        if self.assignment == "device":
            counts = targets["vertex_counts"].to(device=dev, dtype=torch.int64).contiguous()
            # the kernels index targets['vertices'][b, :counts[b]] and need counts[b] <= V real columns: clamp (docstring)
            counts = counts.clamp(min=0, max=min(V, tv.shape[1]))
            ew = predictions.get("edge_width")        # padded edge head: the prediction width is a device scalar
            ew = ew.to(device=dev, dtype=torch.int64) if ew is not None else None
            # matched labels are as wide as the prediction
            scales = self._dp_scales(counts, B, V, pp.shape[1] if ew is None else ew, pp.shape[1] if matched else tl.shape[1], dev)
            total, parts, self.last_assignment, self.last_edge_labels = _LossDevFn.apply(pv, pe, pp, tv, te, tl, counts, w,
                                                                                         scales, ew, edge_opts)
            return {"total_loss": total, "vertex_loss": parts[0], "existence_loss": parts[1], "edge_loss": parts[2]}
        matches = self._hungarian_matching(predictions, targets)
        lens = [len(m[0]) for m in matches]
        off = np.zeros(len(lens) + 1, dtype=np.int32)
        np.cumsum(lens, out=off[1:])
        n_match = int(off[-1])
        cat = lambda k: (np.concatenate([m[k] for m in matches]).astype(np.int32) if n_match else np.zeros(0, np.int32))   # noqa: E731
        col4row = np.full((B, V), V, dtype=np.int32)            # last_assignment: unmatched slots hold V
        for b, (pi, ti) in enumerate(matches):
            col4row[b, pi] = ti
        packed = torch.from_numpy(np.concatenate([cat(0), cat(1), off, col4row.ravel()])).to(dev, non_blocking=True)
        m_pred, m_tgt, m_off = packed[:n_match], packed[n_match:2 * n_match], packed[2 * n_match:2 * n_match + B + 1]
        self.last_assignment = packed[2 * n_match + B + 1:].view(B, V)
        if predictions.get("edge_width") is not None:
            # padded edge head: this path has synced already, the width is read here and the columns past it dropped
            pp = pp[:, :int(predictions["edge_width"])]
        if edge_opts is not None:
            counts = targets["vertex_counts"].to(device=dev, dtype=torch.int64).clamp(min=0, max=min(V, tv.shape[1])).contiguous()
            total, parts, self.last_edge_labels = _LossAssignedFn.apply(pv, pe, pp, tv, te, tl, self.last_assignment, counts,
                                                                        w, edge_opts)
            return {"total_loss": total, "vertex_loss": parts[0], "existence_loss": parts[1], "edge_loss": parts[2]}
        self.last_edge_labels = None
        total, parts = _LossFn.apply(pv, pe, pp, tv, te, tl, m_pred, m_tgt, m_off, n_match, w)
        return {"total_loss": total, "vertex_loss": parts[0], "existence_loss": parts[1], "edge_loss": parts[2]}
