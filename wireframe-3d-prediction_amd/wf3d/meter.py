"""Row f-2, second half: the per-step bookkeeping of the reference's training loop without its
per-step host syncs.

train.py:145-157 calls `total_loss.item()` (twice) and copies sample 0's predicted and target vertices to the host on EVERY
step to keep a loss history, the best loss so far and a monitoring RMSE; each of these drains the GPU queue.  `TrainMeter`
keeps the same quantities in a small device-resident record, updated by one launch per step (csrc/loss.hip,
wf3d_meter_update), and `read()` brings everything back in one copy — call it when the loop logs (every 20 steps in the
reference), not every step.

    meter = TrainMeter(device)
    for step in range(n):
        out = model(x, counts); res = criterion(out, targets); res["total_loss"].backward(); opt.step()
        meter.update(res, out["vertices"], targets["vertices"], counts)          # no sync
        if step % 20 == 0:
            m = meter.read()                                                     # one device -> host copy
            log(m["total_loss"], m["vertex_rmse"], m["best_loss"], m["best_vertex_rmse"])

`WireframeMeter` is the second meter: how well the model is doing, over the whole batch and under the loss's own Hungarian
matching (`WireframeLoss.last_assignment`) — matched vertex error, vertex existence and edge precision / recall — as
sums in a device-resident record, by two small launches per step (csrc/metrics.hip, wf3d_train_metrics) that read
nothing on the host and can be captured with the step.

    qm = WireframeMeter(device, distance_thresh=0.05, edge_threshold=0.5)
    for step in range(n):
        out = model(x, counts); res = criterion(out, targets); ...
        qm.update(out, targets, criterion.last_assignment)                      # no sync
        if step % 20 == 0:
            m = qm.read()                                                        # one device -> host copy
            log(m["last"]["matched_rmse"], m["running"]["edge_f1"])
            qm.reset()
"""
import math

import torch

from . import _lib
from ._lib import check
from .ops import _p, _stream


class TrainMeter:
    def __init__(self, device, history=4096):
        self.capacity = int(history)
        if self.capacity < 0:
            raise ValueError(f"wf3d.TrainMeter: history must be >= 0, got {history}")
        self.state = torch.zeros(8 + self.capacity, dtype=torch.float32, device=device)

    @torch.no_grad()
    def update(self, loss_dict, pred_vertices, target_vertices, counts=None):
        """loss_dict: WireframeLoss output (total_loss, vertex_loss, existence_loss, edge_loss: device scalars);
        pred_vertices [B, V, 3] (any vertex stride, unit inner stride), target_vertices [B, Vt, 3], counts [B] int64 or None."""
        def scalar(k):
            t = loss_dict.get(k)
            if t is None:
                return None
            if not t.is_cuda:
                raise RuntimeError("wf3d.TrainMeter: loss values must be device tensors (no CPU fallback)")
            return t.detach().reshape(-1).float()
        tot = scalar("total_loss")
        if tot is None:
            raise KeyError("total_loss")
        keep = [tot] + [scalar(k) for k in ("vertex_loss", "existence_loss", "edge_loss")]
        pv, tv = pred_vertices.detach(), target_vertices.detach()
        if pv.dtype != torch.float32 or tv.dtype != torch.float32 or pv.stride(-1) != 1 or tv.stride(-1) != 1:
            raise RuntimeError("wf3d.TrainMeter: fp32 vertices with unit inner stride expected")
        max_v = min(pv.shape[1], tv.shape[1])
        cnt = None
        if counts is not None:
            cnt = counts if counts.dtype == torch.int64 else counts.long()
            if not cnt.is_cuda:
                cnt = cnt.to(pv.device)
        check(_lib.load().wf3d_meter_update(_p(keep[0]), _p(keep[1]), _p(keep[2]), _p(keep[3]), _p(pv), pv.stride(1), _p(tv),
                                            tv.stride(1), _p(cnt), max_v, _p(self.state), self.capacity, _stream()), "meter_update")

    def read(self):
        """One device -> host copy: dict(steps, best_loss, best_vertex_rmse, total_loss, vertex_loss, existence_loss,
        edge_loss, vertex_rmse, loss_history (oldest first, at most `history` entries))."""
        s = self.state.cpu()
        steps = int(s[0])
        n = min(steps, self.capacity)
        ring = s[8:8 + self.capacity]
        if steps <= self.capacity or self.capacity == 0:       # history=0: no ring, the other fields as usual
            hist = ring[:n]
        else:
            k = steps % self.capacity
            hist = torch.cat([ring[k:], ring[:k]])
        return {"steps": steps, "best_loss": float(s[1]), "best_vertex_rmse": float(s[2]), "total_loss": float(s[3]),
                "vertex_loss": float(s[4]), "existence_loss": float(s[5]), "edge_loss": float(s[6]), "vertex_rmse": float(s[7]),
                "loss_history": hist.tolist()}


class WireframeMeter:
    """Batch-wide training metrics under the loss's assignment, kept on the device (include/wf3d.h, wf3d_train_metrics,
    defines every counter).

    `state` is a float64 [2, 13] device tensor of plain sums, columns `COLUMNS`: row 0 is the latest batch, row 1 the
    running sum since the last `reset()`.  Because every entry is a sum, data-parallel ranks may `all_reduce` `state`
    themselves before `read()`; nothing is exchanged here."""

    COLUMNS = ("updates", "n_samples", "n_pairs", "sum_sq", "sum_dist", "n_within", "ex_tp", "ex_fp", "ex_fn",
               "count_abs_err", "ed_tp", "ed_fp", "ed_fn")

    def __init__(self, device, distance_thresh=0.05, edge_threshold=0.5):
        self.distance_thresh = float(distance_thresh)
        self.edge_threshold = float(edge_threshold)
        self.state = torch.zeros(2, len(self.COLUMNS), dtype=torch.float64, device=device)
        self._ws = None

    @torch.no_grad()
    def update(self, predictions, targets, assignment):
        """predictions: `vertices` [B, V, 3] (any sample / vertex stride, unit inner stride), `existence_probabilities`
        [B, V], `edge_probs` [B, Ep] and, when present, `edge_width` (a padded edge head's one-element int64 width);
        targets: `vertices` [B, Vt, 3], `vertex_existence` [B, V], `edge_labels` [B, Et], `vertex_counts` int64 [B];
        assignment: int32 [B, V] (`WireframeLoss.last_assignment`).  Everything float32 on the device.  No host read;
        the workspace is kept between calls, so after one eager call of a shape the update can be captured."""
        def take(d, k, dtype, shape, what):
            t = d[k].detach()
            if not t.is_cuda:
                raise RuntimeError(f"wf3d.WireframeMeter: {what}['{k}'] must be a device tensor (no CPU fallback)")
            if t.dtype != dtype:
                raise RuntimeError(f"wf3d.WireframeMeter: {what}['{k}'] must be {dtype}, got {t.dtype}")
            if t.dim() != len(shape) or any(s is not None and s != n for s, n in zip(shape, t.shape)):
                want = "[" + ", ".join("*" if s is None else str(s) for s in shape) + "]"
                raise RuntimeError(f"wf3d.WireframeMeter: {what}['{k}'] must be {want}, got {list(t.shape)}")
            return t
        f32 = torch.float32
        pv = take(predictions, "vertices", f32, (None, None, 3), "predictions")
        B, V = pv.shape[0], pv.shape[1]
        if B < 1 or V < 1 or pv.stride(2) != 1:
            raise RuntimeError("wf3d.WireframeMeter: predictions['vertices'] must be a non-empty [B, V, 3] with unit inner stride")
        pe = take(predictions, "existence_probabilities", f32, (B, V), "predictions").contiguous()
        pp = take(predictions, "edge_probs", f32, (B, None), "predictions").contiguous()
        tv = take(targets, "vertices", f32, (B, None, 3), "targets").contiguous()
        te = take(targets, "vertex_existence", f32, (B, V), "targets").contiguous()
        tl = take(targets, "edge_labels", f32, (B, None), "targets").contiguous()
        cnt = take(targets, "vertex_counts", torch.int64, (B,), "targets").contiguous()
        a = take({"assignment": assignment}, "assignment", torch.int32, (B, V), "arguments").contiguous()
        if tv.shape[1] < 1:
            raise RuntimeError("wf3d.WireframeMeter: targets['vertices'] must hold at least one vertex per sample")
        ew = predictions.get("edge_width")
        if ew is not None:
            ew = ew.detach()
            if not ew.is_cuda or ew.dtype != torch.int64 or ew.numel() != 1:
                raise RuntimeError("wf3d.WireframeMeter: predictions['edge_width'] must be a one-element int64 device tensor")
        lib = _lib.load()
        need = lib.wf3d_train_metrics_ws_bytes(B, pp.shape[1])
        if self._ws is None or self._ws.numel() < need or self._ws.device != pv.device:
            self._ws = torch.empty(max(int(need), 256), dtype=torch.uint8, device=pv.device)
        check(lib.wf3d_train_metrics(_p(pv), pv.stride(0), pv.stride(1), _p(pe), _p(pp), pp.shape[1], _p(tv), tv.shape[1],
                                     _p(te), _p(tl), tl.shape[1], _p(a), _p(cnt), _p(ew), B, V, self.edge_threshold,
                                     self.distance_thresh, _p(self.state), _p(self._ws), self._ws.numel(), _stream()),
              "train_metrics")

    def reset(self):
        """Zero the running row on the device (one fill; capturable).  Row 0 keeps the latest batch."""
        self.state[1].zero_()

    @classmethod
    def derive(cls, row):
        """The raw counters of one state row (13 numbers) by name, and the ratios formed from them; a ratio with a zero
        denominator is nan."""
        r = dict(zip(cls.COLUMNS, (float(x) for x in row)))

        def ratio(num, den):
            return num / den if den != 0 else math.nan

        def prf(tp, fp, fn):
            p, q = ratio(tp, tp + fp), ratio(tp, tp + fn)
            return p, q, ratio(2.0 * tp, 2.0 * tp + fp + fn)
        ms = ratio(r["sum_sq"], 3.0 * r["n_pairs"])
        r["matched_rmse"] = math.sqrt(ms) if ms >= 0 else math.nan       # a NaN sum stays NaN
        r["mean_distance"] = ratio(r["sum_dist"], r["n_pairs"])
        r["corner_recall"] = ratio(r["n_within"], r["n_pairs"])
        r["existence_precision"], r["existence_recall"], r["existence_f1"] = prf(r["ex_tp"], r["ex_fp"], r["ex_fn"])
        r["count_mae"] = ratio(r["count_abs_err"], r["n_samples"])
        r["edge_precision"], r["edge_recall"], r["edge_f1"] = prf(r["ed_tp"], r["ed_fp"], r["ed_fn"])
        return r

    def read(self):
        """One device -> host copy: {"last": ..., "running": ...}, each the row's raw counters by name (`COLUMNS`) plus
        matched_rmse = sqrt(sum_sq / (3 n_pairs)), mean_distance = sum_dist / n_pairs, corner_recall = n_within /
        n_pairs, existence_precision / _recall / _f1, count_mae = count_abs_err / n_samples and edge_precision /
        _recall / _f1 (F1 = 2 tp / (2 tp + fp + fn))."""
        s = self.state.cpu().tolist()
        return {"last": self.derive(s[0]), "running": self.derive(s[1])}
