"""Row f-4: evaluation post-processing behind the hot path (reference evaluate.py:74-110) on the device.

    samples = wireframes_from_predictions(model(x))        # ONE kernel + ONE device->host copy for the whole batch
    evaluate_batch(predictions, wf_vertices, wf_edges, ap_calculator)      # the reference's per-sample loop, fed from it

Opt-in, for evaluating a data set: device work and host traffic that scale with the KEPT edges, not with V^2.

    samples = wireframes_compact(model(x))                 # compaction on the device; B + 1 offsets, then K packed rows
    evaluate_batch(..., compact=True)                      # + all Hausdorff matrices of the batch from one launch

Opt-in on top of that: the metrics themselves on the device (csrc/evalmetrics.hip), the labels prepared once.

    labels = EvalLabels(wf_vertices, wf_edges, device)     # once per label set: device copy + edit-distance constants
    evaluate_batch(..., compact=True, metrics="device", labels=labels)     # both assignments, corner sets, counters: 4 launches

Opt-in before any of them: decoding (csrc/evalpost.hip wf3d_wireframe_decode; the specification is wf3d/decode.py).  The
reference hands all V slots to its metrics; this turns a forward pass into vertices that exist, are distinct and are connected.

    samples = decode_wireframes(model(x), merge_radius=0.05)                # existence filter, vertex merging, edge re-indexing
    evaluate_batch(..., decode={"merge_radius": 0.05})                      # any of the three paths above, fed from it

`hausdorff_lines` is the device form of eval.ap_calculator.hausdorff_distance_line (csrc/evalpost.hip)."""
import numpy as np
import torch

from . import _lib, decode as _decode
from ._lib import check
from .functional import edge_index_lists
from .ops import _stream


def hausdorff_lines(p_line, t_line, sample_points, device):
    """[N, M] float64 numpy matrix; p_line [N, 2, 3], t_line [M, 2, 3] numpy arrays (any float dtype).  The segment
    directions are formed in the arrays' common dtype, as the reference's concatenate + subtraction does (:22-26)."""
    N, M = p_line.shape[0], t_line.shape[0]
    both = np.concatenate((p_line, t_line), axis=0)
    start = both[:, 0, :].astype(np.float64)
    diff = (both[:, 1, :] - both[:, 0, :]).astype(np.float64)
    buf = torch.from_numpy(np.ascontiguousarray(np.stack((start, diff)))).to(device)          # [2, N + M, 3]
    out = torch.empty(N, M, dtype=torch.float64, device=device)
    ps, pd = buf[0, :N], buf[1, :N]
    ts, td = buf[0, N:], buf[1, N:]
    check(_lib.load().wf3d_hausdorff_lines(ps.data_ptr(), pd.data_ptr(), ts.data_ptr(), td.data_ptr(), N, M, int(sample_points),
                                           out.data_ptr(), _stream()), "hausdorff_lines")
    return out.cpu().numpy()


def wireframes_from_predictions(predictions, threshold=0.5):
    """Per sample: dict(pred_vertices [V, 3] float32, pd_edges [k, 2] int64, pd_edges_vertices [k, 2, 3] float32) — the
    edges whose probability exceeds `threshold`, end points ordered higher-z first (evaluate.py:74-92)."""
    verts, probs = predictions["vertices"], predictions["edge_probs"]
    B, V, _ = verts.shape
    lists = predictions["edge_indices"]
    counts = [int(round((1 + (1 + 8 * len(e)) ** 0.5) / 2)) if len(e) else 0 for e in lists]
    max_e = probs.shape[1]
    dev = verts.device
    v = verts.detach().float()
    if v.stride(2) != 1:
        v = v.contiguous()
    ev = torch.zeros(B, max_e, 2, 3, dtype=torch.float32, device=dev)
    keep = torch.zeros(B, max_e, dtype=torch.uint8, device=dev)
    cnt = torch.tensor(counts, dtype=torch.int32).to(dev)
    pr = probs.detach().float().contiguous()
    check(_lib.load().wf3d_edge_endpoints(v.data_ptr(), v.stride(0), v.stride(1), cnt.data_ptr(), pr.data_ptr(), B, V, max_e,
                                          float(threshold), ev.data_ptr(), keep.data_ptr(), _stream()), "edge_endpoints")
    # one packed device->host transfer for the batch
    packed = torch.cat([v.reshape(B, -1) if v.is_contiguous() else v.contiguous().reshape(B, -1), ev.reshape(B, -1), keep.float()], dim=1).cpu().numpy()
    nv, ne = V * 3, max_e * 6
    out = []
    for s in range(B):
        row = packed[s]
        mask = row[nv + ne:] > 0.5
        idx = np.array(lists[s], dtype=np.int64).reshape(-1, 2)
        m = mask[:len(idx)]
        out.append({"pred_vertices": row[:nv].reshape(V, 3).copy(),
                    "pd_edges": idx[m],
                    "pd_edges_vertices": row[nv:nv + ne].reshape(max_e, 2, 3)[:len(idx)][m].copy()})
    return out


def _gt_edge_vertices(gt_vertices, gt_edges):
    if len(gt_edges) == 0:
        return np.empty((0, 2, 3))
    ev = np.stack((gt_vertices[gt_edges[:, 0]], gt_vertices[gt_edges[:, 1]]), axis=1)
    return ev[np.arange(ev.shape[0])[:, np.newaxis], np.flip(np.argsort(ev[:, :, -1]), axis=1)]


def _vertex_counts(predictions, dev):
    """int32 [B] on `dev`: `edge_counts` when the dict has it (padded edge layout; nothing of it is read on the host), else
    each count from len(edge_indices[s])."""
    if predictions.get("edge_counts") is not None:
        return predictions["edge_counts"].detach().to(device=dev, dtype=torch.int32)
    lens = [len(e) for e in predictions["edge_indices"]]
    return torch.tensor([int(round((1 + (1 + 8 * n) ** 0.5) / 2)) if n else 0 for n in lens], dtype=torch.int32).to(dev)


def wireframes_compact(predictions, threshold=0.5, keep_device=False):
    """wireframes_from_predictions with the kept edges compacted on the device (wf3d_edge_compact): the same list of
    per-sample dicts (equal values, dtypes and shapes, the empty (0, 2) / (0, 2, 3) included) plus `pd_edge_probs`
    float32 [k].  The host reads the B + 1 offsets `koff` (the one extra synchronisation), then one buffer of the
    vertices and the first K = koff[B] packed rows: 12 B V + 36 K bytes instead of B (3 V + 7 max_e) 4.
    The contents of `edge_indices` are never touched: with `edge_counts` in the dict (padded edge layout) the counts are
    that device tensor and nothing of it is read on the host; otherwise each count comes from len(edge_indices[s]).
    keep_device=True: returns (samples, {"koff": int32 [B + 1], "seg": float32 [B * max_e, 2, 3] (first K rows valid),
    "koff_host": numpy int32 [B + 1]}) — the device tensors wf3d_hausdorff_lines_batch takes."""
    verts, probs = predictions["vertices"], predictions["edge_probs"]
    B, V, _ = verts.shape
    max_e = probs.shape[1]
    dev = verts.device
    cnt = _vertex_counts(predictions, dev)
    v = verts.detach().float()
    if v.stride(2) != 1:
        v = v.contiguous()
    pr = probs.detach().float().contiguous()
    lib = _lib.load()
    cap = B * max_e
    koff = torch.empty(B + 1, dtype=torch.int32, device=dev)
    pairs = torch.empty(cap, 2, dtype=torch.int32, device=dev)
    seg = torch.empty(cap, 2, 3, dtype=torch.float32, device=dev)
    kprob = torch.empty(cap, dtype=torch.float32, device=dev)
    ws_bytes = lib.wf3d_edge_compact_ws_bytes(B, max_e)
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.int32, device=dev)
    check(lib.wf3d_edge_compact(v.data_ptr(), v.stride(0), v.stride(1), cnt.data_ptr(), pr.data_ptr(), B, V, max_e,
                                float(threshold), koff.data_ptr(), pairs.data_ptr(), seg.data_ptr(), kprob.data_ptr(),
                                ws.data_ptr(), ws_bytes, _stream()), "edge_compact")
    koff_h = koff.cpu().numpy()
    K = int(koff_h[B])
    # one packed device->host transfer: vertices | pairs | segments | probabilities, as raw 32-bit words
    words = torch.cat([v.reshape(-1).view(torch.int32), pairs[:K].reshape(-1), seg[:K].reshape(-1).view(torch.int32),
                       kprob[:K].view(torch.int32)]).cpu().numpy()
    nv = B * V * 3
    pv = words[:nv].view(np.float32).reshape(B, V, 3)
    pe = words[nv:nv + 2 * K].reshape(K, 2).astype(np.int64)
    ps = words[nv + 2 * K:nv + 8 * K].view(np.float32).reshape(K, 2, 3)
    pp = words[nv + 8 * K:].view(np.float32)
    out = []
    for s in range(B):
        a, b = int(koff_h[s]), int(koff_h[s + 1])
        out.append({"pred_vertices": pv[s].copy(), "pd_edges": pe[a:b].copy(), "pd_edges_vertices": ps[a:b].copy(),
                    "pd_edge_probs": pp[a:b].copy()})
    if keep_device:
        return out, {"koff": koff, "seg": seg, "koff_host": koff_h}
    return out


DECODE_OPTIONS = ("existence_threshold", "edge_threshold", "merge_radius", "drop_isolated")


def decode_wireframes(predictions, existence_threshold=0.5, edge_threshold=0.5, merge_radius=None, drop_isolated=False,
                      keep_device=False):
    """One forward pass -> per sample a wireframe of vertices that exist, are distinct and are connected (the steps and
    every tie rule: wf3d/decode.py).  Slots whose `existence_probabilities` do not exceed `existence_threshold` (None: no
    test) are dropped, slots within `merge_radius` of a more probable one are merged into it (None: no merging), the
    candidate edges above `edge_threshold` are re-indexed onto the surviving vertices, and drop_isolated=True keeps only
    vertices with an edge.  Returns the per-sample dict list of wireframes_compact plus `slots` (int64 [n_s], the source
    slot of each vertex); `pred_vertices` is [n_s, 3] and `pd_edges` index into it.  The counts come from `edge_counts`
    when present, else from len(edge_indices[s]), as in wireframes_compact.
    CUDA predictions run wf3d_wireframe_decode (four launches), then one synchronisation for koff | nverts | status and
    one packed copy; CPU predictions run the numpy specification.  Both return equal values.
    keep_device=True (CUDA predictions only, else ValueError): returns (samples, {"koff", "seg", "dverts", "nverts", "status": tensors on the predictions' device,
    "koff_host", "status_host": numpy}) — what wf3d_hausdorff_lines_batch and wf3d_eval_metrics_nv take."""
    if edge_threshold is None:
        raise ValueError("decode_wireframes: edge_threshold must be a number")
    for name, t in (("existence_threshold", existence_threshold), ("edge_threshold", edge_threshold), ("merge_radius", merge_radius)):
        if t is not None and np.isnan(t):
            raise ValueError(f"decode_wireframes: {name} is NaN")
    verts, probs = predictions["vertices"], predictions["edge_probs"]
    B, V, _ = verts.shape
    max_e = probs.shape[1]
    dev = verts.device
    if keep_device and dev.type == "cpu":
        raise ValueError("decode_wireframes: keep_device=True needs CUDA predictions (its tensors feed the batched kernels)")
    cnt = _vertex_counts(predictions, dev)
    ex = predictions["existence_probabilities"].detach().float()
    if tuple(ex.shape) != (B, V):
        raise ValueError(f"decode_wireframes: existence_probabilities must be [B, V] = {(B, V)}, got {tuple(ex.shape)}")
    v = verts.detach().float()
    pr = probs.detach().float().contiguous()
    if dev.type == "cpu":
        d = _decode.decode_batch(v.numpy(), ex.numpy(), pr.numpy(), cnt.numpy(), existence_threshold=existence_threshold,
                                 edge_threshold=edge_threshold, merge_radius=merge_radius, drop_isolated=drop_isolated)
        koff_h, nv_h, st_h = d["koff"], d["nverts"], d["status"]
        pv, sl, pe, ps, pp = d["dverts"], d["slots"], d["pairs"].astype(np.int64), d["seg"], d["kprob"]
    else:
        if v.stride(2) != 1:
            v = v.contiguous()
        # the kernel reads a [B, V] existence array of one element stride: a column of a [B, V, k] tensor passes as it is
        se = ex.stride(1) if V > 1 else (ex.stride(0) if B > 1 else 1)
        if B * V > 0 and not (se >= 1 and (B == 1 or ex.stride(0) == V * se)):
            ex, se = ex.contiguous(), 1
        lib = _lib.load()
        cap = B * max_e
        head = torch.empty(3 * B + 1, dtype=torch.int32, device=dev)         # koff [B + 1] | nverts [B] | status [B]
        koff, nverts, status = head[:B + 1], head[B + 1:2 * B + 1], head[2 * B + 1:]
        dverts = torch.empty(B, V, 3, dtype=torch.float32, device=dev)
        slots = torch.empty(B, V, dtype=torch.int32, device=dev)
        pairs = torch.empty(cap, 2, dtype=torch.int32, device=dev)
        seg = torch.empty(cap, 2, 3, dtype=torch.float32, device=dev)
        kprob = torch.empty(cap, dtype=torch.float32, device=dev)
        ws_bytes = lib.wf3d_wireframe_decode_ws_bytes(B, V, max_e)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        check(lib.wf3d_wireframe_decode(v.data_ptr(), v.stride(0), v.stride(1), ex.data_ptr(), se, cnt.data_ptr(), pr.data_ptr(),
                                        B, V, max_e, float("-inf") if existence_threshold is None else float(existence_threshold),
                                        float(edge_threshold), -1.0 if merge_radius is None else float(merge_radius),
                                        int(bool(drop_isolated)), nverts.data_ptr(), dverts.data_ptr(), slots.data_ptr(),
                                        koff.data_ptr(), pairs.data_ptr(), seg.data_ptr(), kprob.data_ptr(), status.data_ptr(),
                                        ws.data_ptr(), ws_bytes, _stream()), "wireframe_decode")
        head_h = head.cpu().numpy()                                          # the one synchronisation
        koff_h, nv_h, st_h = head_h[:B + 1], head_h[B + 1:2 * B + 1], head_h[2 * B + 1:]
        K = int(koff_h[B])
        # one packed device->host transfer: vertices | slots | pairs | segments | probabilities, as raw 32-bit words
        words = torch.cat([dverts.reshape(-1).view(torch.int32), slots.reshape(-1), pairs[:K].reshape(-1),
                           seg[:K].reshape(-1).view(torch.int32), kprob[:K].view(torch.int32)]).cpu().numpy()
        nv, ns = B * V * 3, B * V
        pv = words[:nv].view(np.float32).reshape(B, V, 3)
        sl = words[nv:nv + ns].reshape(B, V)
        o = nv + ns
        pe = words[o:o + 2 * K].reshape(K, 2).astype(np.int64)
        ps = words[o + 2 * K:o + 8 * K].view(np.float32).reshape(K, 2, 3)
        pp = words[o + 8 * K:].view(np.float32)
        keep = {"koff": koff, "seg": seg, "dverts": dverts, "nverts": nverts, "status": status}
    out = []
    for s in range(B):
        a, b, n = int(koff_h[s]), int(koff_h[s + 1]), int(nv_h[s])
        out.append({"pred_vertices": pv[s, :n].copy(), "pd_edges": pe[a:b].copy(), "pd_edges_vertices": ps[a:b].copy(),
                    "pd_edge_probs": pp[a:b].copy(), "slots": sl[s, :n].astype(np.int64)})
    if keep_device:
        return out, dict(keep, koff_host=koff_h, status_host=st_h)
    return out


def _decoded(predictions, threshold, decode):
    """(samples, device dict) of the batch: wireframes_compact, or decode_wireframes under the `decode` options."""
    if decode is None:
        return wireframes_compact(predictions, threshold, keep_device=True)
    return decode_wireframes(predictions, **decode, keep_device=True)


def _as_numpy(x):
    return x.numpy() if torch.is_tensor(x) else np.asarray(x)


def _compute_sample(ap_calculator, w, gt_v, gt_e, gt_ev, hd):
    """compute_metrics on one sample of wireframes_compact with its Hausdorff matrix (None: compute_metrics makes it)."""
    pd_ev = w["pd_edges_vertices"] if len(w["pd_edges"]) > 0 else np.empty((0, 2, 3))
    ap_calculator.compute_metrics({"predicted_vertices": w["pred_vertices"][np.newaxis, :],
                                   "predicted_edges": w["pd_edges"][np.newaxis, :],
                                   "pred_edges_vertices": pd_ev.reshape((1, -1, 2, 3)),
                                   "wf_vertices": gt_v[np.newaxis, :],
                                   "wf_edges": gt_e[np.newaxis, :],
                                   "wf_edges_vertices": gt_ev.reshape((1, -1, 2, 3)),
                                   "hausdorff": [hd]})


def _evaluate_batch_compact(predictions, wf_vertices, wf_edges, ap_calculator, threshold, sample_points=20, decode=None):
    """evaluate_batch on the compacted edges: every sample's Hausdorff matrix from ONE launch over the segments that
    wireframes_compact (or, with `decode`, decode_wireframes) left on the device, the label segments uploaded once, the
    matrices read back in one copy."""
    samples, d = _decoded(predictions, threshold, decode)
    B = len(samples)
    dev = d["seg"].device
    n = np.diff(d["koff_host"]).astype(np.int64)
    gt = []
    m = np.zeros(B, dtype=np.int64)
    for s in range(B):
        gt_v, gt_e = _as_numpy(wf_vertices[s]), _as_numpy(wf_edges[s]).astype(np.int64)
        gt_ev = _gt_edge_vertices(gt_v, gt_e)
        gt.append((gt_v, gt_e, gt_ev))
        if n[s] > 0 and gt_ev.dtype == np.float32:            # else: compute_metrics computes this sample's matrix itself
            m[s] = gt_ev.shape[0]
    ooff = np.concatenate(([0], np.cumsum(n * m)))
    loff = np.concatenate(([0], np.cumsum(m)))
    hd = [None] * B
    if ooff[-1] > 0:
        if loff[-1] >= 2 ** 31:
            raise ValueError("evaluate_batch(compact=True): more than 2^31 label segments in one batch")
        lseg = np.concatenate([g[2].reshape(-1) for s, g in enumerate(gt) if m[s] > 0])
        # one upload: ooff (int64, 8-byte aligned at the front) | loff | label segments, as raw 32-bit words
        up = torch.from_numpy(np.concatenate((ooff.astype(np.int64).view(np.int32), loff.astype(np.int32),
                                              lseg.view(np.int32)))).to(dev)
        n_o = 2 * (B + 1)
        d_ooff, d_loff, d_lseg = up[:n_o].view(torch.int64), up[n_o:n_o + B + 1], up[n_o + B + 1:].view(torch.float32)
        out = torch.empty(int(ooff[-1]), dtype=torch.float64, device=dev)
        check(_lib.load().wf3d_hausdorff_lines_batch(d["seg"].data_ptr(), d["koff"].data_ptr(), d_lseg.data_ptr(),
                                                     d_loff.data_ptr(), d_ooff.data_ptr(), B, int((n * m).max()),
                                                     int(sample_points), out.data_ptr(), _stream()), "hausdorff_lines_batch")
        flat = out.cpu().numpy()
        hd = [flat[ooff[s]:ooff[s + 1]].reshape(n[s], m[s]) if n[s] * m[s] > 0 else None for s in range(B)]
    for s, w in enumerate(samples):
        _compute_sample(ap_calculator, w, *gt[s], hd[s])


class EvalLabels:
    """The labels of a batch (or of a whole data set) as evaluate_batch(metrics="device") needs them, built once and
    reused across batches and epochs:
      * the host arrays (`verts`, `edges`, `segs`: per sample the label vertices, the int64 edges and the
        _gt_edge_vertices segments) for the samples that take the host call;
      * ONE device upload: label vertices, label segments and their offsets (`lvoff`, `loff`, `lverts`, `lseg`);
      * per sample the label-only constants (wed_e, s, total) of the wireframe edit distance.  compute_metrics calls
        graph_edit_distance on the label's own points and edges, so the prediction enters only through the scalar
        `distances`: wed = (wed_e + (distances + s)) / total, in that association, is the reference's value exactly.
    `host[s]`: the sample's label vertices are not float32 or its label has no edge; it is evaluated by today's
    per-sample call (and contributes no vertex or segment to the upload).
    labels[indices] is the EvalLabels of those samples, in that order: equal to a fresh build, without recomputing the
    constants."""

    def __init__(self, wf_vertices, wf_edges, device, _parts=None):
        from eval.ap_calculator import computer_edges, edit_distance_terms
        self.device = torch.device(device)
        if _parts is not None:
            self.verts, self.edges, self.segs, self.consts = _parts
        else:
            self.verts = [_as_numpy(v) for v in wf_vertices]
            self.edges = [_as_numpy(e).astype(np.int64) for e in wf_edges]
            self.segs = [_gt_edge_vertices(v, e) for v, e in zip(self.verts, self.edges)]
            self.consts = []
            for gt_v, gt_e, gt_ev in zip(self.verts, self.edges, self.segs):
                if len(gt_e) == 0:
                    self.consts.append(None)
                    continue
                label_pts = np.unique(gt_ev.reshape(-1, 3), axis=0)
                self.consts.append(edit_distance_terms(label_pts, computer_edges(gt_ev, label_pts).copy(), gt_v.copy(),
                                                       gt_e.copy(), 0))
        B = len(self.verts)
        self.host = np.array([v.dtype != np.float32 or len(e) == 0 for v, e in zip(self.verts, self.edges)], dtype=bool)
        self.nverts = np.array([0 if h else len(v) for v, h in zip(self.verts, self.host)], dtype=np.int64)
        self.nsegs = np.array([0 if h else len(g) for g, h in zip(self.segs, self.host)], dtype=np.int64)
        lvoff, loff = np.concatenate(([0], np.cumsum(self.nverts))), np.concatenate(([0], np.cumsum(self.nsegs)))
        if lvoff[-1] >= 2 ** 31 or loff[-1] >= 2 ** 31:
            raise ValueError("EvalLabels: more than 2^31 label vertices or segments")
        keep = [s for s in range(B) if not self.host[s]]
        words = [lvoff.astype(np.int32), loff.astype(np.int32)]
        words += [np.ascontiguousarray(self.verts[s]).reshape(-1).view(np.int32) for s in keep]
        words += [np.ascontiguousarray(self.segs[s]).reshape(-1).view(np.int32) for s in keep]
        up = torch.from_numpy(np.concatenate(words)).to(self.device)     # one upload, as raw 32-bit words
        nv, ns = 3 * int(lvoff[-1]), 6 * int(loff[-1])
        self.lvoff, self.loff = up[:B + 1], up[B + 1:2 * B + 2]
        self.lverts = up[2 * B + 2:2 * B + 2 + nv].view(torch.float32)
        self.lseg = up[2 * B + 2 + nv:2 * B + 2 + nv + ns].view(torch.float32)

    def __len__(self):
        return len(self.verts)

    def __getitem__(self, indices):
        idx = [int(i) for i in (range(*indices.indices(len(self))) if isinstance(indices, slice) else indices)]
        return EvalLabels(None, None, self.device, _parts=tuple([part[i] for i in idx] for part in
                                                                (self.verts, self.edges, self.segs, self.consts)))

    def wed(self, s, distances):
        """The reference's wireframe edit distance of sample s given its corner distance sum."""
        wed_e, snap, total = self.consts[s]
        return (wed_e + (distances + snap)) / total


def _evaluate_batch_device(predictions, wf_vertices, wf_edges, ap_calculator, threshold, labels, sample_points=20, decode=None):
    """evaluate_batch(compact=True) with everything that follows the Hausdorff matrices on the device too
    (wf3d_eval_metrics): the matrices stay there, [B] distances and [B, 8] counters come back in one copy.  With `decode`
    the vertices are the decoded ones, each sample with its own count (wf3d_eval_metrics_nv), and a sample whose decode
    status is not zero takes the per-sample host call."""
    if labels is None:
        labels = EvalLabels(wf_vertices, wf_edges, predictions["vertices"].device)
    samples, d = _decoded(predictions, threshold, decode)
    B = len(samples)
    dev = d["seg"].device
    if len(labels) != B or labels.device != dev:
        raise ValueError(f"evaluate_batch(metrics='device'): labels of {len(labels)} samples on {labels.device} for a batch "
                         f"of {B} on {dev}")
    if decode is None:
        verts = predictions["vertices"].detach().float()
        if verts.stride(2) != 1:
            verts = verts.contiguous()
    else:
        verts = d["dverts"]
    V = verts.shape[1]
    n = np.diff(d["koff_host"]).astype(np.int64)
    m = labels.nsegs
    ooff = np.concatenate(([0], np.cumsum(n * m)))
    aoff = np.concatenate(([0], np.cumsum(np.minimum(n, m))))
    if aoff[-1] >= 2 ** 31:
        raise ValueError("evaluate_batch(metrics='device'): more than 2^31 assignment entries in one batch")
    lib = _lib.load()
    # one upload: ooff (int64, 8-byte aligned at the front) | aoff, as raw 32-bit words
    up = torch.from_numpy(np.concatenate((ooff.astype(np.int64).view(np.int32), aoff.astype(np.int32)))).to(dev)
    d_ooff, d_aoff = up[:2 * (B + 1)].view(torch.int64), up[2 * (B + 1):]
    hd = torch.empty(max(int(ooff[-1]), 1), dtype=torch.float64, device=dev)
    if ooff[-1] > 0:
        check(lib.wf3d_hausdorff_lines_batch(d["seg"].data_ptr(), d["koff"].data_ptr(), labels.lseg.data_ptr(),
                                             labels.loff.data_ptr(), d_ooff.data_ptr(), B, int((n * m).max()),
                                             int(sample_points), hd.data_ptr(), _stream()), "hausdorff_lines_batch")
    assign = torch.empty(max(int(aoff[-1]), 1), dtype=torch.int32, device=dev)
    out = torch.empty(2 * B + 8 * B, dtype=torch.int32, device=dev)      # [B] float64 distances | [B, 8] int32 counters
    total_lv, max_lv = int(labels.nverts.sum()), int(labels.nverts.max()) if B else 0
    max_long = int(max(n.max(), m.max())) if B else 0
    ws_bytes = lib.wf3d_eval_metrics_ws_bytes(B, V, total_lv, max_long)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    tail = (d["seg"].data_ptr(), d["koff"].data_ptr(), labels.lverts.data_ptr(), labels.lvoff.data_ptr(), labels.lseg.data_ptr(),
            labels.loff.data_ptr(), hd.data_ptr(), d_ooff.data_ptr(), d_aoff.data_ptr(), assign.data_ptr(),
            float(ap_calculator.distance_thresh), max_lv, total_lv, max_long, out[2 * B:].data_ptr(), out.data_ptr(),
            ws.data_ptr(), ws_bytes, _stream())
    if decode is None:
        check(lib.wf3d_eval_metrics(verts.data_ptr(), verts.stride(0), verts.stride(1), B, V, *tail), "eval_metrics")
    else:
        check(lib.wf3d_eval_metrics_nv(verts.data_ptr(), verts.stride(0), verts.stride(1), B, V, d["nverts"].data_ptr(), *tail),
              "eval_metrics_nv")
    flagged = np.zeros(B, dtype=bool) if decode is None else d["status_host"] != 0
    words = out.cpu().numpy()                                            # the one copy back
    dist, cnt = words[:2 * B].view(np.float64), words[2 * B:].reshape(B, 8)
    names = ("tp_corners", "tp_fp_corners", "tp_fn_corners", "tp_edges", "tp_fp_edges", "tp_fn_edges")
    for s, w in enumerate(samples):
        if labels.host[s] or cnt[s, 6] != 0 or flagged[s]:
            # today's per-sample call, with the sample's own matrix where the batch launch made one
            mat = hd[ooff[s]:ooff[s + 1]].cpu().numpy().reshape(n[s], m[s]) if n[s] * m[s] > 0 else None
            _compute_sample(ap_calculator, w, labels.verts[s], labels.edges[s], labels.segs[s], mat)
            continue
        ap_calculator.batch_size = 1
        for k, name in enumerate(names):
            ap_calculator.ap_dict[name] += int(cnt[s, k])
        ap_calculator.ap_dict["distance"] += dist[s]
        ap_calculator.ap_dict["wed"] += labels.wed(s, dist[s]) if n[s] > 0 else 1


def evaluate_batch(predictions, wf_vertices, wf_edges, ap_calculator, threshold=None, compact=False, metrics="host", labels=None,
                   decode=None):
    """The body of the reference's evaluation loop (evaluate.py:74-110) for one batch: `wf_vertices` / `wf_edges` are the
    collate_batch lists of tensors; accumulates into `ap_calculator`.
    compact=True: the kept edges are compacted on the device (wireframes_compact) and all Hausdorff matrices of the batch
    come from one launch (wf3d_hausdorff_lines_batch) and one copy each way; `ap_calculator.compute_metrics` receives
    them as batch["hausdorff"].  Three kinds of sample silently take today's per-sample call instead: one that keeps no
    edge (the corners-only branch needs no matrix), one whose label has no edge, and one whose label vertices are not
    float32 (the batched kernel forms the segment directions in float32, which is the common dtype only then).
    metrics="device" (with compact=True): the two assignments, the corner sets, the counters and the corner distance sum
    of every sample come from the device as well (wf3d_eval_metrics; csrc/evalmetrics.hip), the Hausdorff matrices are not
    copied back, and `labels` may be an EvalLabels built once for these samples (else one is built here from
    wf_vertices / wf_edges, which are otherwise unused).  A sample the device flags (a non-finite value, kept edges of
    which none matches — the reference raises there, and so does this —, a matched end point that is no vertex row), one
    whose label vertices are not float32 and one whose label has no edge take today's per-sample call.  Where a sample's
    optimal assignment is not unique, the device's choice (the tie rule of tests/lsa_model.py) may differ from scipy's.
    threshold: the edge probability threshold, 0.5 when not given.
    decode: None (today's paths, unchanged: every one of the V slots is a predicted corner, as in the reference) or a dict
    of decode_wireframes' options (DECODE_OPTIONS).  The batch is then decoded once and every path is fed from the decoded
    wireframes: the per-sample host call and compact=True from the decoded samples (the Hausdorff matrices from the
    decoded segments), metrics="device" from the decoded vertices with each sample's own count (wf3d_eval_metrics_nv); a
    sample the decode flags (a non-finite slot) takes the per-sample host call there.  `threshold` and
    decode["edge_threshold"] given together and different: ValueError.  CPU predictions decode through the numpy
    specification (compact=False only)."""
    if metrics not in ("host", "device"):
        raise ValueError(f"evaluate_batch: metrics must be 'host' or 'device' (got {metrics!r})")
    if decode is not None:
        unknown = sorted(set(decode) - set(DECODE_OPTIONS))
        if unknown:
            raise ValueError(f"evaluate_batch: unknown decode option(s) {unknown}; the options are {DECODE_OPTIONS}")
        if threshold is not None and "edge_threshold" in decode and decode["edge_threshold"] != threshold:
            raise ValueError(f"evaluate_batch: threshold={threshold!r} and decode['edge_threshold']={decode['edge_threshold']!r} differ")
        decode = dict(decode)
        if threshold is not None:
            decode["edge_threshold"] = threshold
    if threshold is None:
        threshold = 0.5
    if metrics == "device":
        if not compact:
            raise ValueError("evaluate_batch: metrics='device' needs compact=True")
        return _evaluate_batch_device(predictions, wf_vertices, wf_edges, ap_calculator, threshold, labels, decode=decode)
    if compact:
        return _evaluate_batch_compact(predictions, wf_vertices, wf_edges, ap_calculator, threshold, decode=decode)
    if decode is not None:
        for s, w in enumerate(decode_wireframes(predictions, **decode)):
            gt_v, gt_e = _as_numpy(wf_vertices[s]), _as_numpy(wf_edges[s]).astype(np.int64)
            _compute_sample(ap_calculator, w, gt_v, gt_e, _gt_edge_vertices(gt_v, gt_e), None)
        return
    for s, w in enumerate(wireframes_from_predictions(predictions, threshold)):
        gt_v = wf_vertices[s].numpy() if torch.is_tensor(wf_vertices[s]) else np.asarray(wf_vertices[s])
        gt_e = (wf_edges[s].numpy() if torch.is_tensor(wf_edges[s]) else np.asarray(wf_edges[s])).astype(np.int64)
        pd_ev = w["pd_edges_vertices"] if len(w["pd_edges"]) > 0 else np.empty((0, 2, 3))
        batch = {"predicted_vertices": w["pred_vertices"][np.newaxis, :],
                 "predicted_edges": w["pd_edges"][np.newaxis, :],
                 "pred_edges_vertices": pd_ev.reshape((1, -1, 2, 3)),
                 "wf_vertices": gt_v[np.newaxis, :],
                 "wf_edges": gt_e[np.newaxis, :],
                 "wf_edges_vertices": _gt_edge_vertices(gt_v, gt_e).reshape((1, -1, 2, 3))}
        ap_calculator.compute_metrics(batch)
