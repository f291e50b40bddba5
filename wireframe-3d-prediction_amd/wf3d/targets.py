"""The training targets of train.py (:50-88 existence and edge labels, :112-115 target vertices) built in one pass on
the host, for a batch of ground-truth wireframes.

train_targets(wf_vertices, wf_edges, max_vertices) returns the dict train.py hands to WireframeLoss:
  vertices          [B, max_vertices, 3] float32, sample s's c_s vertices first, zeros after
  vertex_existence  [B, max_vertices] float32, 1.0 for the first c_s entries
  edge_labels       [B, max_s c_s(c_s-1)/2] float32: label of pair (i, j), i < j < c_s, in the reference's
                    lexicographic pair order is 1.0 iff the wireframe has the edge (either direction)
  vertex_counts     [B] int64, c_s = len(wf_vertices[s])
full_width=True: edge_labels is [B, max_vertices(max_vertices-1)/2], the same labels zero-extended — every batch has
the same shapes, so that a loop can copy_ each batch into the static target buffers of a captured training step (the
loss of a padded edge head only reads the first min(edge width, label width) columns).

matched_edge_labels(edge_labels, assignment, vertex_counts, width, pair_counts=None) moves those labels from the ground
truth's pair order to the pair order of the predicted slots under an assignment: the numpy specification of
WireframeLoss(edge_targets="matched") and of its kernel, wf3d.ops.edge_labels_matched."""
import numpy as np
import torch


def _pair_index(i, j, c):
    """Position of pair (i, j), i < j < c, in the lexicographic order of all pairs of c vertices."""
    return i * c - i * (i + 1) // 2 + (j - i - 1)


def _pair_unrank(k, d):
    """The inverse of `_pair_index` on arrays: (p, q) with p < q < d and _pair_index(p, q, d) == k, for 0 <= k < d(d-1)/2
    and d <= 1024.  Closed form as the kernel evaluates it: p ~ ((2d-1) - sqrt((2d-1)^2 - 8k)) / 2 with the square root
    in float32 — its argument is an integer below 2^24, so the estimate is off by at most one — and one integer step
    either way."""
    k, d = np.asarray(k, np.int64), np.asarray(d, np.int64)
    b = 2 * d - 1

    def start(i):                 # _pair_index(i, i + 1, d): the first pair of row i
        return i * (2 * d - i - 1) // 2
    p = ((b.astype(np.float32) - np.sqrt((b * b - 8 * k).astype(np.float32))) * np.float32(0.5)).astype(np.int64)
    p = np.clip(p, 0, np.maximum(d - 2, 0))
    up = start(p + 1) <= k
    p = np.where(up, p + 1, np.where(start(p) > k, p - 1, p))
    return p, k - start(p) + p + 1


def matched_edge_labels(edge_labels, assignment, vertex_counts, width, pair_counts=None):
    """The edge labels under an assignment (the specification of wf3d_edge_labels_matched, include/wf3d.h): column k of a
    prediction row is the pair (p, q) of predicted SLOTS, and its label is that of the pair of ground-truth vertices the
    two slots are matched to.

    edge_labels [B, Et]: sample b's labels in the pair order of its c_b vertices (what train_targets writes);
    assignment [B, V] integers: slot p is matched to target assignment[b, p] iff 0 <= assignment[b, p] < c_b;
    vertex_counts [B]: c_b, clamped to 0..V; pair_counts [B]: d_b, the count whose pair order the PREDICTION row has,
    clamped to 0..V (None: c_b).  Returns float32 [B, width]: for k < d_b(d_b-1)/2 with (p, q) = pair k of d_b vertices,
    the label at _pair_index(min, max, c_b) of the two targets when both slots are matched, to different targets, and
    that index is below Et; 0 everywhere else."""
    tl = np.asarray(edge_labels, np.float32)
    a = np.asarray(assignment, np.int64)
    B, V = a.shape
    Et = tl.shape[1]
    c = np.clip(np.asarray(vertex_counts, np.int64), 0, V)[:, None]
    d = c if pair_counts is None else np.clip(np.asarray(pair_counts, np.int64), 0, V)[:, None]
    out = np.zeros((B, width), np.float32)
    if width == 0 or Et == 0 or B == 0:
        return out
    k = np.arange(width, dtype=np.int64)[None, :]
    live = k < d * (d - 1) // 2
    p, q = _pair_unrank(np.where(live, k, 0), np.maximum(d, 2))       # dead columns: any pair in range
    tp = np.take_along_axis(a, np.minimum(p, V - 1), axis=1)
    tq = np.take_along_axis(a, np.minimum(q, V - 1), axis=1)
    ok = live & (tp >= 0) & (tp < c) & (tq >= 0) & (tq < c) & (tp != tq)
    idx = _pair_index(np.minimum(tp, tq), np.maximum(tp, tq), c)
    ok &= idx < Et
    out[ok] = np.take_along_axis(tl, np.where(ok, idx, 0), axis=1)[ok]
    return out


def train_targets(wf_vertices, wf_edges, max_vertices, device=None, full_width=False):
    B = len(wf_vertices)
    if len(wf_edges) != B:
        raise ValueError(f"{B} vertex sets but {len(wf_edges)} edge sets")
    counts = [len(v) for v in wf_vertices]
    if any(c > max_vertices for c in counts):
        # train.py:115 assigns c_s rows into max_vertices of them and fails there too
        raise ValueError(f"a wireframe has {max(counts)} vertices, more than max_vertices = {max_vertices}")
    width = max_vertices * (max_vertices - 1) // 2 if full_width else max((c * (c - 1) // 2 for c in counts), default=0)
    verts = np.zeros((B, max_vertices, 3), np.float32)
    exist = np.zeros((B, max_vertices), np.float32)
    labels = np.zeros((B, width), np.float32)
    for s, (v, e, c) in enumerate(zip(wf_vertices, wf_edges, counts)):
        if c:
            verts[s, :c] = np.asarray(v, dtype=np.float32).reshape(c, -1)[:, :3]
        exist[s, :c] = 1.0
        e = np.asarray(e, dtype=np.int64).reshape(-1, 2)
        if len(e):
            i, j = np.minimum(e[:, 0], e[:, 1]), np.maximum(e[:, 0], e[:, 1])
            keep = (i >= 0) & (i < j) & (j < c)          # pairs the reference's candidate list holds
            labels[s, _pair_index(i[keep], j[keep], c)] = 1.0
    out = {"vertices": torch.from_numpy(verts), "vertex_existence": torch.from_numpy(exist),
           "edge_labels": torch.from_numpy(labels), "vertex_counts": torch.tensor(counts, dtype=torch.int64)}
    return {k: t.to(device) for k, t in out.items()} if device is not None else out
