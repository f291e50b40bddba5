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
loss of a padded edge head only reads the first min(edge width, label width) columns)."""
import numpy as np
import torch


def _pair_index(i, j, c):
    """Position of pair (i, j), i < j < c, in the lexicographic order of all pairs of c vertices."""
    return i * c - i * (i + 1) // 2 + (j - i - 1)


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
