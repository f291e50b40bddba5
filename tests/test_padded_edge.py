"""CPU side of the padded edge head: the train.py targets helper (wf3d.targets) against an inline rebuild of
train.py:50-88,112-115 on the golden wireframes, its full-width form, and the lazy edge_indices sequence of a padded
forward (wf3d.functional.EdgeIndexLists)."""
import os

import numpy as np
import pytest
import torch

import helpers as H

ROOT = os.path.join(H.GOLDEN, "building3d")
WIREFRAMES = [os.path.join(ROOT, "train", "wireframe", "100.obj"), os.path.join(ROOT, "train", "wireframe", "10040.obj"),
              os.path.join(ROOT, "test", "wireframe", "10024.obj")]


def _golden_batch():
    from datasets.building3d import load_wireframe
    vs, es = [], []
    for p in WIREFRAMES:
        v, e = load_wireframe(p)
        vs.append(torch.from_numpy(v).float())
        es.append(torch.from_numpy(np.asarray(e, dtype=np.int64).reshape(-1, 2)))
    return vs, es


def _inline_train_py(wf_vertices, wf_edges, max_vertices):
    """train.py's own loops (:50-88 existence + edge labels over every candidate pair, :112-115 target vertices)."""
    B = len(wf_vertices)
    exist = torch.zeros(B, max_vertices)
    counts = []
    for i in range(B):
        counts.append(len(wf_vertices[i]))
        exist[i, :counts[i]] = 1.0
    labels = []
    for i in range(B):
        edge_set = {(min(int(a), int(b)), max(int(a), int(b))) for a, b in wf_edges[i].tolist()}
        pairs = [(j, k) for j in range(counts[i]) for k in range(j + 1, counts[i])]
        lab = torch.zeros(len(pairs))
        for n, pr in enumerate(pairs):
            if pr in edge_set:
                lab[n] = 1.0
        labels.append(lab)
    width = max(len(lab) for lab in labels)
    edge_labels = torch.zeros(B, width)
    for i, lab in enumerate(labels):
        edge_labels[i, :len(lab)] = lab
    tv = torch.zeros(B, max_vertices, 3)
    for i in range(B):
        tv[i, :counts[i]] = wf_vertices[i][:counts[i]]
    return {"vertices": tv, "vertex_existence": exist, "edge_labels": edge_labels,
            "vertex_counts": torch.tensor(counts, dtype=torch.long)}


@pytest.mark.parametrize("max_vertices", [38, 64])
def test_train_targets_match_train_py(max_vertices):
    from wf3d.targets import train_targets
    vs, es = _golden_batch()
    want = _inline_train_py(vs, es, max_vertices)
    got = train_targets(vs, es, max_vertices)
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    assert float(want["edge_labels"].sum()) > 0
    full = train_targets(vs, es, max_vertices, full_width=True)
    E = max_vertices * (max_vertices - 1) // 2
    assert tuple(full["edge_labels"].shape) == (len(vs), E)
    w = want["edge_labels"].shape[1]
    assert torch.equal(full["edge_labels"][:, :w], want["edge_labels"])
    assert not full["edge_labels"][:, w:].any()
    for k in ("vertices", "vertex_existence", "vertex_counts"):
        assert torch.equal(full[k], want[k]), k


def test_train_targets_refuses_more_vertices_than_max():
    from wf3d.targets import train_targets
    vs, es = _golden_batch()
    with pytest.raises(ValueError, match="max_vertices"):
        train_targets(vs, es, min(len(v) for v in vs) - 1)


def test_lazy_edge_indices_equal_lists_and_refuse_mutation():
    from wf3d.functional import EdgeIndexLists, edge_index_lists
    counts = torch.tensor([5, 0, 1, 7, 2])
    lazy = EdgeIndexLists(counts)
    assert len(lazy) == 5 and lazy._lists is None          # len() reads nothing
    want = edge_index_lists([5, 0, 1, 7, 2])
    assert lazy == want and list(lazy) == want
    assert lazy[3] == [[i, j] for i in range(7) for j in range(i + 1, 7)]
    assert lazy[1] == [] and lazy[2] == []
    for bad in (lambda: lazy.append([]), lambda: lazy.__setitem__(0, []), lambda: lazy.pop(), lambda: lazy.clear(),
                lambda: lazy[0].append([0, 1]), lambda: lazy[3][0].__setitem__(0, 9)):
        with pytest.raises(TypeError):
            bad()
    assert lazy == edge_index_lists([5, 0, 1, 7, 2])


def test_edge_layout_refuses_int32_overflow_on_host():
    from wf3d import _lib
    lib = _lib.load()
    # B * V(V-1)/2 > 2^31 - 1: refused before anything is launched (no pointer is read)
    assert lib.wf3d_edge_layout(None, 4096, 1100, None, None, None, None, None, None, None) != 0
    assert b"int32" in lib.wf3d_last_error()
    assert lib.wf3d_edge_layout(None, 0, 8, None, None, None, None, None, None, None) != 0
