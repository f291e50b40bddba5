"""Compacted evaluation post-processing, the parts that need no GPU: the numpy model of the compaction
(tests/evalpost_model.py) against the reference semantics recorded in tests/golden/eval.npz, and APCalculator fed with
ready Hausdorff matrices through batch["hausdorff"]."""
import numpy as np
import pytest

import evalpost_model as model
import helpers as H
from test_eval import COUNTERS, _check_counters, _z_first


def test_model_matches_reference_semantics_on_the_fixture():
    g = H.load_golden("eval")
    V = int(g["V"])
    verts = np.stack([g[f"c{c}.vertices"] for c in range(3)])
    probs = np.stack([g[f"c{c}.probs"] for c in range(3)])
    koff, pairs, seg, kprob = model.compact([V, V, V], probs, verts, 0.5)
    assert koff.dtype == np.int32 and pairs.dtype == np.int32 and seg.dtype == np.float32 and kprob.dtype == np.float32
    assert koff[0] == 0 and pairs.shape == (koff[3], 2) and seg.shape == (koff[3], 2, 3) and kprob.shape == (koff[3],)
    for c in range(3):
        want = g["pairs"][g[f"c{c}.probs"] > 0.5]
        a, b = koff[c], koff[c + 1]
        assert b - a == len(want)
        assert np.array_equal(pairs[a:b], want)
        assert np.array_equal(seg[a:b], _z_first(g[f"c{c}.vertices"], want).astype(np.float32).reshape(-1, 2, 3))
        assert np.array_equal(kprob[a:b], g[f"c{c}.probs"][g[f"c{c}.probs"] > 0.5])
    assert koff[3] - koff[2] == 0 and koff[1] > 0                      # case 2 keeps nothing, case 0 something


def test_model_rules():
    verts = np.zeros((4, 5, 3), np.float32)
    verts[:, :, 2] = [3.0, 1.0, 1.0, 2.0, 0.0]                         # vertices 1 and 2 share z
    verts[:, :, 0] = np.arange(5)
    probs = np.full((4, 10), 0.9, np.float32)
    probs[0, 3], probs[0, 4] = 0.5, np.nan                             # equal to the threshold, NaN: not kept
    koff, pairs, seg, kprob = model.compact([5, 3, 1, 0], probs, verts, 0.5)
    assert koff.tolist() == [0, 8, 11, 11, 11]
    assert pairs[:8].tolist() == [[0, 1], [0, 2], [0, 3], [1, 3], [1, 4], [2, 3], [2, 4], [3, 4]]     # (0, 4) and (1, 2) dropped
    assert pairs[8:].tolist() == [[0, 1], [0, 2], [1, 2]]
    assert seg[10, :, 0].tolist() == [2.0, 1.0]                        # equal z: the second vertex comes first
    assert seg[8, :, 0].tolist() == [0.0, 1.0] and seg[3, :, 0].tolist() == [3.0, 1.0]      # higher z first
    assert np.array_equal(kprob, np.full(11, 0.9, np.float32))
    # a probability row narrower than the sample's candidate list cuts it
    assert model.compact([5], probs[:1, :2], verts[:1], 0.5)[1].tolist() == [[0, 1], [0, 2]]
    assert model.compact([5], probs[:1], verts[:1], 0.95)[0].tolist() == [0, 0]


def _fixture_batches(g):
    for c in range(3):
        pv = g[f"c{c}.vertices"].copy()
        pd_edges = g["pairs"][g[f"c{c}.probs"] > 0.5]
        yield c, {"predicted_vertices": pv[None], "predicted_edges": pd_edges[None],
                  "pred_edges_vertices": _z_first(pv, pd_edges).reshape(1, -1, 2, 3),
                  "wf_vertices": g["gt_v"].copy()[None], "wf_edges": g["gt_e"].copy()[None],
                  "wf_edges_vertices": _z_first(g["gt_v"], g["gt_e"]).reshape(1, -1, 2, 3)}


def test_ap_calculator_uses_given_hausdorff_matrices(monkeypatch):
    from eval import ap_calculator as ap
    g = H.load_golden("eval")
    given = {}
    for c, b in _fixture_batches(g):
        if b["predicted_edges"].shape[1]:
            given[c] = ap.hausdorff_distance_line(b["pred_edges_vertices"][0].copy(), b["wf_edges_vertices"][0].copy())
    assert sorted(given) == [0, 1]                                     # case 2 is the corners-only branch

    def refuse(*a, **k):
        raise AssertionError("hausdorff_distance_line called although the matrix was given")
    monkeypatch.setattr(ap, "hausdorff_distance_line", refuse)
    calc = ap.APCalculator(distance_thresh=1)
    for c, b in _fixture_batches(g):
        b["hausdorff"] = [given.get(c)]
        calc.compute_metrics(b)
        _check_counters(calc, g[f"c{c}.counters"], c)


def test_ap_calculator_none_entries_call_the_function(monkeypatch):
    from eval import ap_calculator as ap
    g = H.load_golden("eval")
    calls = []
    real = ap.hausdorff_distance_line

    def counted(p, t, *a, **k):
        calls.append((len(p), len(t)))
        return real(p, t, *a, **k)
    monkeypatch.setattr(ap, "hausdorff_distance_line", counted)
    calc = ap.APCalculator(distance_thresh=1)
    for c, b in _fixture_batches(g):
        b["hausdorff"] = [None]
        calc.compute_metrics(b)
        _check_counters(calc, g[f"c{c}.counters"], c)
    assert len(calls) == 2 and all(n > 0 and m == len(g["gt_e"]) for n, m in calls)
    assert len(COUNTERS) == 8
