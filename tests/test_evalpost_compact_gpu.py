"""Compacted evaluation post-processing on the device: wf3d_edge_compact through wf3d.postprocess.wireframes_compact
against the numpy model (tests/evalpost_model.py) and against wireframes_from_predictions on the same inputs — every
comparison exact — then wf3d_hausdorff_lines_batch against the numpy hausdorff_distance_line, and evaluate_batch with
compact=True against compact=False and the reference's recorded counters."""
import numpy as np
import pytest
import torch

import evalpost_model as model
import helpers as H
from test_eval import COUNTERS, _check_counters

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KEYS = ("pred_vertices", "pd_edges", "pd_edges_vertices")


def _tri(c):
    return c * (c - 1) // 2


def _pred(verts, probs, counts, layout="ragged"):
    """Model-style predictions: `vertices` is the strided [:, :, :3] view of a [B, V, 4] tensor, as the model returns it."""
    from wf3d.functional import EdgeIndexLists, edge_index_lists
    B, V, _ = verts.shape
    v4 = torch.full((B, V, 4), 7.0)
    v4[:, :, :3] = torch.from_numpy(verts)
    pred = {"vertices": v4.to(DEV)[:, :, :3], "edge_probs": torch.from_numpy(probs).to(DEV)}
    if layout == "padded":
        pred["edge_counts"] = torch.tensor(counts, dtype=torch.int64, device=DEV)
        pred["edge_indices"] = EdgeIndexLists(pred["edge_counts"])
    else:
        pred["edge_indices"] = edge_index_lists([int(c) for c in counts])
    return pred


def _check(verts, probs, counts, threshold=0.5, old=True, layout="ragged"):
    """wireframes_compact == the model, exactly, and (old=True) == wireframes_from_predictions."""
    from wf3d import postprocess
    pred = _pred(verts, probs, counts, layout)
    got, d = postprocess.wireframes_compact(pred, threshold, keep_device=True)
    koff, pairs, seg, kprob = model.compact(counts, probs, verts, threshold)
    assert np.array_equal(d["koff"].cpu().numpy(), koff) and np.array_equal(d["koff_host"], koff)
    assert d["koff"].dtype == torch.int32 and np.array_equal(d["seg"][:koff[-1]].cpu().numpy(), seg)
    assert len(got) == len(counts)
    for s, w in enumerate(got):
        a, b = koff[s], koff[s + 1]
        assert sorted(w) == sorted(KEYS + ("pd_edge_probs",))
        assert w["pd_edges"].dtype == np.int64 and w["pd_edges"].shape == (b - a, 2)
        assert w["pd_edges_vertices"].dtype == np.float32 and w["pd_edges_vertices"].shape == (b - a, 2, 3)
        assert w["pd_edge_probs"].dtype == np.float32 and w["pd_edge_probs"].shape == (b - a,)
        assert w["pred_vertices"].dtype == np.float32 and np.array_equal(w["pred_vertices"], verts[s])
        assert np.array_equal(w["pd_edges"], pairs[a:b])
        assert np.array_equal(w["pd_edges_vertices"], seg[a:b])
        assert np.array_equal(w["pd_edge_probs"], kprob[a:b])
    if old:
        ref = postprocess.wireframes_from_predictions(_pred(verts, probs, counts), threshold)
        for s, (w, r) in enumerate(zip(got, ref)):
            for k in KEYS:
                assert w[k].dtype == r[k].dtype and w[k].shape == r[k].shape and np.array_equal(w[k], r[k]), (s, k)
    return got, pred


def _verts(gen, B, V):
    return gen.normal(0, 3, (B, V, 3)).astype(np.float32)


def test_index_inversion_exhaustive_to_64_vertices():
    gen = np.random.RandomState(3)
    counts = list(range(2, 65))
    probs = np.full((63, _tri(64)), 0.9, np.float32)            # above the threshold PAST each sample's pairs too
    got, _ = _check(_verts(gen, 63, 64), probs, counts)
    for c, w in zip(counts, got):
        assert np.array_equal(w["pd_edges"], np.stack(np.triu_indices(c, 1), axis=1))


def test_index_inversion_at_256_vertices():
    gen = np.random.RandomState(4)
    counts = [256, 255, 182, 181, 129, 128, 2]
    probs = np.full((7, _tri(256)), 0.9, np.float32)
    got, _ = _check(_verts(gen, 7, 256), probs, counts)
    for c, w in zip(counts, got):
        assert np.array_equal(w["pd_edges"], np.stack(np.triu_indices(c, 1), axis=1))


def test_chunk_boundary():
    """V = 24: 276 candidates, two 256-candidate chunks; kept edges on both sides, the first and the last candidate."""
    gen = np.random.RandomState(5)
    probs = np.zeros((3, 276), np.float32)
    probs[0, [0, 255, 256, 275]] = 0.8
    probs[1, [63, 64, 127, 128, 191, 192, 254, 255, 256, 257]] = 0.7          # wave boundaries inside the chunk too
    probs[2, 250:262] = 0.6
    got, _ = _check(_verts(gen, 3, 24), probs, [24, 24, 24])
    assert [len(w["pd_edges"]) for w in got] == [4, 10, 12]
    assert got[0]["pd_edges"].tolist() == [[0, 1], [17, 18], [17, 19], [22, 23]]


def test_scan_crosses_its_tile():
    """B = 160 at V = 64: 8 chunks per sample, 1280 chunk counts — more than one scan tile of 1024."""
    gen = np.random.RandomState(6)
    B, V = 160, 64
    counts = gen.randint(0, V + 1, B)
    counts[[0, 127, 128, 159]] = V                               # the samples around the tile boundary are full
    probs = gen.uniform(0, 1, (B, _tri(V))).astype(np.float32)
    probs[gen.uniform(0, 1, probs.shape) < 0.8] = 0.1
    got, _ = _check(_verts(gen, B, V), probs, counts.tolist())
    assert sum(len(w["pd_edges"]) for w in got) > 1024


def test_degenerate_inputs():
    gen = np.random.RandomState(7)
    B, V = 5, 6
    verts = _verts(gen, B, V)
    verts[0, 1, 2] = verts[0, 2, 2] = verts[0, 4, 2]            # equal z: edges (1, 2), (1, 4), (2, 4) of sample 0
    counts = [6, 0, 1, 4, 2]
    probs = gen.uniform(0, 1, (B, _tri(V))).astype(np.float32)
    probs[0, 5:9] = 0.9                                          # e = 5 is (1, 2), e = 7 is (1, 4)
    probs[0, 2], probs[0, 3], probs[3, 1] = 0.5, np.nan, np.nan  # equal to the threshold, NaN: neither is kept
    got, _ = _check(verts, probs, counts)
    assert [1, 2] in got[0]["pd_edges"].tolist() and [0, 3] not in got[0]["pd_edges"].tolist()
    assert [0, 4] not in got[0]["pd_edges"].tolist()
    k = got[0]["pd_edges"].tolist().index([1, 2])
    assert np.array_equal(got[0]["pd_edges_vertices"][k], verts[0, [2, 1]])            # the second vertex first
    assert len(got[1]["pd_edges"]) == len(got[2]["pd_edges"]) == 0
    # a non-default threshold, with probabilities equal to it
    t = np.float32(0.3)
    probs2 = np.where(probs > 0.6, t, probs).astype(np.float32)
    assert (probs2 == t).sum() > 3
    _check(verts, probs2, counts, threshold=0.3)
    _check(verts, probs2, counts, threshold=0.05)
    # nothing kept, everything kept
    got, _ = _check(verts, np.zeros_like(probs), counts)
    for w in got:
        assert w["pd_edges"].shape == (0, 2) and w["pd_edges_vertices"].shape == (0, 2, 3) and w["pd_edge_probs"].shape == (0,)
    got, _ = _check(verts, np.ones_like(probs), [V] * B)
    assert sum(len(w["pd_edges"]) for w in got) == B * _tri(V)


def test_no_probability_columns():
    from wf3d import postprocess
    gen = np.random.RandomState(8)
    verts = _verts(gen, 3, 6)
    for layout, counts in (("ragged", [0, 0, 0]), ("padded", [6, 3, 0])):
        pred = _pred(verts, np.zeros((3, 0), np.float32), counts, layout)
        got, d = postprocess.wireframes_compact(pred, keep_device=True)
        assert d["koff"].cpu().tolist() == [0, 0, 0, 0]
        for s, w in enumerate(got):
            assert np.array_equal(w["pred_vertices"], verts[s])
            assert w["pd_edges"].shape == (0, 2) and w["pd_edges"].dtype == np.int64
            assert w["pd_edges_vertices"].shape == (0, 2, 3) and w["pd_edges_vertices"].dtype == np.float32


class _OpaqueList:
    """An inner edge-index list that may only be measured."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __iter__(self):
        raise AssertionError("wireframes_compact iterated an inner edge_indices list")

    def __getitem__(self, i):
        raise AssertionError("wireframes_compact indexed an inner edge_indices list")


def test_layouts_never_touch_the_index_lists():
    from wf3d import postprocess
    gen = np.random.RandomState(9)
    B, V = 4, 12
    counts = [12, 5, 0, 9]
    verts = _verts(gen, B, V)
    probs = gen.uniform(0, 1, (B, _tri(V))).astype(np.float32)
    want, pred = _check(verts, probs, counts)
    assert not pred["vertices"].is_contiguous() and pred["vertices"].stride(1) == 4
    ragged = dict(pred, edge_indices=[_OpaqueList(_tri(c)) for c in counts])
    padded = _pred(verts, probs, counts, "padded")
    assert padded["edge_counts"].is_cuda and padded["edge_indices"]._lists is None
    for p in (ragged, padded):
        got = postprocess.wireframes_compact(p)
        for w, r in zip(got, want):
            for k in KEYS + ("pd_edge_probs",):
                assert np.array_equal(w[k], r[k])
    assert padded["edge_indices"]._lists is None
    _check(verts, probs, counts, layout="padded")


def test_limits_are_reported():
    from wf3d import _lib
    lib = _lib.load()
    koff = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert lib.wf3d_edge_compact(None, 0, 0, None, None, 65536, 4, 6, 0.5, koff.data_ptr(), None, None, None, None, 0, None) == \
        _lib.DEFINES["WF3D_ERR_UNSUPPORTED"] and b"65535" in lib.wf3d_last_error()
    assert lib.wf3d_edge_compact(None, 0, 0, None, None, 65535, 400, 40000, 0.5, koff.data_ptr(), None, None, None, None, 0,
                                 None) == _lib.DEFINES["WF3D_ERR_UNSUPPORTED"] and b"2^31" in lib.wf3d_last_error()
    assert lib.wf3d_hausdorff_lines_batch(None, None, None, None, None, 1, 1, 33, None, None) == _lib.DEFINES["WF3D_ERR_UNSUPPORTED"]
    koff.fill_(5)
    assert lib.wf3d_edge_compact(None, 0, 0, None, None, 3, 1, 6, 0.5, koff.data_ptr(), None, None, None, None, 0, None) == 0
    assert koff.cpu().tolist() == [0, 0, 0, 0]


# ---- Hausdorff, batched ---------------------------------------------------------------------------------------------
def _hausdorff_batch(ps, ts, S):
    """per-sample [n_s, m_s] matrices (None where n_s * m_s = 0) of float32 segment lists, one launch"""
    from wf3d import _lib
    from wf3d.ops import _stream
    n, m = np.array([len(p) for p in ps]), np.array([len(t) for t in ts])
    koff, loff, ooff = (np.concatenate(([0], np.cumsum(x))) for x in (n, m, n * m))
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)          # noqa: E731
    seg, lseg = dev(np.concatenate(ps), np.float32), dev(np.concatenate(ts), np.float32)
    d_koff, d_loff, d_ooff = dev(koff, np.int32), dev(loff, np.int32), dev(ooff, np.int64)
    out = torch.full((int(ooff[-1]),), np.nan, dtype=torch.float64, device=DEV)
    _lib.check(_lib.load().wf3d_hausdorff_lines_batch(seg.data_ptr(), d_koff.data_ptr(), lseg.data_ptr(), d_loff.data_ptr(),
                                                      d_ooff.data_ptr(), len(ps), int((n * m).max()), S, out.data_ptr(),
                                                      _stream()), "hausdorff_lines_batch")
    flat = out.cpu().numpy()
    return [flat[ooff[s]:ooff[s + 1]].reshape(n[s], m[s]) if n[s] * m[s] else None for s in range(len(ps))]


@pytest.fixture(scope="module")
def ragged_segments():
    gen = np.random.RandomState(1)
    big_p, big_t = gen.normal(0, 3, (500, 2, 3)).astype(np.float32), gen.normal(0, 3, (40, 2, 3)).astype(np.float32)
    shapes = [(0, 8), (1, 1), (37, 0), (500, 40), (37, 8), (1, 40), (0, 0), (500, 1)]
    return [big_p[:n] for n, _ in shapes], [big_t[:m] for _, m in shapes]


@pytest.mark.parametrize("S", [1, 2, 20, 32])
def test_hausdorff_batch_matches_numpy(ragged_segments, S):
    from eval import ap_calculator as ap
    ps, ts = ragged_segments
    got = _hausdorff_batch(ps, ts, S)
    for p, t, h in zip(ps, ts, got):
        if len(p) == 0 or len(t) == 0:
            assert h is None
            continue
        want = ap.hausdorff_distance_line(p, t, sample_points=S)
        assert h.shape == want.shape and np.allclose(h, want, rtol=1e-12, atol=1e-12), (len(p), len(t), np.abs(h - want).max())


def test_hausdorff_batch_matches_reference_fixture():
    g = H.load_golden("eval")
    assert g["hd.p"].dtype == np.float32 and g["hd.t"].dtype == np.float32
    hd = _hausdorff_batch([g["hd.p"][:3], g["hd.p"]], [g["hd.t"], g["hd.t"]], 20)
    assert np.allclose(hd[1], g["hd.matrix"], rtol=1e-12, atol=1e-12)
    assert np.allclose(hd[0], g["hd.matrix"][:3], rtol=1e-12, atol=1e-12)


# ---- end to end -----------------------------------------------------------------------------------------------------
def _fixture_pred(g, cases, counts=None):
    V = int(g["V"])
    verts = np.stack([g[f"c{c}.vertices"] for c in cases])
    probs = np.stack([g[f"c{c}.probs"] for c in cases])
    return verts, probs, counts or [V] * len(cases)


def _both_ways(verts, probs, counts, gt_v, gt_e, monkeypatch, batched_samples):
    """evaluate_batch with compact=False (per-sample device Hausdorff) and compact=True; returns the two calculators.
    `batched_samples`: how many samples must get their matrix from the batched launch (the function is then not called)."""
    from eval import ap_calculator as ap
    from wf3d import postprocess
    labels = [torch.from_numpy(gt_v)] * len(counts), [torch.from_numpy(gt_e.astype(np.float32))] * len(counts)
    old, new = ap.APCalculator(distance_thresh=1), ap.APCalculator(distance_thresh=1)
    ap.set_device(DEV)
    try:
        postprocess.evaluate_batch(_pred(verts, probs, counts), *labels, old)
        calls = []
        real = ap.hausdorff_distance_line
        monkeypatch.setattr(ap, "hausdorff_distance_line", lambda p, t, *a, **k: calls.append(len(p)) or real(p, t, *a, **k))
        postprocess.evaluate_batch(_pred(verts, probs, counts), *labels, new, compact=True)
        monkeypatch.undo()
    finally:
        ap.set_device(None)
    with_edges = sum(1 for s in range(len(counts)) if (probs[s, :_tri(counts[s])] > 0.5).any())
    assert len(calls) == with_edges - batched_samples, (calls, with_edges)
    for k in COUNTERS:
        assert float(old.ap_dict[k]) == float(new.ap_dict[k]), (k, old.ap_dict[k], new.ap_dict[k])
    assert old.batch_size == new.batch_size
    return old, new


def test_evaluate_batch_fixture_samples_as_one_batch(monkeypatch):
    g = H.load_golden("eval")
    verts, probs, counts = _fixture_pred(g, (0, 1, 2))
    old, new = _both_ways(verts, probs, counts, g["gt_v"], g["gt_e"], monkeypatch, batched_samples=2)
    _check_counters(new, g["c2.counters"], "batch")             # the counters accumulate: after the third sample
    _check_counters(old, g["c2.counters"], "batch")


def test_evaluate_batch_ragged_counts(monkeypatch):
    """tests/test_eval.py's ragged case: the second sample has 5 vertices and keeps its own, shorter edge list"""
    g = H.load_golden("eval")
    verts, probs, counts = _fixture_pred(g, (0, 1), [int(g["V"]), 5])
    probs[1, 10:] = 0.0
    _both_ways(verts, probs, counts, g["gt_v"], g["gt_e"], monkeypatch, batched_samples=2)


def test_evaluate_batch_with_a_sample_that_keeps_no_edge(monkeypatch):
    g = H.load_golden("eval")
    verts, probs, counts = _fixture_pred(g, (2, 0))
    assert not (probs[0] > 0.5).any()
    _both_ways(verts, probs, counts, g["gt_v"], g["gt_e"], monkeypatch, batched_samples=1)


def test_evaluate_batch_float64_labels_take_the_per_sample_call(monkeypatch):
    g = H.load_golden("eval")
    verts, probs, counts = _fixture_pred(g, (0, 1))
    _both_ways(verts, probs, counts, g["gt_v"].astype(np.float64), g["gt_e"], monkeypatch, batched_samples=0)
