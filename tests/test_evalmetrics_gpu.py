"""Evaluation metrics on the device (csrc/evalmetrics.hip; the solver body is csrc/lsa_solve.h): wf3d_lsa_rect_batch against the numpy model
(tests/evalmetrics_model.py) element for element and against scipy where the optimum is unique; then
evaluate_batch(compact=True, metrics="device") against metrics="host" on the inputs of tests/test_evalmetrics_model.py —
integer counters exact, `distance` and `wed` within rtol 1e-12 — and EvalLabels reuse."""
import numpy as np
import pytest
import torch

import evalmetrics_model as model
import helpers as H
from test_eval import COUNTERS, _check_counters
from test_evalpost_compact_gpu import _pred

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(0, 8), (1, 1), (1, 40), (40, 1), (37, 8), (8, 37), (64, 64), (65, 64), (130, 129), (500, 40), (0, 0)]
INT_KEYS = ("tp_corners", "tp_fp_corners", "tp_fn_corners", "tp_edges", "tp_fp_edges", "tp_fn_edges")


def _solve(mats):
    """One ragged launch over the [n_s, m_s] float64 matrices -> (entries per sample, status [B])."""
    from wf3d import _lib
    from wf3d.ops import _stream
    lib = _lib.load()
    B = len(mats)
    n, m = np.array([c.shape[0] for c in mats]), np.array([c.shape[1] for c in mats])
    noff, moff, ooff, aoff = (np.concatenate(([0], np.cumsum(x))) for x in (n, m, n * m, np.minimum(n, m)))
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)          # noqa: E731
    cost = dev(np.concatenate([c.reshape(-1) for c in mats] + [np.zeros(1)]), np.float64)
    d_noff, d_moff, d_ooff, d_aoff = dev(noff, np.int32), dev(moff, np.int32), dev(ooff, np.int64), dev(aoff, np.int32)
    out = torch.full((int(aoff[-1]) + 1,), -7, dtype=torch.int32, device=DEV)
    status = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    max_long = int(max(n.max(), m.max()))
    ws_bytes = lib.wf3d_lsa_rect_ws_bytes(B, max_long)
    assert (ws_bytes > 0) == (max_long > 1024)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=DEV)
    _lib.check(lib.wf3d_lsa_rect_batch(cost.data_ptr(), d_ooff.data_ptr(), d_noff.data_ptr(), d_moff.data_ptr(), 1,
                                       d_aoff.data_ptr(), B, max_long, out.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                       ws_bytes, _stream()), "lsa_rect_batch")
    flat = out.cpu().numpy()
    assert flat[-1] == -7                                        # nothing past the last sample's entries
    return [flat[aoff[s]:aoff[s + 1]] for s in range(B)], status.cpu().numpy()


def _check_against_model(mats, got, status, want_status=0):
    for c, e, st in zip(mats, got, status):
        want, wst = model.lsa_rect(c)
        assert st == wst == (want_status if c.size else 0), (c.shape, st, wst)
        assert e.shape == want.shape and np.array_equal(e, want), (c.shape, e, want)


def test_rect_solver_continuous_costs_match_model_and_scipy():
    from scipy.optimize import linear_sum_assignment
    gen = np.random.RandomState(11)
    mats = [gen.uniform(0, 10, s) for s in SHAPES]
    got, status = _solve(mats)
    _check_against_model(mats, got, status)
    for c, e in zip(mats, got):
        if c.size == 0:
            continue
        r, cc = linear_sum_assignment(c)
        n, m = c.shape
        mine_r, mine_c = (np.arange(n), e) if n <= m else (e, np.arange(m))
        order = np.argsort(mine_r)
        assert np.array_equal(mine_r[order], r) and np.array_equal(mine_c[order], cc), c.shape
        assert np.isclose(c[mine_r, mine_c].sum(), c[r, cc].sum(), rtol=1e-12, atol=0.0)


def test_rect_solver_heavy_ties_match_model():
    gen = np.random.RandomState(12)
    mats = [gen.randint(0, 3, s).astype(np.float64) for s in SHAPES]
    got, status = _solve(mats)
    _check_against_model(mats, got, status)
    for c, e in zip(mats, got):
        assert len(set(e.tolist())) == len(e) == min(c.shape)


def test_rect_solver_state_in_the_workspace_beyond_1024_columns():
    gen = np.random.RandomState(13)
    mats = [gen.uniform(0, 10, s) for s in ((3, 1030), (1030, 3), (7, 5), (40, 1100))] + [gen.randint(0, 3, (1025, 6)).astype(np.float64)]
    got, status = _solve(mats)
    _check_against_model(mats, got, status)


def test_rect_solver_returns_on_non_finite_costs():
    gen = np.random.RandomState(14)
    mats = [gen.uniform(0, 10, s) for s in ((6, 9), (9, 6), (70, 66), (5, 5))]
    for c in mats[:3]:
        c[1, 2], c[0, 0], c[3, 4], c[2, :] = np.nan, np.inf, -np.inf, np.nan
    mats[2][:, 7] = np.inf
    mats[2][5, 5] = 1e300                                        # finite, beyond FLT_MAX
    got, status = _solve(mats)
    assert status.tolist() == [model.NONFINITE] * 3 + [0]
    for c, e, st in zip(mats, got, status):
        want, wst = model.lsa_rect(c)                            # the model solves the clamped costs
        assert st == wst and np.array_equal(e, want)
        long_side = max(c.shape)
        assert len(set(e.tolist())) == len(e) == min(c.shape) and e.min() >= 0 and e.max() < long_side


def test_limits_are_reported_without_a_launch():
    from wf3d import _lib
    lib = _lib.load()
    U = _lib.DEFINES["WF3D_ERR_UNSUPPORTED"]
    assert lib.wf3d_lsa_rect_batch(None, None, None, None, 1, None, 65536, 8, None, None, None, 0, None) == U
    assert b"65535" in lib.wf3d_last_error()
    args = lambda B, V, lv: (None, 0, 0, B, V, None, None, None, None, None, None, None, None, None, None, 1.0, lv, 8, 8,   # noqa: E731
                             None, None, None, 0, None)
    assert lib.wf3d_eval_metrics(*args(65536, 12, 8)) == U and b"65535" in lib.wf3d_last_error()
    assert lib.wf3d_eval_metrics(*args(4, 1025, 8)) == U and b"1024" in lib.wf3d_last_error()
    assert lib.wf3d_eval_metrics(*args(4, 12, 1025)) == U and b"1024" in lib.wf3d_last_error()
    assert lib.wf3d_lsa_rect_ws_bytes(32, 1024) == 0 and lib.wf3d_lsa_rect_ws_bytes(32, 2016) >= 32 * 41 * 2016
    assert lib.wf3d_eval_metrics_ws_bytes(32, 64, 32 * 12, 95) >= 8 * 64 * 32 * 12


# ---- end to end -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs():
    g = H.load_golden("eval")
    return g, model.cases(g)


def _batch(cases_, counts=None):
    verts, probs = np.stack([c[1] for c in cases_]), np.stack([c[2] for c in cases_])
    return verts, probs, counts or [verts.shape[1]] * len(cases_)


def _run(verts, probs, counts, gt, layout, metrics, thresh=1, labels=None, monkeypatch=None, may_raise=False):
    """-> (calculator, compute_metrics calls, the ValueError raised (only with may_raise) or None)"""
    from eval import ap_calculator as ap
    from wf3d import postprocess
    calc, calls = ap.APCalculator(distance_thresh=thresh), []
    real = ap.APCalculator.compute_metrics
    monkeypatch.setattr(ap.APCalculator, "compute_metrics", lambda self, batch: calls.append(1) or real(self, batch))
    raised = None
    try:
        postprocess.evaluate_batch(_pred(verts, probs, counts, layout), [torch.from_numpy(v) for v, _ in gt],
                                   [torch.from_numpy(e.astype(np.float32)) for _, e in gt], calc, compact=True, metrics=metrics,
                                   labels=labels)
    except ValueError as e:
        raised = e
    monkeypatch.undo()
    if raised is not None and not may_raise:
        raise raised
    return calc, len(calls), raised


def _same(a, b, what=""):
    for k in INT_KEYS:
        assert int(a.ap_dict[k]) == int(b.ap_dict[k]), (what, k, a.ap_dict[k], b.ap_dict[k])
    for k in ("distance", "wed"):
        assert np.isclose(float(a.ap_dict[k]), float(b.ap_dict[k]), rtol=1e-12, atol=0.0), (what, k, a.ap_dict[k], b.ap_dict[k])
    assert a.batch_size == b.batch_size


@pytest.mark.parametrize("layout", ["ragged", "padded"])
def test_device_metrics_match_the_host_path(inputs, layout, monkeypatch):
    g, cases_ = inputs
    gt1 = (g["gt_v"], g["gt_e"])
    # B = 3: the fixture samples, held to the reference's recorded counters
    verts, probs, counts = _batch(cases_[:3])
    host, calls_h, _ = _run(verts, probs, counts, [gt1] * 3, layout, "host", monkeypatch=monkeypatch)
    dev, calls_d, _ = _run(verts, probs, counts, [gt1] * 3, layout, "device", monkeypatch=monkeypatch)
    assert (calls_h, calls_d) == (3, 0)
    _same(host, dev, "fixture")
    _check_counters(dev, g["c2.counters"], "batch")
    # B = 16: every case that does not raise, one of them with 5 of its 12 vertices counted (a shorter edge list)
    good = [c for c in cases_ if not c[3]]
    assert len(good) == 16
    verts, probs, counts = _batch(good)
    counts[4] = 5
    probs[4, 10:] = 0.0
    assert (probs[4, :10] > 0.5).any()
    # at the tighter threshold two samples keep edges of which none matches (the host raises there): the other 14
    tight = [k for k, c in enumerate(good) if c[0] not in ("fixture1", "noise0.6_3")]
    for thresh, pick in ((1, list(range(16))), (1, list(range(1, 16))), (0.5, tight)):        # B = 16, 15, 14
        B = len(pick)
        args = (verts[pick], probs[pick], [counts[k] for k in pick], [gt1] * B, layout)
        host, calls_h, _ = _run(*args, "host", thresh, monkeypatch=monkeypatch)
        dev, calls_d, _ = _run(*args, "device", thresh, monkeypatch=monkeypatch)
        assert (calls_h, calls_d) == (B, 0), (calls_h, calls_d)
        _same(host, dev, thresh)


def _prism():
    """12 vertices, 18 edges: two hexagons and the six uprights (the label of scripts/bench_evalpost.py)"""
    a = np.arange(6) * (np.pi / 3)
    low = np.stack((4 * np.cos(a), 4 * np.sin(a), np.zeros(6)), axis=1)
    top = np.stack((3 * np.cos(a + 0.2), 3 * np.sin(a + 0.2), np.full(6, 3.0)), axis=1)
    edges = [(i, (i + 1) % 6) for i in range(6)] + [(6 + i, 6 + (i + 1) % 6) for i in range(6)] + [(i, 6 + i) for i in range(6)]
    return np.concatenate((low, top)).astype(np.float32), np.array(sorted((min(e), max(e)) for e in edges), dtype=np.int64)


def test_device_metrics_beyond_one_pass_of_the_workgroup(monkeypatch):
    """V = 300 predicted vertices: more than the 256 threads of the corner-set workgroup, 44,850 candidates; more kept
    edges than label edges in one sample, fewer in the other, duplicate free corners in both."""
    gt_v, gt_e = _prism()
    gen = np.random.RandomState(21)
    B, V = 2, 300
    max_e = V * (V - 1) // 2
    verts = gen.uniform(-8, 8, (B, V, 3)).astype(np.float32)
    verts[:, :12] = gt_v + gen.normal(0, 0.02, (B, 12, 3)).astype(np.float32)
    verts[:, 270:] = verts[:, 260:261]                           # 30 coincident free corners past the first pass
    offset = lambda i: i * (2 * V - i - 1) // 2                  # noqa: E731
    label_e = np.array([offset(i) + j - i - 1 for i, j in gt_e])
    probs = gen.uniform(0.0, 0.45, (B, max_e)).astype(np.float32)
    probs[0, label_e] = 0.9
    probs[0, gen.choice(max_e, 30, replace=False)] = 0.8
    probs[1, label_e[:11]] = 0.9
    for thresh in (1, 0.1):
        host, calls_h, _ = _run(verts, probs, [V, V], [(gt_v, gt_e)] * B, "ragged", "host", thresh, monkeypatch=monkeypatch)
        dev, calls_d, _ = _run(verts, probs, [V, V], [(gt_v, gt_e)] * B, "ragged", "device", thresh, monkeypatch=monkeypatch)
        assert (calls_h, calls_d) == (2, 0)
        _same(host, dev, thresh)
        assert int(dev.ap_dict["tp_edges"]) == 18 + 11 and int(dev.ap_dict["tp_fp_corners"]) == 600


def test_device_metrics_raise_where_the_host_raises(inputs, monkeypatch):
    g, cases_ = inputs
    gt1 = (g["gt_v"], g["gt_e"])
    by = {c[0]: c for c in cases_}
    verts, probs, counts = _batch([by["fixture0"], by["coincident"], by["all_miss"], by["fixture1"]])
    host, _, err_h = _run(verts, probs, counts, [gt1] * 4, "ragged", "host", monkeypatch=monkeypatch, may_raise=True)
    dev, calls_d, err_d = _run(verts, probs, counts, [gt1] * 4, "ragged", "device", monkeypatch=monkeypatch, may_raise=True)
    assert isinstance(err_h, ValueError) and type(err_d) is type(err_h) and str(err_d) == str(err_h)
    assert calls_d == 1                                          # the flagged sample alone went through the host call
    _same(host, dev, "before the raise")                         # what the two samples before it accumulated


def test_float64_and_edgeless_labels_take_the_host_call(inputs, monkeypatch):
    g, cases_ = inputs
    verts, probs, counts = _batch(cases_[:4])
    gt = [(g["gt_v"], g["gt_e"]), (g["gt_v"].astype(np.float64), g["gt_e"]), (g["gt_v"], g["gt_e"]),
          (g["gt_v"], np.empty((0, 2), dtype=np.int64))]
    probs[3] = 0.0                                               # an edgeless label is only evaluable without kept edges
    host, calls_h, err_h = _run(verts, probs, counts, gt, "ragged", "host", monkeypatch=monkeypatch)
    dev, calls_d, err_d = _run(verts, probs, counts, gt, "ragged", "device", monkeypatch=monkeypatch)
    assert err_h is None and err_d is None and (calls_h, calls_d) == (4, 2)
    _same(host, dev)


def test_compact_false_with_device_metrics_is_refused(inputs):
    from eval import ap_calculator as ap
    from wf3d import postprocess
    g, cases_ = inputs
    verts, probs, counts = _batch(cases_[:1])
    with pytest.raises(ValueError, match="compact=True"):
        postprocess.evaluate_batch(_pred(verts, probs, counts), [torch.from_numpy(g["gt_v"])],
                                   [torch.from_numpy(g["gt_e"].astype(np.float32))], ap.APCalculator(distance_thresh=1),
                                   metrics="device")


def test_eval_labels_are_reusable(inputs, monkeypatch):
    from wf3d.postprocess import EvalLabels
    g, cases_ = inputs
    second_v = (g["gt_v"] + np.float32(0.03)).astype(np.float32)            # another label that the predictions still match
    second_e = np.concatenate((g["gt_e"][:7], np.array([[3, 5], [1, 2]], dtype=np.int64)))
    gt = [(g["gt_v"], g["gt_e"]), (second_v, second_e), (g["gt_v"], g["gt_e"]), (second_v, second_e)]
    tensors = lambda gt_: ([torch.from_numpy(v) for v, _ in gt_], [torch.from_numpy(e) for _, e in gt_])    # noqa: E731
    labels = EvalLabels(*tensors(gt), DEV)
    ptrs = [t.data_ptr() for t in (labels.lvoff, labels.loff, labels.lverts, labels.lseg)]
    good = [c for c in cases_ if not c[3]]
    for batch in (good[:4], good[5:9]):
        verts, probs, counts = _batch(batch)
        kept, calls, _ = _run(verts, probs, counts, gt, "ragged", "device", labels=labels, monkeypatch=monkeypatch)
        fresh, _, _ = _run(verts, probs, counts, gt, "ragged", "device", monkeypatch=monkeypatch)
        host, _, _ = _run(verts, probs, counts, gt, "ragged", "host", monkeypatch=monkeypatch)
        assert calls == 0
        for k in COUNTERS:
            assert float(kept.ap_dict[k]) == float(fresh.ap_dict[k]), k
        _same(host, kept)
    assert ptrs == [t.data_ptr() for t in (labels.lvoff, labels.loff, labels.lverts, labels.lseg)]
    part, built = labels[[3, 0]], EvalLabels(*tensors([gt[3], gt[0]]), DEV)
    for a, b in ((part.lvoff, built.lvoff), (part.loff, built.loff), (part.lverts, built.lverts), (part.lseg, built.lseg)):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert part.consts == built.consts
    verts, probs, counts = _batch(good[:2])
    a, _, _ = _run(verts, probs, counts, [gt[3], gt[0]], "ragged", "device", labels=part, monkeypatch=monkeypatch)
    b, _, _ = _run(verts, probs, counts, [gt[3], gt[0]], "ragged", "device", labels=built, monkeypatch=monkeypatch)
    for k in COUNTERS:
        assert float(a.ap_dict[k]) == float(b.ap_dict[k]), k
    with pytest.raises(ValueError, match="labels of 4 samples"):
        _pred_and_eval(verts, probs, counts, gt[:2], labels)


def _pred_and_eval(verts, probs, counts, gt, labels):
    from eval import ap_calculator as ap
    from wf3d import postprocess
    postprocess.evaluate_batch(_pred(verts, probs, counts), [torch.from_numpy(v) for v, _ in gt],
                               [torch.from_numpy(e) for _, e in gt], ap.APCalculator(distance_thresh=1), compact=True,
                               metrics="device", labels=labels)
