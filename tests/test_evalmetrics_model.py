"""The numpy model of the device evaluation metrics (tests/evalmetrics_model.py) against the host path,
APCalculator.compute_metrics: integer counters exact, `distance` and `wed` within rtol 1e-12, on the three fixture samples
of eval.npz (held to the reference-recorded counters) and on seeded synthetic samples with coincident vertices, a
prediction equal to a label vertex, signed zeros, a corners-only sample with duplicate rows and one whose kept edges all
miss.  Then wf3d.postprocess.EvalLabels' label-only constants against graph_edit_distance, to the bit.  No GPU."""
import numpy as np
import pytest
import torch

import evalmetrics_model as model
import helpers as H
from test_eval import COUNTERS, _check_counters

INT_KEYS = ("tp_corners", "tp_fp_corners", "tp_fn_corners", "tp_edges", "tp_fp_edges", "tp_fn_edges")


@pytest.fixture(scope="module")
def setup():
    from eval import ap_calculator as ap
    from wf3d.postprocess import EvalLabels
    g = H.load_golden("eval")
    labels = EvalLabels([torch.from_numpy(g["gt_v"])], [torch.from_numpy(g["gt_e"].astype(np.float32))], "cpu")
    prepared = []
    for name, v, p, raises in model.cases(g):
        pd_edges = g["pairs"][p > 0.5]
        seg = model.z_first(v, pd_edges).astype(np.float32)
        hd = ap.hausdorff_distance_line(seg.copy(), labels.segs[0].copy()) if len(seg) else None
        prepared.append((name, v, pd_edges, seg, hd, raises))
    return g, labels, prepared


def _host(calc, g, labels, v, pd_edges, seg, hd):
    pd_ev = seg.copy() if len(pd_edges) else np.empty((0, 2, 3))
    calc.compute_metrics({"predicted_vertices": v.copy()[None], "predicted_edges": pd_edges[None],
                          "pred_edges_vertices": pd_ev.reshape(1, -1, 2, 3), "wf_vertices": g["gt_v"].copy()[None],
                          "wf_edges": g["gt_e"].copy()[None], "wf_edges_vertices": labels.segs[0].copy().reshape(1, -1, 2, 3),
                          "hausdorff": [None if hd is None else hd.copy()]})


def _same(a, b, what):
    for k in INT_KEYS:
        assert int(a.ap_dict[k]) == int(b.ap_dict[k]), (what, k, a.ap_dict[k], b.ap_dict[k])
    for k in ("distance", "wed"):
        assert np.isclose(float(a.ap_dict[k]), float(b.ap_dict[k]), rtol=1e-12, atol=0.0), (what, k, a.ap_dict[k], b.ap_dict[k])
    assert a.batch_size == b.batch_size


@pytest.mark.parametrize("thresh", [1, 0.1])
def test_model_matches_the_host_path(setup, thresh):
    from eval import ap_calculator as ap
    g, labels, prepared = setup
    assert len(prepared) >= 3 + 12 and sum(r for *_, r in prepared) == 1
    host, mod = ap.APCalculator(distance_thresh=thresh), ap.APCalculator(distance_thresh=thresh)
    for c, (name, v, pd_edges, seg, hd, raises) in enumerate(prepared):
        args = (v, seg, g["gt_v"], g["gt_e"], labels.segs[0], hd, labels.consts[0])
        if raises or (thresh == 0.1 and _raises_on_host(g, labels, v, pd_edges, seg, hd, thresh)):
            with pytest.raises(ValueError):
                _host(host, g, labels, v, pd_edges, seg, hd)
            with pytest.raises(ValueError):
                model.accumulate(mod, *args)
            continue
        _host(host, g, labels, v, pd_edges, seg, hd)
        one = ap.APCalculator(distance_thresh=thresh)
        model.accumulate(one, *args)
        model.accumulate(mod, *args)
        _same(host, mod, name)
        if thresh == 1 and c < 3:
            _check_counters(mod, g[f"c{c}.counters"], c)
            _check_counters(host, g[f"c{c}.counters"], c)


def _raises_on_host(g, labels, v, pd_edges, seg, hd, thresh):
    """at the tight threshold a noisy sample may keep edges of which none matches: then BOTH paths must raise"""
    from eval import ap_calculator as ap
    try:
        _host(ap.APCalculator(distance_thresh=thresh), g, labels, v, pd_edges, seg, hd)
    except ValueError:
        return True
    return False


def test_special_cases_are_what_they_claim(setup):
    g, labels, prepared = setup
    by = {name: (v, pd_edges, seg, hd) for name, v, pd_edges, seg, hd, _ in prepared}
    v, _, seg, hd = by["signed_zero"]
    r = model.sample(v, seg, g["gt_v"], labels.segs[0], hd, 1)
    assert np.signbit(v[9, 0]) and not np.signbit(v[8, 0]) and model._eq(v[8], v[9])
    v, _, seg, hd = by["coincident"]
    assert model._eq(v[3], v[5]) and len(model._distinct(list(v))) == 10
    v, _, seg, hd = by["corners_only_duplicates"]
    assert len(seg) == 0 and hd is None and len(model._distinct(list(v))) == 9
    r = model.sample(v, seg, g["gt_v"], labels.segs[0], hd, 1)
    assert r["tp_fp_corners"] == 12 and r["tp_edges"] == 0 and r["status"] == 0
    v, _, seg, hd = by["all_miss"]
    assert model.sample(v, seg, g["gt_v"], labels.segs[0], hd, 1)["status"] == model.NO_MATCH
    assert by["many_kept"][3].shape[0] > 8 > by["few_kept"][3].shape[0] > 0
    assert any(model._eq(by["equal_to_label"][0][2], u) for u in g["gt_v"])


def test_rect_solver_model_is_scipys_on_unique_optima():
    from scipy.optimize import linear_sum_assignment
    gen = np.random.RandomState(0)
    for n, m in ((1, 1), (3, 7), (7, 3), (12, 12), (20, 5), (5, 20)):
        C = gen.uniform(0, 1, (n, m))
        r, c, st = model.pairs(C)
        rr, cc = linear_sum_assignment(C)
        assert st == 0 and np.array_equal(r, rr) and np.array_equal(c, cc)
    C = gen.uniform(0, 1, (4, 6))
    C[1, 2], C[0, 0], C[3, 5], C[2, :] = np.nan, np.inf, -np.inf, np.nan
    e, st = model.lsa_rect(C)
    assert st == model.NONFINITE and sorted(set(e.tolist())) == sorted(e.tolist()) and e[3] == 5
    assert model.lsa_rect(np.empty((0, 5)))[0].size == 0


def test_label_constants_reproduce_graph_edit_distance_bit_for_bit(setup):
    from eval import ap_calculator as ap
    from wf3d.postprocess import EvalLabels, _gt_edge_vertices
    g, labels, _ = setup
    gen = np.random.RandomState(5)
    second_v = (g["gt_v"][::-1] * np.float32(1.7)).copy()
    second_e = np.array([[0, 1], [1, 2], [2, 3], [3, 0], [4, 5], [0, 5], [6, 7], [2, 7], [2, 6]], dtype=np.int64)
    both = EvalLabels([g["gt_v"], second_v, g["gt_v"].astype(np.float64), g["gt_v"]],
                      [g["gt_e"], second_e, g["gt_e"], np.empty((0, 2), dtype=np.int64)], "cpu")
    assert both.host.tolist() == [False, False, True, True] and both.consts[3] is None
    assert both.nverts.tolist() == [8, 8, 0, 0] and both.nsegs.tolist() == [8, 9, 0, 0]
    for s, (gt_v, gt_e) in enumerate(((g["gt_v"], g["gt_e"]), (second_v, second_e), (g["gt_v"].astype(np.float64), g["gt_e"]))):
        gt_ev = _gt_edge_vertices(gt_v, gt_e)
        for distances in (np.float64(0.0), np.float64(1.1934094724), np.float64(gen.uniform(0, 30)), np.float64(1e-9), np.float64(123456.789)):
            label_pts = np.unique(gt_ev.reshape(-1, 3), axis=0)
            want = ap.graph_edit_distance(label_pts, ap.computer_edges(gt_ev, label_pts).copy(), gt_v.copy(), gt_e.copy(), distances)
            got = both.wed(s, distances)
            assert float(got) == float(want), (s, distances, got, want)
    # a slice equals a fresh build
    part = both[[1, 0]]
    fresh = EvalLabels([second_v, g["gt_v"]], [second_e, g["gt_e"]], "cpu")
    for a, b in ((part.lvoff, fresh.lvoff), (part.loff, fresh.loff), (part.lverts, fresh.lverts), (part.lseg, fresh.lseg)):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert part.consts == fresh.consts and part.host.tolist() == [False, False] and len(both[1:3]) == 2
