"""wf3d.meter.WireframeMeter (csrc/metrics.hip) against tests/train_metrics_model.py, the definitions in numpy float64.

Bounds: the eleven integer counters are compared exactly.  sum_sq and sum_dist to rtol 1e-12: each d2 is formed as the
model forms it (products and sums rounded one by one), so only the order of summation differs; the sums have at most
789 non-negative fp64 terms (here at most 480: two updates of B = 2, V = 260 with 263 and 217 pairs), and the
order-of-summation bound (n - 1) * 2^-53 is below 1e-13.

Cases: B=3, V=5, Vt=7, counts [0, 2, 5] with `vertices` the [:, :, :3] view of a [B, V, 4] tensor (an empty sample, a full
one, wider targets, the model's layout); B=2, V=260, counts [3, 260], Ep=Et=33,670 (the stride loops past 256 threads,
17 edge chunks, rows whose start is and is not 16-byte aligned, a count above the V <= 64 solver's range); Ep != Et both
ways with device widths 0, Ep // 2 and past min(Ep, Et), NaN in every column at or past the common width; the decision
boundaries on exactly representable values; assignment entries -1, c_b and V; a NaN coordinate; the running row, reset
and bit-equal repeats; both assignment modes of the loss; and a captured criterion + update replayed on three contents."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402,F401
import train_metrics_model as TM  # noqa: E402


def dev():
    return torch.device("cuda:0")


def make(B, V, Vt, Ep, Et, counts, seed, near=0.05):
    """numpy inputs: a permutation of the V columns per sample as the assignment; matched targets lie around their
    prediction at distances on both sides of `near`; a few probabilities sit exactly on 0.5."""
    rng = np.random.RandomState(seed)
    out4 = rng.standard_normal((B, V, 4)).astype(np.float32)
    tverts = rng.standard_normal((B, Vt, 3)).astype(np.float32)
    counts = np.asarray(counts, np.int64)
    col4row = np.stack([rng.permutation(V) for _ in range(B)]).astype(np.int32)
    for b in range(B):
        cb = max(0, min(int(counts[b]), V, Vt))
        for p in range(V):
            t = col4row[b, p]
            if t < cb:
                step = rng.standard_normal(3)
                tverts[b, t] = out4[b, p, :3] + (step / np.linalg.norm(step) * near * rng.uniform(0.2, 1.8)).astype(np.float32)
    exist = rng.random_sample((B, V)).astype(np.float32)
    exist[:, ::3] = 0.5
    texist = (np.arange(V)[None, :] < counts[:, None]).astype(np.float32)
    edge = rng.random_sample((B, Ep)).astype(np.float32)
    edge[:, ::7] = 0.5
    tlabel = (rng.random_sample((B, Et)) > 0.7).astype(np.float32)
    return dict(out4=out4, exist=exist, edge=edge, tverts=tverts, texist=texist, tlabel=tlabel, col4row=col4row, counts=counts)


def model_row(c, edge_width=None, edge_threshold=0.5, distance_thresh=0.05):
    return TM.batch_row(c["out4"][:, :, :3], c["exist"], c["edge"], c["tverts"], c["texist"], c["tlabel"], c["col4row"],
                        c["counts"], edge_width, edge_threshold, distance_thresh)


def to_device(c, edge_width=None):
    t = {k: torch.from_numpy(v).to(dev()) for k, v in c.items()}
    pv = t["out4"][:, :, :3]
    assert pv.stride(1) == 4 and not pv.is_contiguous()
    pred = {"vertices": pv, "existence_probabilities": t["exist"], "edge_probs": t["edge"]}
    if edge_width is not None:
        pred["edge_width"] = torch.tensor(edge_width, dtype=torch.int64, device=dev())
    tgt = {"vertices": t["tverts"], "vertex_existence": t["texist"], "edge_labels": t["tlabel"], "vertex_counts": t["counts"]}
    return pred, tgt, t["col4row"]


def assert_rows(got, want, label):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    print(f"[train metrics] {label}: got {got.tolist()} model {want.tolist()}")
    assert np.array_equal(got[..., TM.INT_COLUMNS], want[..., TM.INT_COLUMNS]), (label, got, want)
    for k in TM.SUM_COLUMNS:
        g, w = got[..., k], want[..., k]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (label, k, g, w)
        ok = ~np.isnan(w)
        assert np.all(np.abs(g[ok] - w[ok]) <= 1e-12 * np.abs(w[ok])), (label, k, g, w)


def run_once(c, edge_width=None, edge_threshold=0.5, distance_thresh=0.05):
    from wf3d.meter import WireframeMeter
    qm = WireframeMeter(dev(), distance_thresh=distance_thresh, edge_threshold=edge_threshold)
    qm.update(*to_device(c, edge_width))
    s = qm.state.cpu().numpy()
    assert np.array_equal(s[0], s[1], equal_nan=True)               # first update after zeros: both rows are the batch
    return s[0]


def test_small_strided_case_with_wider_targets():
    c = make(3, 5, 7, 10, 10, [0, 2, 5], seed=1)
    row = run_once(c)
    assert_rows(row, model_row(c), "B3 V5 Vt7")
    assert row[2] == 7 and row[1] == 3 and 0 < row[5] < 7           # 0 + 2 + 5 pairs, some within 0.05 and some not


def test_many_vertices_and_edge_chunks():
    c = make(2, 260, 260, 33670, 33670, [3, 260], seed=2)
    row = run_once(c)
    assert_rows(row, model_row(c), "B2 V260 E33670")
    assert row[2] == 263


@pytest.mark.parametrize("Ep,Et", [(10, 7), (7, 10), (5000, 4100), (4100, 5000)])
def test_edge_widths_and_poison_past_the_common_width(Ep, Et):
    c = make(2, 5, 5, Ep, Et, [4, 5], seed=3)
    for ew in (None, 0, Ep // 2, min(Ep, Et) + 5):
        w = min(Ep, Et) if ew is None else min(ew, Ep, Et)
        want = model_row(c, ew)
        clean = run_once(c, ew)
        assert_rows(clean, want, f"Ep {Ep} Et {Et} width {ew}")
        p = dict(c, edge=c["edge"].copy(), tlabel=c["tlabel"].copy())
        p["edge"][:, w:] = np.nan
        p["tlabel"][:, w:] = np.nan
        assert np.array_equal(run_once(p, ew), clean), (Ep, Et, ew)
        if w == 0:
            assert clean[10:].tolist() == [0, 0, 0]


def test_decision_boundaries_on_exact_values():
    """0.5 and a probability equal to edge_threshold are not predicted, the next float32 is; a pair at distance exactly
    distance_thresh (difference (0.75, 1, 0), threshold 1.25) is within, the next float32 above is not."""
    up = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))      # noqa: E731
    out4 = np.zeros((1, 3, 4), np.float32)
    tverts = np.array([[[0.75, 1.0, 0.0], [0.75, up(1.0), 0.0], [0.75, -1.0, 0.0]]], np.float32)
    c = dict(out4=out4, tverts=tverts, exist=np.array([[0.5, up(0.5), 0.25]], np.float32), texist=np.ones((1, 3), np.float32),
             edge=np.array([[0.625, up(0.625), 0.5, 0.75]], np.float32), tlabel=np.array([[1, 1, 1, 0]], np.float32),
             col4row=np.array([[0, 1, 2]], np.int32), counts=np.array([3], np.int64))
    row = run_once(c, edge_threshold=0.625, distance_thresh=1.25)
    assert_rows(row, model_row(c, edge_threshold=0.625, distance_thresh=1.25), "boundaries")
    got = dict(zip(TM.COLUMNS, row.tolist()))
    assert got["n_pairs"] == 3 and got["n_within"] == 2 and got["sum_sq"] > 3 * 1.5625
    assert (got["ex_tp"], got["ex_fp"], got["ex_fn"], got["count_abs_err"]) == (1, 0, 2, 2)
    assert (got["ed_tp"], got["ed_fp"], got["ed_fn"]) == (1, 1, 2)


def test_unmatched_entries_and_a_nan_coordinate():
    c = make(2, 6, 6, 15, 15, [4, 6], seed=4)
    c["col4row"][0] = [-1, 4, 6, 0, 3, 2]                # -1, c_b = 4 and V = 6 are unmatched: three pairs, not c_b
    c["col4row"][1] = [5, -1, 6, 1, 100000, -2147483648]
    row = run_once(c)
    assert_rows(row, model_row(c), "unmatched entries")
    assert row[2] == 3 + 2
    c["out4"][0, 3, 1] = np.nan                          # a matched slot's coordinate
    c["exist"][1, 2] = np.nan
    c["edge"][0, 3] = np.nan
    c["tlabel"][1, 4] = np.nan
    row = run_once(c)
    want = model_row(c)
    assert math.isnan(row[3]) and math.isnan(row[4]) and row[2] == 5
    assert_rows(row, want, "NaN inputs")


def test_running_row_reset_and_repeatability():
    from wf3d.meter import WireframeMeter
    a, b = make(2, 260, 260, 33670, 33670, [3, 260], seed=5), make(2, 260, 260, 33670, 33670, [200, 17], seed=6)
    states = []
    for _ in range(2):
        qm = WireframeMeter(dev())
        qm.update(*to_device(a))
        qm.update(*to_device(b))
        states.append(qm.state.clone())
    assert torch.equal(states[0], states[1])
    want = TM.state_after([model_row(a), model_row(b)])
    assert_rows(states[0].cpu().numpy(), want, "two updates")
    m = qm.read()
    assert m["running"]["updates"] == 2 and m["running"]["n_samples"] == 4 and m["last"]["updates"] == 1
    assert m["running"]["n_pairs"] == 263 + 217 and m["last"]["n_pairs"] == 217
    assert abs(m["running"]["matched_rmse"] - math.sqrt(want[1, 3] / (3 * 480))) <= 1e-12
    assert m["last"]["count_mae"] == want[0, 9] / 2 and 0 < m["last"]["edge_f1"] < 1
    qm.reset()
    s = qm.state.cpu().numpy()
    assert not s[1].any() and np.array_equal(s[0], states[0][0].cpu().numpy())
    qm.update(*to_device(a))
    assert_rows(qm.state.cpu().numpy(), TM.state_after([model_row(a)]), "after reset")


def _loss_batch(B, V, seed):
    g = torch.Generator().manual_seed(seed)
    E = V * (V - 1) // 2
    counts = torch.tensor([3, 8, 5])[:B]
    pred = {"vertices": torch.randn(B, V, 4, generator=g).to(dev())[:, :, :3],
            "existence_probabilities": torch.rand(B, V, generator=g).to(dev()),
            "edge_probs": torch.rand(B, E, generator=g).to(dev())}
    tgt = {"vertices": torch.randn(B, V, 3, generator=g).to(dev()),
           "vertex_existence": (torch.arange(V)[None] < counts[:, None]).float().to(dev()),
           "edge_labels": (torch.rand(B, E, generator=g) > 0.7).float().to(dev()), "vertex_counts": counts.to(dev())}
    return pred, tgt


def test_both_assignment_modes_of_the_loss_feed_the_meter():
    """Gaussian coordinates: no cost ties, so the device solver and scipy find the same matching."""
    from losses.WireframeLoss import WireframeLoss
    from wf3d.meter import WireframeMeter
    pred, tgt = _loss_batch(3, 8, seed=7)
    states, assigns = {}, {}
    for mode in ("device", "scipy"):
        crit = WireframeLoss(assignment=mode)
        assert crit.last_assignment is None
        res = crit(pred, tgt)
        assert set(res) == {"total_loss", "vertex_loss", "existence_loss", "edge_loss"}
        a = crit.last_assignment
        assert a.is_cuda and a.dtype == torch.int32 and tuple(a.shape) == (3, 8)
        qm = WireframeMeter(dev(), distance_thresh=1.5)
        qm.update(pred, tgt, a)
        states[mode], assigns[mode] = qm.state.clone(), a.cpu().numpy()
        want = TM.batch_row(pred["vertices"].cpu().numpy(), pred["existence_probabilities"].cpu().numpy(),
                            pred["edge_probs"].cpu().numpy(), tgt["vertices"].cpu().numpy(), tgt["vertex_existence"].cpu().numpy(),
                            tgt["edge_labels"].cpu().numpy(), assigns[mode], tgt["vertex_counts"].cpu().numpy(), None, 0.5, 1.5)
        assert_rows(states[mode][0].cpu().numpy(), want, f"loss, assignment={mode}")
    cnt = tgt["vertex_counts"].cpu().numpy()[:, None]
    matched = assigns["device"] < cnt
    assert np.array_equal(matched, assigns["scipy"] < cnt) and np.array_equal(assigns["device"][matched], assigns["scipy"][matched])
    assert (assigns["scipy"][~matched] == 8).all()
    assert torch.equal(states["device"], states["scipy"])
    assert states["device"][0, 2] == 16 and 0 < states["device"][0, 5] < 16


def test_captured_loss_and_update_replay_bit_for_bit():
    """criterion(...) + update(...) captured once over static buffers (a padded head's device edge width among them);
    three replays on different contents and widths leave the state an eager meter reaches on the same contents."""
    from losses.WireframeLoss import WireframeLoss
    from wf3d.meter import WireframeMeter
    B, V = 3, 8
    E = V * (V - 1) // 2
    pred, tgt = _loss_batch(B, V, seed=8)
    pred["edge_width"] = torch.tensor(E, dtype=torch.int64, device=dev())
    crit, qm = WireframeLoss(), WireframeMeter(dev(), distance_thresh=1.5)

    def step():
        crit(pred, tgt)
        qm.update(pred, tgt, crit.last_assignment)
    step()                                                   # the eager warm-up: workspace and library are there
    s = torch.cuda.Stream(dev())
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    qm.state.zero_()
    eager_crit, eager = WireframeLoss(), WireframeMeter(dev(), distance_thresh=1.5)
    seen = []
    for k, width in enumerate((E, 11, 0)):
        new_pred, new_tgt = _loss_batch(B, V, seed=20 + k)
        new_tgt["vertex_counts"] = torch.tensor([[8, 1, 4], [0, 6, 8], [2, 2, 7]][k], device=dev())
        for d, n in ((pred, new_pred), (tgt, new_tgt)):
            for key, t in n.items():
                d[key].copy_(t)
        pred["edge_width"].fill_(width)
        graph.replay()
        eager_crit(pred, tgt)
        eager.update(pred, tgt, eager_crit.last_assignment)
        torch.cuda.synchronize()
        assert torch.equal(qm.state, eager.state), (k, qm.state, eager.state)
        seen.append(qm.state[0].cpu().numpy().copy())
    assert qm.state[1, 0] == 3 and seen[2][10:].tolist() == [0, 0, 0] and seen[0][10:].sum() > 0
    assert not np.array_equal(seen[0], seen[1])


def test_update_refuses_wrong_dtypes_and_shapes():
    from wf3d.meter import WireframeMeter
    qm = WireframeMeter(dev())
    pred, tgt, a = to_device(make(2, 3, 3, 3, 3, [2, 3], seed=9))
    bad = (("p", "vertices", pred["vertices"].double()), ("p", "existence_probabilities", pred["edge_probs"][:, :2]),
           ("p", "edge_probs", pred["edge_probs"][:1]), ("t", "vertex_counts", tgt["vertex_counts"].int()),
           ("t", "vertex_existence", tgt["vertex_existence"][:, :2]), ("t", "vertices", tgt["vertices"][:, :, :2]),
           ("t", "edge_labels", tgt["edge_labels"].cpu()), ("p", "edge_width", torch.tensor(3, dtype=torch.int32, device=dev())))
    for which, key, t in bad:
        pd, td = dict(pred), dict(tgt)
        (pd if which == "p" else td)[key] = t
        with pytest.raises(RuntimeError, match="WireframeMeter"):
            qm.update(pd, td, a)
    with pytest.raises(RuntimeError, match="int32"):
        qm.update(pred, tgt, a.long())
    with pytest.raises(RuntimeError, match="WireframeMeter"):
        qm.update(pred, tgt, a[:, :2])
    assert not qm.state.any()
