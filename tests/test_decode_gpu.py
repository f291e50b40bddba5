"""Wireframe decoding on the device: wf3d_wireframe_decode against the numpy specification (wf3d/decode.py), every output
tensor exact (floats as bits); wf3d.postprocess.decode_wireframes over the prediction layouts; wf3d_eval_metrics_nv against
wf3d_eval_metrics; and evaluate_batch(decode=...) on its three paths against the specification plus compute_metrics."""
import numpy as np
import pytest
import torch

import evalmetrics_model
import helpers as H
from test_eval import _check_counters
from test_evalmetrics_gpu import INT_KEYS, _batch, _prism, _same
from test_evalpost_compact_gpu import _pred
from wf3d import decode

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
OUT = ("nverts", "dverts", "slots", "koff", "pairs", "seg", "kprob", "status")


def _tri(c):
    return c * (c - 1) // 2


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _kernel(verts, exist, probs, counts, existence_threshold=0.5, edge_threshold=0.5, merge_radius=None, drop_isolated=False):
    """One call of wf3d_wireframe_decode on strided inputs (`vertices` the [:, :, :3] view of [B, V, 4], existence a column
    of [B, V, 2]) into buffers filled with sentinels -> the arrays of decode.decode_batch."""
    from wf3d import _lib
    from wf3d.ops import _stream
    lib = _lib.load()
    B, V, _ = verts.shape
    max_e = probs.shape[1]
    v4 = torch.full((B, V, 4), 7.0)
    v4[:, :, :3] = torch.from_numpy(verts)
    e2 = torch.full((B, V, 2), 0.99)
    e2[:, :, 1] = torch.from_numpy(exist)
    v, e = v4.to(DEV)[:, :, :3], e2.to(DEV)[:, :, 1]
    pr, cnt = torch.from_numpy(probs).to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV)
    cap = B * max_e
    ints = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=DEV)           # noqa: E731
    flts = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device=DEV)        # noqa: E731
    o = {"nverts": ints(B), "dverts": flts(B, V, 3), "slots": ints(B, V), "koff": ints(B + 1), "pairs": ints(cap + 1, 2),
         "seg": flts(cap + 1, 2, 3), "kprob": flts(cap + 1), "status": ints(B)}
    ws_bytes = lib.wf3d_wireframe_decode_ws_bytes(B, V, max_e)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=DEV)
    _lib.check(lib.wf3d_wireframe_decode(v.data_ptr(), v.stride(0), v.stride(1), e.data_ptr(), e.stride(1), cnt.data_ptr(),
                                         pr.data_ptr(), B, V, max_e,
                                         float("-inf") if existence_threshold is None else existence_threshold, edge_threshold,
                                         -1.0 if merge_radius is None else merge_radius, int(drop_isolated),
                                         *(o[k].data_ptr() for k in OUT), ws.data_ptr(), ws_bytes, _stream()), "wireframe_decode")
    o = {k: t.cpu().numpy() for k, t in o.items()}
    K = int(o["koff"][B])
    assert 0 <= K <= cap
    for k in ("pairs", "seg", "kprob"):                          # rows at and past K are left untouched
        assert (o[k][K:] == (-7 if k == "pairs" else 7.0)).all(), k
        o[k] = o[k][:K]
    return o


def _check(verts, exist, probs, counts, **opts):
    got = _kernel(verts, exist, probs, counts, **opts)
    want = decode.decode_batch(verts, exist, probs, counts, **opts)
    for k in OUT:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, opts, got[k].shape, want[k].shape)
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (k, opts)
    return got


def _lattice_case(V):
    """B = 7 samples on an integer lattice (coincident slots, distances equal to the radius, equal z, -0.0), existence
    from 4 levels (ties) plus +-inf and NaN, probabilities from levels that include the threshold itself and NaN,
    non-finite coordinates, every kind of count, a probability row shorter than c (c - 1) / 2."""
    gen = np.random.RandomState(100 + V)
    B, span = 7, 3 if V <= 64 else 5
    verts = gen.randint(-span, span + 1, (B, V, 3)).astype(np.float32)
    verts[(verts == 0) & (gen.uniform(0, 1, verts.shape) < 0.5)] = -0.0
    exist = gen.choice(np.array([0.2, 0.6, 0.8, 0.95], np.float32), (B, V))
    max_e = _tri(V) - 3 if V >= 4 else _tri(V)
    probs = gen.choice(np.array([0.1, 0.5, 0.6, 0.7, 0.9, np.nan], np.float32), (B, max_e), p=[0.3, 0.15, 0.15, 0.15, 0.2, 0.05])
    counts = [0, 1, 2, V, V + 5, -2, V - 1]
    verts[3, V // 2, 1], verts[3, 0, 0], exist[3, 1] = np.nan, np.inf, np.nan
    exist[4, 0], exist[4, V - 1], probs[4, 0] = np.inf, -np.inf, np.inf
    return verts, exist, probs, counts


@pytest.mark.parametrize("V", [2, 3, 5, 64, 65, 256, 300])          # 300: more slots than the workgroup has threads
def test_kernel_matches_the_specification(V):
    verts, exist, probs, counts = _lattice_case(V)
    option_sets = [dict(), dict(merge_radius=0.0), dict(merge_radius=2.0), dict(merge_radius=2.0, drop_isolated=True),
                   dict(existence_threshold=None, merge_radius=5.0 ** 0.5, edge_threshold=0.6),
                   dict(existence_threshold=None, drop_isolated=True)]
    merged = 0
    for opts in option_sets if V < 256 else option_sets[2:5]:
        got = _check(verts, exist, probs, counts, **opts)
        assert got["status"].tolist() == [0, 0, 0, 1, 0, 0, 0]
        merged += opts.get("merge_radius") is not None and int(got["nverts"][3]) < V - 3
    assert merged or V < 64                                      # the lattice does merge where it is dense


def test_hand_checked_cases():
    v = np.array([[(0, 0, 0), (3, 4, 0), (6, 8, 0), (50, 0, 0)]] * 4, dtype=np.float32)
    p = np.array([[.9, .9, .6, .9, .7, .8]] * 4, dtype=np.float32)
    ex = np.array([[.9, .8, .7, .6], [.8, .9, .7, .6], [.9, .8, .7, .6], [.7, .7, .7, .7]], dtype=np.float32)
    got = _check(v, ex, p, [4, 4, 4, 4], merge_radius=5.0)                   # the chain in both orders; distance exactly r
    assert got["nverts"].tolist() == [3, 2, 3, 3] and got["slots"][1].tolist() == [1, 3, -1, -1]
    assert got["koff"].tolist() == [0, 3, 4, 7, 10]
    assert got["pairs"][:4].tolist() == [[0, 1], [0, 2], [1, 2], [0, 1]]
    assert got["kprob"][:4].tolist() == [np.float32(.9), np.float32(.7), np.float32(.8), np.float32(.8)]
    got = _check(v, ex, p, [4, 4, 4, 4], merge_radius=float(np.nextafter(5.0, 0.0)))
    assert got["nverts"].tolist() == [4, 4, 4, 4]
    for r in (1e9, float("inf")):                                            # everything merged into one vertex: no edge
        got = _check(v, ex, p, [4, 4, 4, 4], merge_radius=r)
        assert got["nverts"].tolist() == [1, 1, 1, 1] and got["koff"].tolist() == [0] * 5
        assert got["slots"][:, 0].tolist() == [0, 1, 0, 0]
        got = _check(v, ex, p, [4, 4, 4, 4], merge_radius=r, drop_isolated=True)
        assert got["nverts"].tolist() == [0, 0, 0, 0] and not got["dverts"].any()
    got = _check(v, ex, p, [4, 4, 4, 4], existence_threshold=0.95)           # nothing alive
    assert got["nverts"].tolist() == [0] * 4 and got["koff"].tolist() == [0] * 5 and (got["slots"] == -1).all()
    # V < 2 and max_e = 0 still decode the vertices and write koff = 0
    got = _check(v[:, :1], ex[:, :1], np.zeros((4, 0), np.float32), [1, 0, 1, 3])
    assert got["nverts"].tolist() == [1, 0, 1, 1] and got["koff"].tolist() == [0] * 5
    got = _check(v, ex, np.zeros((4, 0), np.float32), [4, 4, 4, 4], merge_radius=5.0)
    assert got["nverts"].tolist() == [3, 2, 3, 3] and got["koff"].tolist() == [0] * 5


def _samples_equal(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y) == sorted(("pred_vertices", "pd_edges", "pd_edges_vertices", "pd_edge_probs", "slots"))
        for k in x:
            assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and np.array_equal(_bits(x[k]), _bits(y[k])), k


def test_layouts_and_repeatability():
    """decode_wireframes on ragged and padded prediction dicts, strided and contiguous inputs: equal to the CPU path (the
    specification) in values, dtypes and shapes; two runs give the same bits."""
    from wf3d import postprocess
    from wf3d.functional import edge_index_lists
    verts, exist, probs, counts = _lattice_case(65)
    counts = [0, 1, 2, 65, 65, 30, 64]                           # what an edge index list can express
    probs[:, :] = np.where(np.isnan(probs), np.float32(0.9), probs)
    B, V = len(counts), 65
    full = np.full((B, _tri(V)), 0.9, np.float32)
    full[:, :probs.shape[1]] = probs
    opts = dict(merge_radius=2.0, drop_isolated=True)
    cpu = {"vertices": torch.from_numpy(verts), "existence_probabilities": torch.from_numpy(exist),
           "edge_probs": torch.from_numpy(full), "edge_indices": edge_index_lists(counts)}
    want = postprocess.decode_wireframes(cpu, **opts)
    assert sum(len(w["pd_edges"]) for w in want) > 100 and want[3]["pred_vertices"].shape[0] < 62
    e2 = torch.zeros(B, V, 2)
    e2[:, :, 0] = torch.from_numpy(exist)
    runs = []
    for layout in ("ragged", "padded"):
        for ex in (e2.to(DEV)[:, :, 0], torch.from_numpy(exist).to(DEV), torch.from_numpy(exist.T.copy()).to(DEV).T):
            pred = dict(_pred(verts, full, counts, layout), existence_probabilities=ex)
            assert not pred["vertices"].is_contiguous()
            got, d = postprocess.decode_wireframes(pred, **opts, keep_device=True)
            _samples_equal(got, want)
            assert sorted(d) == sorted(("koff", "seg", "dverts", "nverts", "status", "koff_host", "status_host"))
            assert d["koff"].dtype == torch.int32 and np.array_equal(d["koff"].cpu().numpy(), d["koff_host"])
            assert d["nverts"].cpu().tolist() == [len(w["slots"]) for w in want]
            runs.append(torch.cat([d["dverts"].reshape(-1).view(torch.int32), d["seg"][:int(d["koff_host"][B])].reshape(-1).view(torch.int32),
                                   d["koff"], d["nverts"], d["status"]]).cpu().numpy())
    assert all(np.array_equal(r, runs[0]) for r in runs[1:])
    assert want[1]["pd_edges"].shape == (0, 2) and want[0]["pred_vertices"].shape == (0, 3)


# ---- per-sample vertex counts in the device metrics ---------------------------------------------------------------------
def _metrics_call(entry, verts, d, labels, thresh, nverts=None):
    """wf3d_eval_metrics (entry "plain") or wf3d_eval_metrics_nv on the compacted batch `d`, as evaluate_batch calls it
    -> (the raw [B] distances | [B, 8] counters words, the first assignment)."""
    from wf3d import _lib
    from wf3d.ops import _stream
    lib = _lib.load()
    B, V = verts.shape[:2]
    n, m = np.diff(d["koff_host"]).astype(np.int64), labels.nsegs
    ooff, aoff = np.concatenate(([0], np.cumsum(n * m))), np.concatenate(([0], np.cumsum(np.minimum(n, m))))
    d_ooff = torch.from_numpy(ooff.astype(np.int64)).to(DEV)
    d_aoff = torch.from_numpy(aoff.astype(np.int32)).to(DEV)
    hd = torch.empty(max(int(ooff[-1]), 1), dtype=torch.float64, device=DEV)
    _lib.check(lib.wf3d_hausdorff_lines_batch(d["seg"].data_ptr(), d["koff"].data_ptr(), labels.lseg.data_ptr(), labels.loff.data_ptr(),
                                              d_ooff.data_ptr(), B, int((n * m).max()), 20, hd.data_ptr(), _stream()), "hausdorff")
    assign = torch.full((max(int(aoff[-1]), 1),), -7, dtype=torch.int32, device=DEV)
    out = torch.full((10 * B,), -7, dtype=torch.int32, device=DEV)
    total_lv, max_lv, max_long = int(labels.nverts.sum()), int(labels.nverts.max()), int(max(n.max(), m.max()))
    ws_bytes = lib.wf3d_eval_metrics_ws_bytes(B, V, total_lv, max_long)
    ws = torch.zeros(max(ws_bytes, 16), dtype=torch.uint8, device=DEV)
    head = (verts.data_ptr(), verts.stride(0), verts.stride(1), B, V)
    tail = (d["seg"].data_ptr(), d["koff"].data_ptr(), labels.lverts.data_ptr(), labels.lvoff.data_ptr(), labels.lseg.data_ptr(),
            labels.loff.data_ptr(), hd.data_ptr(), d_ooff.data_ptr(), d_aoff.data_ptr(), assign.data_ptr(), float(thresh), max_lv,
            total_lv, max_long, out[2 * B:].data_ptr(), out.data_ptr(), ws.data_ptr(), ws_bytes, _stream())
    if entry == "plain":
        _lib.check(lib.wf3d_eval_metrics(*head, *tail), "eval_metrics")
    else:
        _lib.check(lib.wf3d_eval_metrics_nv(*head, None if nverts is None else nverts.data_ptr(), *tail), "eval_metrics_nv")
    return out.cpu().numpy(), assign.cpu().numpy()


def test_eval_metrics_nv_with_full_counts_is_eval_metrics():
    from wf3d import postprocess
    g = H.load_golden("eval")
    good = [c for c in evalmetrics_model.cases(g) if not c[3]]
    verts, probs, counts = _batch(good)
    B, V = verts.shape[:2]
    pred = _pred(verts, probs, counts)
    _, d = postprocess.wireframes_compact(pred, keep_device=True)
    labels = postprocess.EvalLabels([torch.from_numpy(g["gt_v"])] * B, [torch.from_numpy(g["gt_e"])] * B, DEV)
    for thresh in (1, 0.5):
        plain = _metrics_call("plain", pred["vertices"], d, labels, thresh)
        assert (plain[0].reshape(-1)[2 * B:].reshape(B, 8)[:, 1] == V).all()
        for nverts in (None, torch.full((B,), V, dtype=torch.int32, device=DEV), torch.full((B,), V + 9, dtype=torch.int32, device=DEV)):
            nv = _metrics_call("nv", pred["vertices"], d, labels, thresh, nverts)
            assert np.array_equal(nv[0], plain[0]) and np.array_equal(nv[1], plain[1])


# ---- end to end ---------------------------------------------------------------------------------------------------------
def _noisy_prisms(B=5, V=20):
    """Predictions around the 12-vertex / 18-edge prism at generic (Gaussian) positions, so every optimal assignment is
    unique: slots 0..11 the label vertices plus noise, 12..15 second, less probable copies of slots 0..3 within the merge
    radius, 16..19 dead slots far away (one of them also a free live corner in sample 1); the label edges probable between
    either copy, a few other pairs probable too.  Sample 3 has a NaN coordinate in a slot below its count."""
    gt_v, gt_e = _prism()
    gen = np.random.RandomState(31)
    verts = gen.normal(150, 20, (B, V, 3)).astype(np.float32)
    verts[:, :12] = gt_v + gen.normal(0, 0.02, (B, 12, 3)).astype(np.float32)
    verts[:, 12:16] = verts[:, :4] + gen.normal(0, 0.003, (B, 4, 3)).astype(np.float32)
    exist = np.concatenate((gen.uniform(0.8, 0.99, (B, 12)), gen.uniform(0.55, 0.79, (B, 4)), gen.uniform(0, 0.3, (B, 4))), axis=1)
    exist = exist.astype(np.float32)
    exist[1, 17] = 0.9                                           # a live corner that matches nothing
    exist[2, 5] = 0.2                                            # a label corner the model missed
    counts = [V, V, V, V, 14]
    probs = gen.uniform(0.0, 0.45, (B, _tri(V))).astype(np.float32)
    for s, c in enumerate(counts):
        index = {(i, j): e for e, (i, j) in enumerate(zip(*np.triu_indices(c, 1)))}          # the pair order over c slots
        for u, v in gt_e:
            for a, b in ((u, v), (u + 12 if u < 4 else u, v + 12 if v < 4 else v)):
                if max(a, b) < c:
                    probs[s, index[(min(a, b), max(a, b))]] = gen.uniform(0.6, 0.99)
        probs[s, gen.choice(_tri(c), 6, replace=False)] = 0.8
    verts[3, 9, 1] = np.nan
    return gt_v, gt_e, verts, exist, probs, counts


def test_evaluate_batch_decode_paths_agree(monkeypatch):
    from eval import ap_calculator as ap
    from wf3d import postprocess
    gt_v, gt_e, verts, exist, probs, counts = _noisy_prisms()
    B = len(counts)
    opts = dict(existence_threshold=0.5, edge_threshold=0.5, merge_radius=0.05, drop_isolated=False)
    wf_v, wf_e = [torch.from_numpy(gt_v)] * B, [torch.from_numpy(gt_e)] * B
    # the specification plus compute_metrics, sample by sample
    want = ap.APCalculator(distance_thresh=0.1)
    spec = [decode.decode_wireframe(verts[s], exist[s], probs[s], counts[s], **opts) for s in range(B)]
    assert [w["status"] for w in spec] == [0, 0, 0, 1, 0] and [len(w["slots"]) for w in spec] == [12, 13, 11, 11, 12]
    for w in spec:
        postprocess._compute_sample(want, {"pred_vertices": w["vertices"], "pd_edges": w["edges"], "pd_edges_vertices": w["seg"]},
                                    gt_v, gt_e, evalmetrics_model.z_first(gt_v, gt_e), None)
    assert int(want.ap_dict["tp_fp_corners"]) == 59 and int(want.ap_dict["tp_edges"]) > 4 * 15

    def run(layout, **kw):
        calc, calls = ap.APCalculator(distance_thresh=0.1), []
        real = ap.APCalculator.compute_metrics
        monkeypatch.setattr(ap.APCalculator, "compute_metrics", lambda self, batch: calls.append(1) or real(self, batch))
        pred = dict(_pred(verts, probs, counts, layout), existence_probabilities=torch.from_numpy(exist).to(DEV))
        try:
            postprocess.evaluate_batch(pred, wf_v, wf_e, calc, decode=opts, **kw)
        finally:
            monkeypatch.undo()
        return calc, len(calls)

    for layout in ("ragged", "padded"):
        host, calls = run(layout)
        assert calls == B
        for k in INT_KEYS + ("distance", "wed"):
            assert float(host.ap_dict[k]) == float(want.ap_dict[k]), k                      # the same code on equal samples
        compact, calls = run(layout, compact=True)
        assert calls == B
        _same(want, compact, "compact")
        device, calls = run(layout, compact=True, metrics="device")
        assert calls == 1                                        # the sample the decode flagged, and no other
        _same(want, device, "device")
        labels = postprocess.EvalLabels(wf_v, wf_e, DEV)
        device, calls = run(layout, compact=True, metrics="device", labels=labels, threshold=0.5)
        assert calls == 1
        _same(want, device, "device, prepared labels")


# What evaluate_batch accumulated for the three fixture samples as one batch BEFORE it took `decode`: recorded on an MI355X
# from the build of the commit that precedes decoding, the same on its three paths (compact=False, compact=True,
# metrics="device"), floats as float.hex().
BEFORE_DECODE = {"tp_corners": 18, "tp_fp_corners": 36, "tp_fn_corners": 24, "tp_edges": 9, "tp_fp_edges": 19, "tp_fn_edges": 24,
                 "distance": float.fromhex("0x1.112452dfcbdaep+3"), "wed": float.fromhex("0x1.2cd16a8685d80p+0")}


def test_decode_none_is_the_existing_path():
    """decode=None on all three paths: the ap_dict recorded from the code path as it was before (integer counters equal,
    `distance` and `wed` to rtol 1e-12, the bound these paths hold among themselves), the counters recorded from the
    reference, and the default call."""
    from eval import ap_calculator as ap
    from wf3d import postprocess
    g = H.load_golden("eval")
    verts = np.stack([g[f"c{c}.vertices"] for c in range(3)])
    probs = np.stack([g[f"c{c}.probs"] for c in range(3)])
    labels = [torch.from_numpy(g["gt_v"])] * 3, [torch.from_numpy(g["gt_e"].astype(np.float32))] * 3
    ap.set_device(DEV)
    try:
        for kw in ({}, {"compact": True}, {"compact": True, "metrics": "device"}):
            explicit, default = ap.APCalculator(distance_thresh=1), ap.APCalculator(distance_thresh=1)
            postprocess.evaluate_batch(_pred(verts, probs, [int(g["V"])] * 3), *labels, explicit, decode=None, **kw)
            postprocess.evaluate_batch(_pred(verts, probs, [int(g["V"])] * 3), *labels, default, 0.5, **kw)
            _check_counters(explicit, g["c2.counters"], "batch")
            for k, want in BEFORE_DECODE.items():
                if isinstance(want, int):
                    assert int(explicit.ap_dict[k]) == want, (kw, k)
                else:
                    assert np.isclose(float(explicit.ap_dict[k]), want, rtol=1e-12, atol=0.0), (kw, k, explicit.ap_dict[k])
            assert all(float(explicit.ap_dict[k]) == float(default.ap_dict[k]) for k in explicit.ap_dict)
            assert int(explicit.ap_dict["tp_fp_corners"]) == 3 * int(g["V"])
    finally:
        ap.set_device(None)
