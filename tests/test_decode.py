"""Wireframe decoding, the specification (wf3d/decode.py: existence filter, greedy vertex merging, edge re-indexing): the
hand-checked example value for value, its invariants on random lattice inputs (checked as properties, not against a copy
of the code), the identity settings against tests/evalpost_model.py, the metrics of a prediction with duplicate and dead
slots around a golden wireframe, and the argument checks of wf3d_wireframe_decode that need no launch."""
import os

import numpy as np
import pytest
import torch

import evalpost_model
import helpers as H
from wf3d import decode

IDENTITY = dict(existence_threshold=None, merge_radius=None, drop_isolated=False)


def _tri(c):
    return c * (c - 1) // 2


# ---- the example of the specification ---------------------------------------------------------------------------------
EXAMPLE_V = np.array([(0, 0, 0), (3, 4, 0), (6, 8, 0), (50, 0, 0)], dtype=np.float32)
EXAMPLE_P = np.array([.9, .9, .6, .9, .7, .8], dtype=np.float32)


@pytest.mark.parametrize("existence, slots, edges, kprob", [
    ([.9, .8, .7, .6], [0, 2, 3], [(0, 1), (0, 2), (1, 2)], [.9, .7, .8]),
    ([.8, .9, .7, .6], [1, 3], [(0, 1)], [.8]),
])
def test_hand_checked_example(existence, slots, edges, kprob):
    w = decode.decode_wireframe(EXAMPLE_V, np.array(existence, np.float32), EXAMPLE_P, 4, merge_radius=5, edge_threshold=0.5)
    assert w["slots"].tolist() == slots and w["slots"].dtype == np.int64
    assert np.array_equal(w["vertices"], EXAMPLE_V[slots]) and w["vertices"].dtype == np.float32
    assert w["edges"].tolist() == [list(e) for e in edges] and w["edges"].dtype == np.int64
    assert np.array_equal(w["kprob"], np.array(kprob, np.float32))
    assert w["status"] == 0
    # equal z at both ends: vertex b comes first
    assert np.array_equal(w["seg"], np.stack([(EXAMPLE_V[slots[b]], EXAMPLE_V[slots[a]]) for a, b in edges]))


def test_distance_exactly_the_radius_merges_and_just_below_does_not():
    ex = np.array([.9, .8, .7, .6], np.float32)
    assert decode.decode_wireframe(EXAMPLE_V, ex, EXAMPLE_P, 4, merge_radius=5.0)["rep"].tolist() == [0, 0, 2, 3]
    below = float(np.nextafter(np.float64(5.0), 0.0))
    assert decode.decode_wireframe(EXAMPLE_V, ex, EXAMPLE_P, 4, merge_radius=below)["rep"].tolist() == [0, 1, 2, 3]
    # None merges nothing, 0.0 coincident vertices only (-0.0 coincides with 0.0)
    v = np.array([(0, 0, 0), (-0.0, 0, -0.0), (0, 0, 1e-30)], np.float32)
    ex = np.array([.9, .9, .9], np.float32)
    assert decode.decode_wireframe(v, ex, np.ones(3, np.float32), 3, merge_radius=None)["rep"].tolist() == [0, 1, 2]
    assert decode.decode_wireframe(v, ex, np.ones(3, np.float32), 3, merge_radius=0.0)["rep"].tolist() == [0, 0, 2]


def test_non_finite_slots_are_dropped_and_flagged():
    v = np.array([(0, 0, 0), (np.nan, 0, 0), (1, 0, 0), (2, np.inf, 0), (3, 0, 0), (np.nan, 0, 0)], np.float32)
    ex = np.array([.9, .9, np.nan, .9, np.inf, .9], np.float32)
    w = decode.decode_wireframe(v, ex, np.full(15, .9, np.float32), 5, existence_threshold=None)
    assert w["slots"].tolist() == [0, 4] and w["status"] == decode.NONFINITE and w["edges"].tolist() == [[0, 1]]
    # the bad slot 5 lies past the count: not flagged
    assert decode.decode_wireframe(v[[0, 4, 5]], ex[[0, 4, 5]], np.zeros(3, np.float32), 2)["status"] == 0
    for bad in ({"merge_radius": np.nan}, {"edge_threshold": np.nan}, {"existence_threshold": np.nan}):
        with pytest.raises(ValueError, match="NaN"):
            decode.decode_wireframe(v, ex, np.zeros(15, np.float32), 5, **bad)


# ---- invariants -------------------------------------------------------------------------------------------------------
def _lattice(gen, V):
    """integer lattice coordinates (many distances equal the radius exactly), 4 existence levels (ties are common)"""
    verts = gen.randint(-3, 4, (V, 3)).astype(np.float32)
    exist = gen.choice(np.array([0.2, 0.6, 0.8, 0.95], np.float32), V)
    count = int(gen.choice([V, V, max(V - 1, 0), V + 3]))
    max_e = int(gen.choice([_tri(V), max(_tri(V) - 2, 0)]))
    probs = gen.choice(np.array([0.1, 0.5, 0.6, 0.7, 0.9], np.float32), max_e)
    return verts, exist, probs, count


def _d2(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)                  # lattice points: exact in integers
    return int((d * d).sum())


@pytest.mark.parametrize("V", [2, 3, 5, 17, 64])
def test_invariants_on_lattice_inputs(V):
    gen = np.random.RandomState(40 + V)
    for trial in range(12 if V < 64 else 4):
        verts, exist, probs, count = _lattice(gen, V)
        r = float(gen.choice([0.0, 1.0, 2.0, 3.0, 5.0 ** 0.5]))
        r2 = float(np.float64(r) * np.float64(r))
        c = min(count, V)
        for drop in (False, True):
            w = decode.decode_wireframe(verts, exist, probs, count, existence_threshold=0.5, edge_threshold=0.5, merge_radius=r,
                                        drop_isolated=drop)
            rep = w["rep"]
            alive = (np.arange(V) < c) & (exist > np.float32(0.5))
            assert np.array_equal(rep >= 0, alive)
            order = [int(i) for i in np.lexsort((np.arange(V), -exist.astype(np.float64))) if alive[i]]
            place = {i: t for t, i in enumerate(order)}
            reps = [i for i in order if rep[i] == i]
            # no two representatives within r
            for a in reps:
                for b in reps:
                    assert a == b or _d2(verts[a], verts[b]) > r2, (a, b)
            # a merged slot: within r of its representative, which precedes it, and of no earlier representative
            for i in order:
                k = int(rep[i])
                if k == i:
                    continue
                assert k in reps and place[k] < place[i] and _d2(verts[i], verts[k]) <= r2
                assert all(_d2(verts[i], verts[q]) > r2 for q in reps if place[q] < place[k])
            # the output edges: exactly the image of the surviving candidates, each with its maximum probability
            image = {}
            iu = np.stack(np.triu_indices(c, 1), axis=1)[:len(probs)] if c >= 2 else np.empty((0, 2), np.int64)
            for e, (i, j) in enumerate(iu):
                if alive[i] and alive[j] and probs[e] > np.float32(0.5) and rep[i] != rep[j]:
                    key = (min(rep[i], rep[j]), max(rep[i], rep[j]))
                    image[key] = max(image.get(key, -np.inf), float(probs[e]))
            got = {(int(w["slots"][a]), int(w["slots"][b])): float(p) for (a, b), p in zip(w["edges"], w["kprob"])}
            assert got == image
            assert w["edges"].tolist() == sorted(w["edges"].tolist()) and (len(w["edges"]) == 0 or (w["edges"][:, 0] < w["edges"][:, 1]).all())
            # the vertices: representatives in slot order; with drop_isolated every one has an edge
            ends = {k for key in image for k in key}
            assert w["slots"].tolist() == sorted(i for i in reps if not drop or i in ends)
            assert np.array_equal(w["vertices"], verts[w["slots"]])
            if drop:
                assert set(w["edges"].reshape(-1).tolist()) == set(range(len(w["slots"])))
            # every segment end point is a row of the vertex array, higher z first
            for (a, b), sg in zip(w["edges"], w["seg"]):
                hi, lo = (a, b) if w["vertices"][a, 2] > w["vertices"][b, 2] else (b, a)
                assert np.array_equal(sg, w["vertices"][[hi, lo]])


# ---- identity settings ------------------------------------------------------------------------------------------------
def test_identity_settings_equal_the_compaction():
    gen = np.random.RandomState(7)
    B, V = 7, 9
    verts = gen.normal(0, 3, (B, V, 3)).astype(np.float32)
    verts[0, 1, 2] = verts[0, 2, 2] = verts[0, 4, 2]            # equal z
    verts[1, 3] = verts[1, 5]                                    # coincident: merge_radius=None keeps both
    exist = gen.uniform(0, 1, (B, V)).astype(np.float32)
    counts = [9, 0, 1, 2, 5, 12, -3]
    for max_e in (_tri(V), _tri(V) - 7):
        probs = gen.uniform(0, 1, (B, max_e)).astype(np.float32)
        probs[0, :3], probs[4, 1] = (0.5, np.nan, 0.9), np.nan
        d = decode.decode_batch(verts, exist, probs, counts, edge_threshold=0.5, **IDENTITY)
        clamped = [min(max(c, 0), V) for c in counts]
        koff, pairs, seg, kprob = evalpost_model.compact(clamped, probs, verts, 0.5)
        assert np.array_equal(d["koff"], koff) and np.array_equal(d["pairs"], pairs)
        assert np.array_equal(d["seg"], seg) and np.array_equal(d["kprob"], kprob)
        assert d["nverts"].tolist() == clamped and not d["status"].any()
        for s, c in enumerate(clamped):
            assert np.array_equal(d["dverts"][s, :c], verts[s, :c]) and not d["dverts"][s, c:].any()
            assert d["slots"][s].tolist() == list(range(c)) + [-1] * (V - c)


# ---- metrics on the golden wireframe ----------------------------------------------------------------------------------
def _duplicated_prediction():
    """V = 24 slots around the 8-vertex label: every label vertex twice (jitter far below the merge radius, the two
    copies with different existence), 8 dead slots far away; the label edges probable between either copy."""
    from datasets.building3d import load_wireframe
    gt_v, gt_e = load_wireframe(os.path.join(H.GOLDEN, "building3d", "train", "wireframe", "100.obj"))
    gt_v = (gt_v - gt_v.mean(axis=0)).astype(np.float32)
    gt_e = np.array(sorted(map(tuple, gt_e)), dtype=np.int64)
    L, V = len(gt_v), 24
    assert L == 8 and len(gt_e) == 8
    gen = np.random.RandomState(3)
    verts = np.empty((V, 3), np.float32)
    verts[:L] = gt_v + gen.normal(0, 0.004, (L, 3)).astype(np.float32)
    verts[L:2 * L] = gt_v + gen.normal(0, 0.004, (L, 3)).astype(np.float32)
    verts[2 * L:] = gen.uniform(100, 200, (V - 2 * L, 3)).astype(np.float32)
    exist = np.concatenate((gen.uniform(0.8, 0.99, L), gen.uniform(0.6, 0.79, L), gen.uniform(0.0, 0.3, V - 2 * L))).astype(np.float32)
    exist[[1, L + 1]] = exist[[L + 1, 1]]                        # for one vertex the second copy is the more probable
    index = {(i, j): e for e, (i, j) in enumerate(zip(*np.triu_indices(V, 1)))}
    probs = gen.uniform(0.0, 0.4, _tri(V)).astype(np.float32)
    for u, v in gt_e:
        for a, b, p in ((u, v, 0.9), (u + L, v + L, 0.8), (u, v + L, 0.7), (u + L, v, 0.95)):
            probs[index[(min(a, b), max(a, b))]] = p
    for u in range(L):
        probs[index[(u, u + L)]] = 0.9                           # an edge between the two copies of one corner
    probs[index[(0, 2 * L)]] = probs[index[(2 * L, 2 * L + 1)]] = 0.9        # edges that touch dead slots
    return gt_v, gt_e, verts, exist, probs


def _z_first(v, e):
    ev = np.stack((v[e[:, 0]], v[e[:, 1]]), axis=1)
    return ev[np.arange(len(ev))[:, None], np.flip(np.argsort(ev[:, :, -1]), axis=1)]


def test_metrics_count_corners_not_slots():
    from eval import ap_calculator as ap
    from wf3d import postprocess
    from wf3d.functional import edge_index_lists
    gt_v, gt_e, verts, exist, probs = _duplicated_prediction()
    V = len(verts)
    # the reference's evaluation: every slot is a predicted corner
    ref = ap.APCalculator(distance_thresh=0.1)
    pd_e = np.stack(np.triu_indices(V, 1), axis=1)[probs > 0.5]
    ref.compute_metrics({"predicted_vertices": verts[None], "predicted_edges": pd_e[None],
                         "pred_edges_vertices": _z_first(verts, pd_e).reshape(1, -1, 2, 3), "wf_vertices": gt_v[None],
                         "wf_edges": gt_e[None], "wf_edges_vertices": _z_first(gt_v, gt_e).reshape(1, -1, 2, 3)})
    assert int(ref.ap_dict["tp_fp_corners"]) == 24 and int(ref.ap_dict["tp_fp_edges"]) > len(gt_e)
    pred = {"vertices": torch.from_numpy(verts)[None], "existence_probabilities": torch.from_numpy(exist)[None],
            "edge_probs": torch.from_numpy(probs)[None], "edge_indices": edge_index_lists([V])}
    calc = ap.APCalculator(distance_thresh=0.1)
    postprocess.evaluate_batch(pred, [torch.from_numpy(gt_v)], [torch.from_numpy(gt_e)], calc,
                               decode={"merge_radius": 0.05, "existence_threshold": 0.5})
    assert int(calc.ap_dict["tp_fp_corners"]) == len(gt_v) == int(calc.ap_dict["tp_fn_corners"])
    assert int(calc.ap_dict["tp_corners"]) == len(gt_v)                      # corner precision 1.0
    assert int(calc.ap_dict["tp_fp_edges"]) == len(gt_e) == int(calc.ap_dict["tp_edges"])
    w = postprocess.decode_wireframes(pred, merge_radius=0.05)[0]
    assert w["slots"].tolist() == [0, 2, 3, 4, 5, 6, 7, 9] and w["slots"].dtype == np.int64
    assert w["pred_vertices"].shape == (8, 3) and w["pd_edges"].max() < 8 and len(w["pd_edge_probs"]) == len(gt_e)
    assert np.array_equal(w["pd_edge_probs"], np.full(len(gt_e), 0.95, np.float32))         # the maximum over the four copies
    with pytest.raises(ValueError, match="differ"):
        postprocess.evaluate_batch(pred, [torch.from_numpy(gt_v)], [torch.from_numpy(gt_e)], calc, threshold=0.4,
                                   decode={"edge_threshold": 0.5})
    # the device tensors exist for the batched kernels only: CPU predictions have none
    with pytest.raises(ValueError, match="needs CUDA predictions"):
        postprocess.decode_wireframes(pred, keep_device=True)
    with pytest.raises(ValueError, match="needs CUDA predictions"):
        postprocess.evaluate_batch(pred, [torch.from_numpy(gt_v)], [torch.from_numpy(gt_e)], calc, compact=True,
                                   decode={"merge_radius": 0.05})
    with pytest.raises(ValueError, match="unknown decode option"):
        postprocess.evaluate_batch(pred, [torch.from_numpy(gt_v)], [torch.from_numpy(gt_e)], calc, decode={"radius": 0.05})


# ---- the C entry point's argument checks (nothing is launched) ---------------------------------------------------------
def test_argument_errors_are_reported_without_a_launch():
    from wf3d import _lib
    lib = _lib.load()
    D = _lib.DEFINES
    assert D["WF3D_DECODE_NONFINITE"] == decode.NONFINITE == 1

    def call(B=2, V=4, max_e=6, ethr=0.5, thr=0.5, r=0.1, ws_bytes=0):
        return lib.wf3d_wireframe_decode(None, 0, 0, None, 1, None, None, B, V, max_e, ethr, thr, r, 0, None, None, None, None,
                                         None, None, None, None, None, ws_bytes, None)
    assert call(V=1025) == D["WF3D_ERR_UNSUPPORTED"] and b"1024" in lib.wf3d_last_error()
    assert call(B=65536) == D["WF3D_ERR_UNSUPPORTED"] and b"65535" in lib.wf3d_last_error()
    assert call(B=65535, V=400, max_e=40000) == D["WF3D_ERR_UNSUPPORTED"] and b"2^31" in lib.wf3d_last_error()
    for bad in ({"ethr": float("nan")}, {"thr": float("nan")}, {"r": float("nan")}):
        assert call(**bad) == D["WF3D_ERR_ARG"] and b"NaN" in lib.wf3d_last_error()
    assert call(B=-1) == D["WF3D_ERR_ARG"]
    need = lib.wf3d_wireframe_decode_ws_bytes(2, 4, 6)
    assert need >= 2 * 4 * 4 * 4
    assert call(ws_bytes=need - 1) == D["WF3D_ERR_WS"] and b"workspace" in lib.wf3d_last_error()
    assert call(B=0) == 0                                                    # B = 0 launches nothing
    ws = lib.wf3d_wireframe_decode_ws_bytes
    assert ws(0, 64, 2016) == 0 and ws(4, 1, 0) == 0 and ws(4, 64, 0) == 0
    for B, V, max_e in ((1, 2, 1), (4, 64, 2016), (32, 256, 32640), (7, 1024, 100)):
        assert ws(B, V, max_e) <= ws(B + 1, V, max_e) and ws(B, V, max_e) <= ws(B, V + 1, max_e) <= ws(B, 2 * V, max_e)
        assert ws(B, V, max_e) <= ws(B, V, max_e + 1) and ws(B, V, max_e) >= 4 * B * V * V
