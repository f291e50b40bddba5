"""Edge labels that follow the matching, on the host: the numpy specification wf3d.targets.matched_edge_labels (what
wf3d_edge_labels_matched computes on the device), the constructor of WireframeLoss's edge options, and every refusal of
the two new C entry points, which return before any launch and so without a GPU."""
import ctypes
import os

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import helpers as H

OBJ_DIR = os.path.join(H.GOLDEN, "building3d", "train", "wireframe")


@pytest.mark.parametrize("d", [2, 3, 64, 65, 1024])
def test_unranking_equals_the_nested_loops(d):
    from wf3d.targets import _pair_index, _pair_unrank
    ref = np.array([(p, q) for p in range(d) for q in range(p + 1, d)], dtype=np.int64)
    p, q = _pair_unrank(np.arange(len(ref)), d)
    assert np.array_equal(p, ref[:, 0]) and np.array_equal(q, ref[:, 1])
    assert np.array_equal(_pair_index(p, q, d), np.arange(len(ref)))


def test_identity_assignment_reproduces_the_positional_labels():
    from wf3d.targets import matched_edge_labels
    rng = np.random.default_rng(3)
    B, V = 4, 7
    counts = np.array([7, 4, 0, 2])
    Et = V * (V - 1) // 2
    tl = np.zeros((B, Et), np.float32)
    for b, c in enumerate(counts):                       # what train_targets writes: zeros past a sample's own pairs
        tl[b, :c * (c - 1) // 2] = rng.random(c * (c - 1) // 2) > 0.5
    ident = np.tile(np.arange(V), (B, 1))
    for Ep in (Et, Et - 5, 3, 0):
        assert np.array_equal(matched_edge_labels(tl, ident, counts, Ep), tl[:, :Ep])
    # d_b != c_b: the same pairs of vertices sit at other columns
    out = matched_edge_labels(tl, ident, counts, Et, pair_counts=np.full(B, V))
    for b, c in enumerate(counts):
        k = 0
        for p in range(V):
            for q in range(p + 1, V):
                want = tl[b, p * c - p * (p + 1) // 2 + q - p - 1] if q < c else 0.0
                assert out[b, k] == want, (b, p, q)
                k += 1


def test_spec_against_a_loop_model():
    """Unmatched slots (V, negative), a repeated target, counts clamped, narrow labels, wide output."""
    from wf3d.targets import matched_edge_labels
    rng = np.random.default_rng(11)
    B, V, Et, Ep = 5, 6, 9, 20
    tl = (rng.random((B, Et)) > 0.4).astype(np.float32)
    a = np.stack([rng.permutation(V) for _ in range(B)]).astype(np.int32)
    a[1, 2], a[2, 0], a[3, 4] = V, -3, a[3, 1]
    counts, pair = np.array([6, 4, 9, 3, -2]), np.array([6, 6, 3, 7, 5])
    out = matched_edge_labels(tl, a, counts, Ep, pair)
    for b in range(B):
        c, d = min(max(int(counts[b]), 0), V), min(max(int(pair[b]), 0), V)
        want = np.zeros(Ep, np.float32)
        k = 0
        for p in range(d):
            for q in range(p + 1, d):
                tp, tq = int(a[b, p]), int(a[b, q])
                if k < Ep and 0 <= tp < c and 0 <= tq < c and tp != tq:
                    lo, hi = min(tp, tq), max(tp, tq)
                    i = lo * c - lo * (lo + 1) // 2 + hi - lo - 1
                    want[k] = tl[b, i] if i < Et else 0.0
                k += 1
        assert np.array_equal(out[b], want), b


# slot p of the permuted-perfect prediction holds ground-truth vertex PERM[name][p] (to 1e-3)
PERM = {"100": [2, 4, 3, 6, 5, 0, 1, 7], "10040": [2, 0, 1, 3]}


@pytest.mark.parametrize("name, n_edges, positional_right", [("100", 8, 1), ("10040", 4, 2)])
def test_permuted_perfect_prediction_on_the_golden_wireframes(name, n_edges, positional_right):
    """A model that predicts every vertex to 1e-3 in another slot order: the matched labels mark exactly the true edges,
    the positional ones mark 1 of 8 and 2 of 4."""
    from datasets.building3d import load_wireframe
    from wf3d.targets import matched_edge_labels, train_targets
    v, e = load_wireframe(os.path.join(OBJ_DIR, name + ".obj"))
    c = len(v)
    assert len(e) == n_edges
    perm = np.array(PERM[name])
    assert sorted(perm.tolist()) == list(range(c))
    t = train_targets([v], [e], c)
    tl = t["edge_labels"].numpy()
    pred = t["vertices"].numpy()[0][perm] + 1e-3 * np.random.default_rng(1).standard_normal((c, 3)).astype(np.float32)
    cost = np.abs(pred[:, None, :] - t["vertices"].numpy()[0][None, :, :]).sum(-1)       # existence 1: no further term
    rows, cols = linear_sum_assignment(cost)
    assert np.array_equal(rows, np.arange(c)) and np.array_equal(cols, perm)
    m = matched_edge_labels(tl, cols[None, :], [c], c * (c - 1) // 2)[0]
    edges = {(min(a, b), max(a, b)) for a, b in e.tolist()}
    pairs = [(p, q) for p in range(c) for q in range(p + 1, c)]
    truth = np.array([(min(perm[p], perm[q]), max(perm[p], perm[q])) in edges for p, q in pairs], dtype=np.float32)
    assert np.array_equal(m, truth) and int(m.sum()) == n_edges
    assert int(((tl[0] == 1) & (truth == 1)).sum()) == positional_right


def test_constructor_validation():
    from losses.WireframeLoss import WireframeLoss
    crit = WireframeLoss()
    assert (crit.edge_targets, crit.edge_pos_weight, crit.edge_focal_gamma) == ("positional", 1.0, 0.0)
    assert crit.last_edge_labels is None
    crit = WireframeLoss(edge_targets="matched", edge_pos_weight=4, edge_focal_gamma=2)
    assert (crit.edge_targets, crit.edge_pos_weight, crit.edge_focal_gamma) == ("matched", 4.0, 2.0)
    for kw in ({"edge_targets": "auto"}, {"edge_targets": None}, {"edge_pos_weight": 0.0}, {"edge_pos_weight": -1.0},
               {"edge_pos_weight": float("nan")}, {"edge_pos_weight": float("inf")}, {"edge_pos_weight": "auto"},
               {"edge_focal_gamma": -0.5}, {"edge_focal_gamma": float("nan")}, {"edge_focal_gamma": float("inf")},
               {"edge_focal_gamma": None}):
        with pytest.raises(ValueError):
            WireframeLoss(**kw)


def test_label_entry_refusals_without_gpu():
    from wf3d import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)           # never dereferenced: every call below returns before a launch
    ARG, UNSUPPORTED = _lib.DEFINES["WF3D_ERR_ARG"], _lib.DEFINES["WF3D_ERR_UNSUPPORTED"]
    f = lib.wf3d_edge_labels_matched
    # (tlabel, Et, col4row, counts, pair_counts, B, V, Ep, out, stream)
    for B, V, Ep, Et in ((-1, 4, 6, 6), (2, 0, 6, 6), (2, -4, 6, 6), (2, 4, -1, 6), (2, 4, 6, -1)):
        assert f(ptr, Et, ptr, ptr, None, B, V, Ep, ptr, None) == ARG
        assert b"bad dims" in lib.wf3d_last_error()
    for B, V, Ep, Et, word in ((2, 1025, 6, 6, b"V > 1024"), (65536, 4, 6, 6, b"B > 65535"),
                               (4096, 1024, 524288, 6, b"2^31"), (4096, 4, 6, 524288, b"2^31")):
        assert f(ptr, Et, ptr, ptr, None, B, V, Ep, ptr, None) == UNSUPPORTED
        assert word in lib.wf3d_last_error()
    for args in ((None, 6, ptr, ptr, None, 2, 4, 6, ptr), (ptr, 6, None, ptr, None, 2, 4, 6, ptr),
                 (ptr, 6, ptr, None, ptr, 2, 4, 6, ptr), (ptr, 6, ptr, ptr, ptr, 2, 4, 6, None)):
        assert f(*args, None) == ARG
        assert b"null pointer" in lib.wf3d_last_error()
    # nothing to write: no launch, no pointer needed
    assert f(None, 0, None, None, None, 0, 4, 6, None, None) == 0
    assert f(None, 0, None, None, None, 2, 4, 0, None, None) == 0


def test_balanced_entry_refusals_without_gpu():
    from wf3d import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)
    ARG = _lib.DEFINES["WF3D_ERR_ARG"]

    def call(w=4.0, gamma=2.0, B=2, V=4, Ep=6, Et=6, null=(), ws_bytes=1024):
        p = {k: (None if k in null else ptr) for k in ("verts", "exist", "edge", "tverts", "texist", "tlabel", "ew",
                                                       "col4row", "counts", "dverts", "dexist", "dedge", "losses", "ws")}
        return lib.wf3d_loss_terms_assigned_bal(p["verts"], V * 3, 3, p["exist"], p["edge"], Ep, p["tverts"], V, p["texist"],
                                                p["tlabel"], Et, p["ew"], p["col4row"], p["counts"], B, V, 1.0, 1.0, 1.0,
                                                w, gamma, p["dverts"], p["dexist"], p["dedge"], p["losses"], p["ws"],
                                                ws_bytes, None)
    for w, gamma in ((0.0, 0.0), (-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1.0, -0.5), (1.0, float("nan")),
                     (1.0, float("inf"))):
        assert call(w=w, gamma=gamma) == ARG
        assert b"edge_pos_weight" in lib.wf3d_last_error()
    for dims in ({"B": 0}, {"B": -1}, {"V": 0}, {"Ep": -1}, {"Et": -1}):
        assert call(**dims) == ARG
        assert b"bad dims" in lib.wf3d_last_error()
    for k in ("verts", "exist", "tverts", "texist", "col4row", "counts", "dverts", "dexist", "losses", "edge", "dedge"):
        assert call(null=(k,)) == ARG, k
        assert b"null" in lib.wf3d_last_error()
    assert call(null=("tlabel",)) == ARG and b"null edge labels" in lib.wf3d_last_error()      # a device width needs labels
    assert call(null=("ws",)) == _lib.DEFINES["WF3D_ERR_WS"]
    assert call(ws_bytes=2 * 3 * 4 - 1) == _lib.DEFINES["WF3D_ERR_WS"]
