"""CPU-side checks of the training metrics (wf3d.meter.WireframeMeter, csrc/metrics.hip): the C ABI declares and exports
the two entry points and refuses what it does not support before any launch; WireframeMeter.read() derives its ratios
from a state tensor written by hand, zero denominators included; and tests/train_metrics_model.py, the numpy model the
GPU tests hold the kernel to, gives the counters written out by hand for a 2-sample case."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import train_metrics_model as TM

HDR = os.path.join(H.ROOT, "include", "wf3d.h")
NAMES = ("wf3d_train_metrics_ws_bytes", "wf3d_train_metrics")


def test_header_declares_and_library_exports_the_entry_points():
    from wf3d import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, txt), f"include/wf3d.h does not declare {n}"
        assert n in _lib.SIGNATURES
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines()}
    assert set(NAMES) <= exported
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NAMES)


def test_workspace_size_and_limits_without_a_gpu():
    """One 64-byte record per sample and one 16-byte record per sample and 2048 edge columns; V > 1024 and B * Ep >= 2^31
    are WF3D_ERR_UNSUPPORTED, bad dims and null pointers WF3D_ERR_ARG, a short workspace WF3D_ERR_WS: all before a launch."""
    from wf3d import _lib
    lib = _lib.load()
    ws = lib.wf3d_train_metrics_ws_bytes
    assert ws(0, 10) == 0 and ws(3, 0) == 3 * 64
    assert ws(3, 1) == ws(3, 2048) == 3 * 64 + 3 * 16
    assert ws(32, 32640) == 32 * 64 + 32 * 16 * 16 and ws(2, 33670) == 2 * 64 + 2 * 17 * 16
    host = np.zeros(4096, dtype=np.float64)                  # host memory: no call below gets as far as a launch
    buf = host.ctypes.data

    def call(B=2, V=4, Vt=4, Ep=6, Et=6, ptr=buf, ws_bytes=4096 * 8):
        return lib.wf3d_train_metrics(ptr, V * 3, 3, ptr, ptr, Ep, ptr, Vt, ptr, ptr, Et, ptr, ptr, None, B, V, 0.5, 0.05,
                                      ptr, ptr, ws_bytes, None)
    assert call(V=1025) == _lib.DEFINES["WF3D_ERR_UNSUPPORTED"] and b"1024" in lib.wf3d_last_error()
    assert call(B=65536, Ep=32768, Et=4) == _lib.DEFINES["WF3D_ERR_UNSUPPORTED"]
    assert call(B=4096, Ep=1 << 19, Et=4) == _lib.DEFINES["WF3D_ERR_UNSUPPORTED"] and b"2^31" in lib.wf3d_last_error()
    assert call(B=0) == call(V=0) == call(Vt=0) == call(Ep=-1) == _lib.DEFINES["WF3D_ERR_ARG"]
    assert call(ptr=None) == _lib.DEFINES["WF3D_ERR_ARG"]
    assert call(ws_bytes=2 * 64 + 2 * 16 - 1) == _lib.DEFINES["WF3D_ERR_WS"]


def _hand_case():
    verts = np.array([[[0, 0, 0], [1, 0, 0], [5, 5, 5]], [[9, 9, 9], [1, 1, 1], [7, 7, 7]]], np.float32)
    tverts = np.array([[[1, 0, 2], [0.75, 1.0, 0], [5, 5, 5]], [[9, 9, 9], [7, 7, 7], [1, 1, 1]]], np.float32)
    exist = np.array([[0.9, 0.5, 0.6], [0.1, 0.2, 0.3]], np.float32)
    texist = np.array([[1, 1, 0], [1, 1, 1]], np.float32)
    edge = np.array([[0.9, 0.7, 0.2], [0.8, 0.8, 0.1]], np.float32)
    tlabel = np.array([[1, 0, 1], [0, 1, 0]], np.float32)
    col4row = np.array([[1, 0, 2], [-1, 2, 3]], np.int32)
    counts = np.array([2, 5], np.int64)
    return verts, exist, edge, tverts, texist, tlabel, col4row, counts


def test_model_on_a_case_counted_by_hand():
    """Sample 0 (count 2): slot 0 -> target 1 at distance 1.25 (d2 = 0.5625 + 1 = 1.5625, within a threshold of 1.25),
    slot 1 -> target 0 at distance 2 (d2 = 4, not within), slot 2 holds 2 = c_b: unmatched although its target row equals
    it.  Existence 0.9 / 0.5 / 0.6 against 1 / 1 / 0: tp, fn (0.5 is not predicted), fp; two predicted, count 2.  Edges
    0.9 / 0.7 / 0.2 at threshold 0.7 against 1 / 0 / 1: tp, nothing (0.7 is not predicted), fn.
    Sample 1 (count 5, clamped to 3): -1 unmatched, slot 1 -> target 2 at distance 0, 3 = c_b unmatched.  No vertex
    predicted against three labels: 3 fn, count error 3.  Edges 0.8 / 0.8 / 0.1 against 0 / 1 / 0: fp, tp."""
    row = TM.batch_row(*_hand_case(), edge_threshold=0.7, distance_thresh=1.25)
    want = dict(updates=1, n_samples=2, n_pairs=3, sum_sq=5.5625, sum_dist=3.25, n_within=2, ex_tp=1, ex_fp=1, ex_fn=4,
                count_abs_err=3, ed_tp=2, ed_fp=1, ed_fn=1)
    assert dict(zip(TM.COLUMNS, row.tolist())) == want
    # a device edge width of 2 drops column 2 (sample 0's fn); 0 and negative widths read nothing; past 3 is 3
    for width, ed in ((2, (2, 1, 0)), (0, (0, 0, 0)), (-3, (0, 0, 0)), (7, (2, 1, 1))):
        r = TM.batch_row(*_hand_case(), edge_width=width, edge_threshold=0.7, distance_thresh=1.25)
        assert tuple(r[10:]) == ed and np.array_equal(r[:10], row[:10])
    # the next float32 above the threshold's distance is not within
    case = list(_hand_case())
    case[3] = case[3].copy()
    case[3][0, 1, 1] = np.nextafter(np.float32(1.0), np.float32(2.0))
    assert TM.batch_row(*case, edge_threshold=0.7, distance_thresh=1.25)[5] == 1
    # NaN: the sums carry it, every integer counter stays what the comparisons (false) make it
    case = list(_hand_case())
    case[0] = case[0].copy()
    case[0][0, 0, 2] = np.nan
    case[1] = case[1].copy()
    case[1][0, 2] = np.nan
    r = TM.batch_row(*case, edge_threshold=0.7, distance_thresh=1.25)
    assert math.isnan(r[3]) and math.isnan(r[4])
    assert r[TM.INT_COLUMNS].tolist() == [1, 2, 3, 1, 1, 0, 4, 4, 2, 1, 1]      # slot 2 of sample 0 is no longer predicted
    s = TM.state_after([row, row])
    assert np.array_equal(s[0], row) and np.array_equal(s[1], 2 * row)


def test_read_derives_its_ratios_from_a_state_written_by_hand():
    from wf3d.meter import WireframeMeter
    assert WireframeMeter.COLUMNS == TM.COLUMNS
    qm = WireframeMeter(torch.device("cpu"), distance_thresh=0.1, edge_threshold=0.6)
    assert qm.state.shape == (2, 13) and qm.state.dtype == torch.float64 and not qm.state.any()
    #                          upd  B  pairs sum_sq dist within tp fp fn cae  tp fp fn
    qm.state[0] = torch.tensor([1., 4., 6., 4.5, 3.0, 3., 5., 3., 1., 6., 0., 0., 2.], dtype=torch.float64)
    qm.state[1] = torch.tensor([3., 12., 0., 0.0, 0.0, 0., 0., 0., 0., 9., 4., 0., 0.], dtype=torch.float64)
    m = qm.read()
    assert set(m) == {"last", "running"}
    last, run = m["last"], m["running"]
    for name, v in zip(TM.COLUMNS, qm.state[0].tolist()):
        assert last[name] == v
    assert last["matched_rmse"] == math.sqrt(4.5 / 18.0) == 0.5
    assert last["mean_distance"] == 0.5 and last["corner_recall"] == 0.5
    assert last["existence_precision"] == 5 / 8 and last["existence_recall"] == 5 / 6 and last["existence_f1"] == 10 / 14
    assert last["count_mae"] == 1.5
    assert math.isnan(last["edge_precision"]) and last["edge_recall"] == 0.0 and last["edge_f1"] == 0.0
    assert run["updates"] == 3 and run["n_samples"] == 12 and run["count_mae"] == 0.75
    for k in ("matched_rmse", "mean_distance", "corner_recall", "existence_precision", "existence_recall", "existence_f1"):
        assert math.isnan(run[k]), k
    assert run["edge_precision"] == run["edge_recall"] == run["edge_f1"] == 1.0
    qm.state[0, 3] = float("nan")
    assert math.isnan(qm.read()["last"]["matched_rmse"])
    qm.reset()
    assert not qm.state[1].any() and qm.state[0, 2] == 6.0          # reset() zeroes the running row only
    fresh = WireframeMeter(torch.device("cpu")).read()               # nothing recorded yet: every ratio is nan
    assert fresh["last"]["updates"] == 0 and math.isnan(fresh["running"]["count_mae"])


def test_update_refuses_cpu_tensors():
    from wf3d.meter import WireframeMeter
    qm = WireframeMeter(torch.device("cpu"))
    v, e, p, tv, te, tl, a, c = (torch.from_numpy(x) for x in _hand_case())
    pred = {"vertices": v, "existence_probabilities": e, "edge_probs": p}
    tgt = {"vertices": tv, "vertex_existence": te, "edge_labels": tl, "vertex_counts": c}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        qm.update(pred, tgt, a)
    assert not qm.state.any()
