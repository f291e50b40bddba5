"""A numpy fp64 model of the streaming 4-way pool (include/wf3d.h, "STREAMING 4-way pool"): init, fold blocks, finish.
The reference of tests/test_infer_stream_gpu.py, checked against the direct per-cloud pools in
tests/test_infer_stream.py.

The state is what the kernels keep per cloud and channel — masked sum, unmasked sum, masked max, unmasked max — and the
valid-row count per cloud.  offsets: B + 1 row offsets; rows at or past offsets[B] belong to no cloud."""
import numpy as np


def init(B, C):
    return {"msum": np.zeros((B, C)), "usum": np.zeros((B, C)), "mmax": np.full((B, C), -np.inf),
            "umax": np.full((B, C), -np.inf), "cnt": np.zeros(B)}


def fold(state, offsets, pf, valid, r0):
    """Folds the block pf [rows, C], valid [rows] = rows r0 .. r0 + rows - 1 of the flat row space into the state."""
    pf = np.asarray(pf, dtype=np.float64)
    ok = np.asarray(valid) != 0
    r1 = r0 + pf.shape[0]
    for b in range(len(offsets) - 1):
        lo, hi = max(int(offsets[b]), r0), min(int(offsets[b + 1]), r1)
        if hi <= lo:
            continue
        v, m = pf[lo - r0:hi - r0], ok[lo - r0:hi - r0]
        state["usum"][b] += v.sum(0)
        state["umax"][b] = np.maximum(state["umax"][b], v.max(0))
        if m.any():
            state["msum"][b] += v[m].sum(0)
            state["mmax"][b] = np.maximum(state["mmax"][b], v[m].max(0))
            state["cnt"][b] += m.sum()


def finish(state, offsets):
    """masked = [max | mean], unmasked = [mean | max], cnt = max(valid rows, 1), nvalid = valid rows."""
    n = np.diff(np.asarray(offsets, dtype=np.int64)).astype(np.float64)
    cnt = state["cnt"]
    cl = np.maximum(cnt, 1.0)
    mmax = np.where((cnt > 0)[:, None], state["mmax"], 0.0)
    umax = np.where((n > 0)[:, None], state["umax"], 0.0)
    umean = np.where((n > 0)[:, None], state["usum"] / np.maximum(n, 1.0)[:, None], 0.0)
    return {"masked": np.concatenate([mmax, state["msum"] / cl[:, None]], 1),
            "unmasked": np.concatenate([umean, umax], 1), "cnt": cl, "nvalid": cnt.copy()}


def stream(offsets, pf, valid, cuts):
    """The pools of pf [R, C] folded block by block; cuts: ascending row indices 0 = cuts[0] < ... < cuts[-1] = R."""
    state = init(len(offsets) - 1, pf.shape[1])
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        fold(state, offsets, pf[r0:r1], valid[r0:r1], r0)
    return finish(state, offsets)


def direct(offsets, pf, valid):
    """The same pools cloud by cloud, as the reference forms them (PointNetEncoder.py:103-115, VertexPredictor.py:86-88);
    a cloud of no rows pools to zeros."""
    pf = np.asarray(pf, dtype=np.float64)
    B, C = len(offsets) - 1, pf.shape[1]
    out = {"masked": np.zeros((B, 2 * C)), "unmasked": np.zeros((B, 2 * C)), "cnt": np.ones(B), "nvalid": np.zeros(B)}
    for b in range(B):
        v = pf[offsets[b]:offsets[b + 1]]
        m = np.asarray(valid[offsets[b]:offsets[b + 1]]) != 0
        if not len(v):
            continue
        out["unmasked"][b] = np.concatenate([v.mean(0), v.max(0)])
        out["nvalid"][b] = m.sum()
        out["cnt"][b] = max(m.sum(), 1)
        if m.any():
            out["masked"][b] = np.concatenate([v[m].max(0), v[m].sum(0) / m.sum()])
    return out
