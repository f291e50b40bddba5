"""The training metrics of wf3d.meter.WireframeMeter (csrc/metrics.hip, wf3d_train_metrics) stated in numpy float64 with
plain loops: one row of 13 counters per batch, in the column order of the state tensor.

    c_b = clamp(counts[b], 0, min(V, Vt))
    matched pair: slot p of sample b with 0 <= col4row[b, p] < c_b; d2 = ((dx dx + dy dy) + dz dz) in float64 from the
        float32 coordinates; sum_sq += d2, sum_dist += sqrt(d2), n_within += (d2 <= float64(float32(thresh))^2)
    existence over all B V slots: predicted exist > 0.5, label texist > 0.5; count_abs_err += |#(exist_b > 0.5) - c_b|
    edges over the first w = min(Ep, Et[, edge_width]) columns: predicted edge > float32(edge_threshold), label > 0.5;
        columns at or past w are not read
Comparisons with NaN are false; the two sums carry a NaN."""
import numpy as np

COLUMNS = ("updates", "n_samples", "n_pairs", "sum_sq", "sum_dist", "n_within", "ex_tp", "ex_fp", "ex_fn",
           "count_abs_err", "ed_tp", "ed_fp", "ed_fn")
INT_COLUMNS = [i for i, c in enumerate(COLUMNS) if c not in ("sum_sq", "sum_dist")]
SUM_COLUMNS = [COLUMNS.index("sum_sq"), COLUMNS.index("sum_dist")]


def batch_row(verts, exist, edge, tverts, texist, tlabel, col4row, counts, edge_width=None, edge_threshold=0.5,
              distance_thresh=0.05):
    """float64 [13]: the counters of one batch.  Arrays are what the kernel reads: float32 values, int32 col4row,
    int64 counts."""
    verts, tverts = np.asarray(verts, np.float32), np.asarray(tverts, np.float32)
    exist, texist = np.asarray(exist, np.float32), np.asarray(texist, np.float32)
    edge, tlabel = np.asarray(edge, np.float32), np.asarray(tlabel, np.float32)
    B, V, Vt, Ep, Et = verts.shape[0], verts.shape[1], tverts.shape[1], edge.shape[1], tlabel.shape[1]
    thr = np.float32(edge_threshold)
    t2 = np.float64(np.float32(distance_thresh)) ** 2
    half = np.float32(0.5)
    r = dict.fromkeys(COLUMNS, 0.0)
    r["updates"], r["n_samples"] = 1.0, float(B)
    w = min(Ep, Et) if edge_width is None else max(0, min(int(edge_width), Ep, Et))
    with np.errstate(invalid="ignore"):
        for b in range(B):
            cb = max(0, min(int(counts[b]), V, Vt))
            predicted = 0
            for p in range(V):
                t = int(col4row[b, p])
                if 0 <= t < cb:
                    d = verts[b, p].astype(np.float64) - tverts[b, t].astype(np.float64)
                    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                    r["n_pairs"] += 1
                    r["sum_sq"] += d2
                    r["sum_dist"] += np.sqrt(d2)
                    r["n_within"] += bool(d2 <= t2)
                pr, lb = bool(exist[b, p] > half), bool(texist[b, p] > half)
                predicted += pr
                r["ex_tp"] += pr and lb
                r["ex_fp"] += pr and not lb
                r["ex_fn"] += (not pr) and lb
            r["count_abs_err"] += abs(predicted - cb)
            pr, lb = edge[b, :w] > thr, tlabel[b, :w] > half               # element-wise; the loop over columns in numpy
            r["ed_tp"] += int(np.count_nonzero(pr & lb))
            r["ed_fp"] += int(np.count_nonzero(pr & ~lb))
            r["ed_fn"] += int(np.count_nonzero(~pr & lb))
    return np.array([r[c] for c in COLUMNS], dtype=np.float64)


def state_after(rows):
    """float64 [2, 13]: the state after updates with these batch rows since the last reset."""
    s = np.zeros((2, len(COLUMNS)))
    for row in rows:
        s[0] = row
        s[1] = s[1] + row
    return s
