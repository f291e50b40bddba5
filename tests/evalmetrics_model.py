"""A numpy statement of the device evaluation metrics (csrc/evalmetrics.hip; wf3d_lsa_rect_batch and wf3d_eval_metrics): what
APCalculator._with_edges / _corners_only derive from a sample's Hausdorff matrix, written with the device's own choices.

  lsa_rect(C)       the rectangular assignment: lsa_model._augmenting_paths on the clamped fp64 costs, the shorter side
                    as the solver's rows (transpose iff n > m, as scipy does) -> (entries [min(n, m)], status)
  sample(...)       counters, distances and status of one sample
  accumulate(...)   the same `+=` into an APCalculator as compute_metrics, wed from the label-only constants

The choices: corner sets by VALUE equality on the three floats (-0.0 == 0.0), free corners in lexicographic (x, y, z)
order, distances sqrt((dx dx + dy dy) + dz dz) in fp64 from the fp32 coordinates, every sum taken sequentially: the
matched free corners in row order, then + e_term, e_term over pr_u in lexicographic order.

Also the inputs the CPU and the GPU test share: cases()."""
import numpy as np

import lsa_model

FLT_MAX = lsa_model.FLT_MAX
NONFINITE, NO_MATCH, STEPS, RANGE, ENDPOINT = 1, 2, 4, 8, 16


def clamp(C):
    """NaN, +inf and anything above FLT_MAX -> FLT_MAX, -inf and anything below -FLT_MAX -> -FLT_MAX (float64)."""
    C = np.asarray(C, dtype=np.float64)
    out = np.where(C < FLT_MAX, C, FLT_MAX)                     # NaN compares false
    return np.where(out > -FLT_MAX, out, -FLT_MAX)


def lsa_rect(C):
    """(entries, status): n <= m: entry i = the column of row i; n > m: entry j = the row of column j."""
    C = np.asarray(C, dtype=np.float64)
    n, m = C.shape
    if n * m == 0:
        return np.empty(0, dtype=np.int64), 0
    A = clamp(C)
    status = 0 if np.array_equal(A, C) else NONFINITE
    col4row, _, _ = lsa_model._augmenting_paths(np.ascontiguousarray(A.T if n > m else A))
    return col4row, status


def pairs(C):
    """(rows, cols) of the assignment, by increasing row: what scipy.optimize.linear_sum_assignment returns."""
    n, m = C.shape
    e, status = lsa_rect(C)
    if n <= m:
        return np.arange(len(e)), e, status
    order = np.argsort(e)
    return e[order], np.arange(len(e))[order], status


def _eq(a, b):
    return bool(a[0] == b[0] and a[1] == b[1] and a[2] == b[2])


def _distinct(rows):
    out = []
    for r in rows:
        if not any(_eq(r, o) for o in out):
            out.append(r)
    return out


def _lex(rows):
    return sorted(rows, key=lambda r: (float(r[0]), float(r[1]), float(r[2])))         # tuples compare by value: -0.0 == 0.0


def _dist(a, b):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def _dm(P, G):
    return np.array([[_dist(p, g) for g in G] for p in P], dtype=np.float64).reshape(len(P), len(G))


def sample(pred_v, seg, gt_v, gt_seg, hd, thresh):
    """pred_v [V, 3], seg [n, 2, 3], gt_v [Lv, 3], gt_seg [m, 2, 3] float32; hd [n, m] float64 (unused when n = 0).
    -> dict(tp_corners, tp_fp_corners, tp_fn_corners, tp_edges, tp_fp_edges, tp_fn_edges, distances, status)"""
    n, m = len(seg), len(gt_seg)
    status = 0
    if not (np.isfinite(pred_v).all() and np.isfinite(gt_v).all()):
        status |= NONFINITE
    if n == 0:
        P, G, pr_u, e_term, tp_edges = list(pred_v), list(gt_v), [], 0.0, 0
    else:
        pi, li, st = pairs(np.asarray(hd, dtype=np.float64).reshape(n, m))
        status |= st
        ok = [(p, l) for p, l in zip(pi, li) if hd[p, l] <= thresh]
        tp_edges = len(ok)
        pr_u = _lex(_distinct([seg[p][e] for p, _ in ok for e in (0, 1)]))
        gt_u = _lex(_distinct([gt_seg[l][e] for _, l in ok for e in (0, 1)]))
        P = _lex([r for r in _distinct(list(pred_v)) if not any(_eq(r, u) for u in pr_u)])
        G = _lex([r for r in _distinct(list(gt_v)) if not any(_eq(r, u) for u in gt_u)])
        e_term = 0.0
        for p in pr_u:
            e_term += min(_dist(p, g) for g in gt_u)
        if not pr_u:
            status |= NO_MATCH
    dm = _dm(P, G)
    fi, fj, st = pairs(dm)
    status |= st
    total, nok = 0.0, 0
    for i, j in zip(fi, fj):
        if dm[i, j] <= thresh:
            total += dm[i, j]
            nok += 1
    return dict(tp_corners=len(pr_u) + nok, tp_fp_corners=len(pred_v), tp_fn_corners=len(gt_v), tp_edges=tp_edges,
                tp_fp_edges=n, tp_fn_edges=m, distances=total + e_term, status=status)


def accumulate(calc, pred_v, seg, gt_v, gt_e, gt_seg, hd, consts):
    """The `+=` of compute_metrics for one sample; consts = (wed_e, s, total) of the label (EvalLabels.consts[s]).
    A sample with kept edges of which none matches raises ValueError, as the host path does on its empty reduction."""
    r = sample(pred_v, seg, gt_v, gt_seg, hd, calc.distance_thresh)
    if r["status"] & NO_MATCH:
        raise ValueError("no kept edge matches a label edge")
    assert r["status"] == 0, r["status"]
    calc.batch_size = 1
    for k in ("tp_corners", "tp_fp_corners", "tp_fn_corners", "tp_edges", "tp_fp_edges"):
        calc.ap_dict[k] += r[k]
    calc.ap_dict["tp_fn_edges"] += len(gt_e)
    calc.ap_dict["distance"] += r["distances"]
    calc.ap_dict["wed"] += (consts[0] + (r["distances"] + consts[1])) / consts[2] if len(seg) else 1
    return r


# ---- shared inputs ----------------------------------------------------------------------------------------------------
def z_first(vertices, edges):
    """[E, 2, 3] end points, higher z first (equal z: the second vertex first), as evaluate.py:88-89 orders them."""
    if len(edges) == 0:
        return np.empty((0, 2, 3), dtype=vertices.dtype)
    ev = np.stack((vertices[edges[:, 0]], vertices[edges[:, 1]]), axis=1)
    return ev[np.arange(len(ev))[:, None], np.flip(np.argsort(ev[:, :, -1]), axis=1)]


def cases(g):
    """[(name, vertices [12, 3] float32, probs [66] float32, raises)]: the three fixture samples of eval.npz, then seeded
    synthetic predictions at V = 12 around the fixture's 8-vertex / 8-edge label: the label vertices plus noise in the
    first 8 rows, the label edges kept, a few random other pairs kept."""
    gt_v, gt_e, prs, V = g["gt_v"], g["gt_e"], g["pairs"], int(g["V"])
    index = {(int(i), int(j)): e for e, (i, j) in enumerate(prs)}
    label_e = np.array([index[(min(a, b), max(a, b))] for a, b in gt_e])
    out = [(f"fixture{c}", g[f"c{c}.vertices"].copy(), g[f"c{c}.probs"].copy(), False) for c in range(3)]

    def base(seed, noise, extra=4):
        gen = np.random.RandomState(100 + seed)
        v = gen.uniform(-7, 7, (V, 3)).astype(np.float32)
        v[:8] = gt_v + gen.normal(0, noise, (8, 3)).astype(np.float32)
        p = gen.uniform(0.0, 0.45, len(prs)).astype(np.float32)
        p[label_e] = 0.9
        p[gen.choice(len(prs), extra, replace=False)] = 0.8
        return v, p

    for seed, noise in enumerate((0.01, 0.05, 0.2, 0.6, 0.02, 0.3)):
        out.append((f"noise{noise}_{seed}", *base(seed, noise), False))
    v, p = base(10, 0.05)                                        # coincident predicted vertices, both with kept edges
    v[5] = v[3]
    v[9] = v[8]                                                  # ... and two coincident free ones
    out.append(("coincident", v, p, False))
    v, p = base(11, 0.05)                                        # predictions equal to label vertices
    v[2], v[6], v[10] = gt_v[2], gt_v[6], gt_v[0]
    out.append(("equal_to_label", v, p, False))
    v, p = base(12, 0.05, extra=0)                               # -0.0 against 0.0: one free corner, not two
    v[8] = (0.0, 3.0, -0.0)
    v[9] = (-0.0, 3.0, 0.0)
    v[10] = (-0.0, -2.0, 1.0)
    v[11] = (0.0, -2.5, 1.0)
    p[[index[(8, 9)], index[(10, 11)]]] = 0.0
    out.append(("signed_zero", v, p, False))
    v, p = base(13, 0.05)                                        # corners only, with duplicate rows (kept as given)
    v[1], v[7], v[11] = v[0], v[0], v[10]
    out.append(("corners_only_duplicates", v, np.zeros_like(p), False))
    v, p = base(14, 0.05)                                        # kept edges that all miss: both paths raise
    out.append(("all_miss", (v + np.float32(100.0)).astype(np.float32), p, True))
    v, p = base(15, 0.4, extra=20)                               # more kept edges than label edges: the transposed solve
    out.append(("many_kept", v, p, False))
    v, p = base(16, 0.05, extra=0)                               # fewer kept edges than label edges
    p[label_e[:5]] = 0.1
    out.append(("few_kept", v, p, False))
    v, p = base(17, 0.05, extra=0)                               # one distinct free predicted corner, several free label ones
    p[label_e[:5]] = 0.1
    on_kept = set(int(i) for i in prs[p > 0.5].reshape(-1))
    v[[i for i in range(V) if i not in on_kept]] = v[11]
    out.append(("free_coincide", v, p, False))
    return out
