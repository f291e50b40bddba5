"""Drop-in `eval.ap_calculator` (reference eval/ap_calculator.py:8-307) — row f-4, what runs behind the hot path at
evaluation time: Hausdorff distances between predicted and labelled edges, optimal edge / corner matching, corner and
edge precision / recall / F1, average corner offset, wireframe edit distance.

Same public names, arguments and accumulated `ap_dict` as the reference, including its quirks (the edit distance is
computed from the LABEL edges, :262-266; a sample with predicted edges of which none matches raises on an empty
reduction, :251).  Rewritten as small vectorised helpers; the one heavy piece — the [N, M] line-to-line Hausdorff
matrix, (20 N) x (20 M) point distances per sample — runs on the device when `device=` is given (csrc/evalpost.hip),
otherwise in numpy.  The reference's per-sample debug prints are not reproduced."""
import numpy as np
from scipy.optimize import linear_sum_assignment
from scipy.spatial.distance import cdist

_DEVICE = None


def set_device(device):
    """Route hausdorff_distance_line through the HIP kernel on `device` (None: numpy)."""
    global _DEVICE
    _DEVICE = device


def _line_weights(sample_points):
    w = np.arange(sample_points, dtype=np.float64) * (1.0 / (sample_points - 1)) if sample_points > 1 else np.zeros(1)
    if sample_points > 1:
        w[-1] = 1.0                                  # np.linspace pins the end point
    return w


def hausdorff_distance_line(p_line, t_line, sample_points=20):
    """[N, M] symmetric Hausdorff distance between N query and M target segments ([*, 2, 3] end points), each sampled
    at `sample_points` equidistant points including both ends (reference :8-36)."""
    N, M = p_line.shape[0], t_line.shape[0]
    if N == 0:
        return np.array([])
    if _DEVICE is not None and M > 0:
        from wf3d import postprocess
        return postprocess.hausdorff_lines(p_line, t_line, sample_points, _DEVICE)
    w = _line_weights(sample_points).reshape(1, sample_points, 1)
    # segment directions in the arrays' COMMON dtype (float32 predictions and labels: a float32 subtraction, as the
    # reference's concatenate-then-subtract does), sample points in float64
    both = np.concatenate((p_line, t_line), axis=0)
    start = both[:, 0, :][:, None, :]
    pts = start + w * (both[:, 1, :][:, None, :] - start)
    d = cdist(pts[:N].reshape(-1, 3), pts[N:].reshape(-1, 3), "euclidean").reshape(N, sample_points, M, sample_points)
    d = d.transpose(0, 2, 1, 3)                                   # [N, M, query point, target point]
    h_pt = d.min(-1).max(-1)                                      # every query point to its nearest target point
    h_tp = d.min(-2).max(-1)                                      # every target point to its nearest query point
    return np.maximum(h_pt, h_tp)


def _row_index(table, row):
    hit = np.where((table == row).all(axis=1))[0]
    return hit[0] if len(hit) else -1


def _length(vertices, edge):
    return np.linalg.norm(vertices[edge[0]] - vertices[edge[1]])


def graph_edit_distance(pd_vertices, pd_edges, gt_vertices, gt_edges, wed_v):
    """Weighted wireframe edit distance (reference :39-88): predicted corners are snapped to their nearest label corner
    (cost: the snap distances, added to `wed_v`), predicted edges that do not exist in the label graph cost their
    length, label edges left unexplained cost theirs; normalised by the total label edge length."""
    wed_e, wed_v, total = edit_distance_terms(pd_vertices, pd_edges, gt_vertices, gt_edges, wed_v)
    return (wed_e + wed_v) / total


def edit_distance_terms(pd_vertices, pd_edges, gt_vertices, gt_edges, wed_v):
    """The three terms of graph_edit_distance, which returns (wed_e + wed_v) / total: the edge cost, `wed_v` plus the snap
    distances, and the total label edge length.  compute_metrics passes the LABEL's own points and edges as the
    "prediction", so wed_e, the snap distances and total depend on the labels alone (wf3d.postprocess.EvalLabels)."""
    wed_e = 0
    remaining = gt_edges.copy()
    if len(pd_vertices) > 0:
        dist = cdist(pd_vertices, gt_vertices)
        wed_v += sum(np.min(dist, axis=1))
        for i, j in enumerate(np.argmin(dist, axis=1)):
            pd_vertices[i] = gt_vertices[j]
        uniq = np.unique(pd_vertices, axis=0)
        relabelled = pd_edges.copy()
        for new_id, point in enumerate(uniq):
            for old_id in np.where((pd_vertices == point).all(axis=1))[0]:
                relabelled[pd_edges == old_id] = new_id
        relabelled = np.unique(relabelled, axis=0)
        for edge in relabelled:
            a = np.where((gt_vertices == uniq[edge[0]]).all(axis=1))[0]
            b = np.where((gt_vertices == uniq[edge[1]]).all(axis=1))[0]
            key = np.array(sorted([a[0], b[0]]))
            if len(np.where((gt_edges == key).all(axis=1))[0]):
                remaining = remaining[np.any(remaining != key, axis=1)]
            else:
                wed_e += np.linalg.norm(uniq[edge[0]] - uniq[edge[1]])
    else:
        wed_v = 0
    for edge in remaining:
        wed_e += _length(gt_vertices, edge)
    total = 0
    for edge in gt_edges:
        total += _length(gt_vertices, edge)
    return wed_e, wed_v, total


def computer_edges(edges, vertices):
    """Index pairs (sorted, -1 where a point is not a row of `vertices`) of [E, 2, 3] edge end points (reference :91-106)."""
    return np.sort(np.array([[_row_index(vertices, point) for point in edge] for edge in edges]), axis=-1)


def remove_corners(corner_a, corner_b):
    """Rows of corner_a that are not rows of corner_b — sorted and unique, like np.setdiff1d on row views (reference :109-113)."""
    row = [("", corner_a.dtype)] * corner_a.shape[1]
    return np.setdiff1d(corner_a.view(row), corner_b.view(row)).view(corner_a.dtype).reshape(-1, corner_a.shape[1])


_COUNTERS = ("tp_corners", "tp_fp_corners", "tp_fn_corners", "distance", "tp_edges", "wed", "tp_fp_edges", "tp_fn_edges")


class APCalculator(object):
    def __init__(self, distance_thresh=0.1, confidence_thresh=0.7):
        # distance_thresh: matching radius (1 for un-normalised clouds, evaluate.py:60); confidence_thresh: unused, as in the reference
        self.distance_thresh = distance_thresh
        self.confidence_thresh = confidence_thresh
        self.batch_size = 0
        self.ap_dict = {"tp_corners": 0, "tp_fp_corners": 0, "tp_fn_corners": 0, "distance": 0, "tp_edges": 0, "wed": 0,
                        "tp_fp_edges": 0, "tp_fn_edges": 0, "average_corner_offset": 0, "corners_precision": 0,
                        "corners_recall": 0, "corner_f1": 0, "edges_precision": 0, "edges_recall": 0, "edges_f1": 0}

    # -- one sample ----------------------------------------------------------------------------------------------
    def _with_edges(self, corners, edges, edge_pts, gt_corners_all, gt_edges, gt_edge_pts, hd=None):
        thr = self.distance_thresh
        if hd is None:
            hd = hausdorff_distance_line(edge_pts, gt_edge_pts)
        pi, li = linear_sum_assignment(hd)
        ok = hd[pi, li] <= thr
        pr_c, gt_c = edge_pts[pi[ok]], gt_edge_pts[li[ok]]
        pr_u, gt_u = np.unique(pr_c.reshape(-1, 3), axis=0), np.unique(gt_c.reshape(-1, 3), axis=0)
        # corners not used by a matched edge get their own matching
        free_pr, free_gt = remove_corners(corners, pr_u), remove_corners(gt_corners_all, gt_u)
        dm = cdist(free_pr, free_gt)
        fi, fj = linear_sum_assignment(dm)
        fok = dm[fi, fj] <= thr
        distances = np.sum(dm[fi[fok], fj[fok]])
        counts = dict(tp_corners=len(pr_u) + sum(fok), tp_fp_corners=len(corners), tp_fn_corners=len(gt_corners_all),
                      tp_edges=sum(ok), tp_fp_edges=len(edges), tp_fn_edges=len(gt_edges))
        distances += np.sum(np.min(cdist(pr_u, gt_u), axis=1))        # raises on an empty match set, as the reference does
        for k, q in enumerate(pi[ok]):
            edge_pts[q] = gt_edge_pts[li[ok][k]]
        label_pts = np.unique(gt_edge_pts.reshape(-1, 3), axis=0)
        wed = graph_edit_distance(label_pts, computer_edges(gt_edge_pts, label_pts).copy(), gt_corners_all.copy(),
                                  gt_edges.copy(), distances)
        return counts, distances, wed

    def _corners_only(self, corners, gt_corners_all, gt_edges):
        dm = cdist(corners, gt_corners_all)
        pi, li = linear_sum_assignment(dm)
        ok = dm[pi, li] <= self.distance_thresh
        counts = dict(tp_corners=len(pi[ok]), tp_fp_corners=len(corners), tp_fn_corners=len(gt_corners_all),
                      tp_edges=0, tp_fp_edges=0, tp_fn_edges=len(gt_edges))
        return counts, np.sum(dm[pi[ok], li[ok]]), 1

    def compute_metrics(self, batch):
        """batch: predicted_vertices [B, V, 3], predicted_edges [B, E, 2], pred_edges_vertices [B, E, 2, 3] and the
        labels wf_vertices, wf_edges, wf_edges_vertices (reference :121-272); accumulates into self.ap_dict.
        Optional batch["hausdorff"]: per sample an [E, M] float64 Hausdorff matrix of its predicted against its label
        edges computed elsewhere (wf3d.postprocess.evaluate_batch(compact=True): one launch per batch), or None to have
        hausdorff_distance_line compute it as without the key."""
        self.batch_size = len(batch["predicted_vertices"])
        given = batch.get("hausdorff")
        for b in range(self.batch_size):
            corners, edges = batch["predicted_vertices"][b], batch["predicted_edges"][b]
            args = (batch["wf_vertices"][b], batch["wf_edges"][b])
            if len(edges) != 0:
                counts, dist, wed = self._with_edges(corners, edges, batch["pred_edges_vertices"][b], args[0], args[1],
                                                     batch["wf_edges_vertices"][b], None if given is None else given[b])
            else:       # corners without any edge: an empty model
                counts, dist, wed = self._corners_only(corners, *args)
            for k, v in counts.items():
                self.ap_dict[k] += v
            self.ap_dict["distance"] += dist
            self.ap_dict["wed"] += wed

    def output_accuracy(self):
        d = self.ap_dict

        def ratio(a, b):
            return a / b if b > 0 else 0.0

        def f1(p, r):
            return 2 * p * r / (p + r) if p + r > 0 else 0.0

        d["average_corner_offset"] = ratio(d["distance"], d["tp_corners"])
        d["average_wed"] = ratio(d["wed"], self.batch_size)
        d["corners_precision"], d["corners_recall"] = ratio(d["tp_corners"], d["tp_fp_corners"]), ratio(d["tp_corners"], d["tp_fn_corners"])
        d["corners_f1"] = f1(d["corners_precision"], d["corners_recall"])
        d["edges_precision"], d["edges_recall"] = ratio(d["tp_edges"], d["tp_fp_edges"]), ratio(d["tp_edges"], d["tp_fn_edges"])
        d["edges_f1"] = f1(d["edges_precision"], d["edges_recall"])
        print("Wireframe Edit distance", d["average_wed"])
        print("Average Corner offset", d["average_corner_offset"])
        print("Corners Precision: ", d["corners_precision"])
        print("Corners Recall: ", d["corners_recall"])
        print("Corners F1：", d["corners_f1"])
        print("Edges Precision: ", d["edges_precision"])
        print("Edges Recall: ", d["edges_recall"])
        print("Edges F1: ", d["edges_f1"])

    def reset(self):
        self.ap_dict = {"tp_corners": 0, "tp_fp_corners": 0, "tp_fn_corners": 0, "distance": 0, "tp_edges": 0, "wed": 0,
                        "tp_fp_edges": 0, "tp_fn_edges": 0, "average_corner_offset": 0, "corners_precision": 0,
                        "corners_recall": 0, "corners_f1": 0, "edges_precision": 0, "edges_recall": 0, "edges_f1": 0}
