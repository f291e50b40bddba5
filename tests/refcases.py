"""Cases of the checks against the reference (tests/test_*_vs_reference.py, tests/test_dropin_surface.py) and the inputs
they regenerate, shared with the fixture generator tests/golden/make_golden_refcheck.py."""
import numpy as np
import torch

from refsummary import digest

MODEL_OUTPUTS = ("vertices", "existence_probabilities", "edge_probs", "global_features")
MODEL_COTANGENTS = ("vertices", "existence_probabilities", "edge_probs")

ENCODER_SIZES = (([256, 768], 768), ([264, 520], 264), ([], 40), ([64, 128, 256, 128, 64], 32), ([512], 96))
EDGE_SIZES = ((3, 208, 4, 6), (6, 96, 3, 8), (3, 1024, 16, 5), (2, 128, 8, 9), (3, 384, 6, 4))      # vertex_dim, hidden, heads, count
VERTEX_SIZES = ((384, 10), (200, 7), (64, 40), (1024, 12))                                           # global_feature_dim, max_vertices

# B, V, counts (None: random), predicted edges, target edges
LOSS_SHAPES = ((1, 1, [1], 1, 1), (1, 2, [0], 1, 1), (2, 3, [0, 0], 3, 3), (5, 4, [4, 1, 0, 2, 3], 6, 4), (64, 3, None, 3, 3),
               (3, 130, [130, 1, 77], 400, 8385), (2, 256, [256, 200], 32640, 32640), (7, 17, None, 136, 50))
LOSS_KEYS = ("total_loss", "vertex_loss", "existence_loss", "edge_loss")


def loss_inputs(B, V, counts, ep, et):
    """(predictions, targets) of one loss case, from a generator seeded by the shape."""
    g = torch.Generator().manual_seed(B * 1000 + V)
    if counts is None:
        counts = torch.randint(0, V + 1, (B,), generator=g).tolist()
    cnt = torch.tensor(counts, dtype=torch.long)
    pv, tv = torch.randn(B, V, 3, generator=g), torch.randn(B, V, 3, generator=g)
    pe = torch.sigmoid(2.0 * torch.randn(B, V, generator=g))
    pp = torch.sigmoid(2.0 * torch.randn(B, ep, generator=g))
    tl = (torch.rand(B, et, generator=g) > 0.7).float()
    te = (torch.arange(V)[None, :] < cnt[:, None]).float()
    return ({"vertices": pv, "existence_probabilities": pe, "edge_probs": pp},
            {"vertices": tv, "vertex_existence": te, "edge_labels": tl, "vertex_counts": cnt})


EVAL_THRESHOLDS = (0.1, 1.0)
# predicted vertices, predicted edges, target vertices, target edges, noise
EVAL_CASES = ((6, 5, 6, 5, 0.01), (6, 0, 6, 5, 0.01), (9, 12, 5, 4, 0.3), (3, 3, 8, 10, 0.05), (12, 30, 12, 20, 0.02),
              (2, 1, 2, 1, 0.0), (7, 7, 7, 7, 2.0), (5, 10, 5, 1, 0.01))
EVAL_KEYS = ("tp_corners", "tp_fp_corners", "tp_fn_corners", "distance", "tp_edges", "wed", "tp_fp_edges", "tp_fn_edges")
EVAL_ACCURACY_KEYS = ("average_corner_offset", "average_wed", "corners_precision", "corners_recall", "corners_f1",
                      "edges_precision", "edges_recall", "edges_f1")


def _z_first(v, e):
    if len(e) == 0:
        return np.empty((0, 2, 3), dtype=np.float32)
    ev = np.stack((v[e[:, 0]], v[e[:, 1]]), axis=1)
    return ev[np.arange(len(ev))[:, None], np.flip(np.argsort(ev[:, :, -1]), axis=1)].astype(np.float32)


def eval_sample(rng, nv_p, ne_p, nv_g, ne_g, noise):
    """One single-sample batch for APCalculator.compute_metrics: a random wireframe and a noisy prediction of it."""
    gv = rng.normal(0, 2, (nv_g, 3)).astype(np.float32)
    pairs = np.array([(i, j) for i in range(nv_g) for j in range(i + 1, nv_g)], dtype=np.int64).reshape(-1, 2)
    ge = pairs[rng.permutation(len(pairs))[:ne_g]] if len(pairs) else pairs
    pv = (np.resize(gv, (nv_p, 3)) + rng.normal(0, noise, (nv_p, 3))).astype(np.float32)
    pp = np.array([(i, j) for i in range(nv_p) for j in range(i + 1, nv_p)], dtype=np.int64).reshape(-1, 2)
    pe = pp[rng.permutation(len(pp))[:ne_p]] if len(pp) else pp
    return {"predicted_vertices": [pv], "predicted_edges": [pe], "pred_edges_vertices": [_z_first(pv, pe)],
            "wf_vertices": [gv], "wf_edges": [ge], "wf_edges_vertices": [_z_first(gv, ge)]}


def eval_batch_digest(batch):
    return ";".join(digest(batch[k][0]) for k in sorted(batch))
