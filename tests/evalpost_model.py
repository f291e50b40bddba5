"""A numpy model of the kept-edge compaction (wf3d_edge_compact / wf3d.postprocess.wireframes_compact), written from the
semantics of the reference's evaluate.py:79-91, not from the kernel:

    :79     mask  = edge_probs[s] > threshold             (a NaN or a value equal to the threshold is not kept)
    :80-82  edges = edge_indices[s][mask]                 (the lexicographic i < j pairs of the sample's c_s vertices)
    :86-89  end points gathered from the predicted vertices, each edge's pair flipped from an ascending argsort over z

for the c_s (c_s - 1) / 2 candidates of every sample that fit the probability row, concatenated in sample order."""
import numpy as np


def compact(counts, probs, vertices, threshold=0.5):
    """counts [B] ints, probs [B, max_e] float32, vertices [B, V, 3] float32 ->
    koff int32 [B + 1], pairs int32 [K, 2], seg float32 [K, 2, 3], kprob float32 [K]."""
    probs = np.asarray(probs, dtype=np.float32)
    vertices = np.asarray(vertices, dtype=np.float32)
    B, max_e = probs.shape
    thr = np.float32(threshold)
    koff, pairs, seg, kprob = [0], [], [], []
    for s in range(B):
        c = int(counts[s])
        iu = np.triu_indices(c, 1) if c >= 2 else (np.empty(0, np.int64), np.empty(0, np.int64))
        cand = np.stack(iu, axis=1)[:max_e]                              # row-major upper triangle = lexicographic order
        with np.errstate(invalid="ignore"):
            mask = probs[s, :len(cand)] > thr
        e = cand[mask]
        ev = np.stack((vertices[s][e[:, 0]], vertices[s][e[:, 1]]), axis=1).reshape(-1, 2, 3)
        if len(e):
            ev = ev[np.arange(len(e))[:, None], np.flip(np.argsort(ev[:, :, -1]), axis=1)]
        pairs.append(e)
        seg.append(ev)
        kprob.append(probs[s, :len(cand)][mask])
        koff.append(koff[-1] + len(e))
    return (np.array(koff, dtype=np.int32), np.concatenate(pairs).astype(np.int32).reshape(-1, 2),
            np.concatenate(seg).astype(np.float32).reshape(-1, 2, 3), np.concatenate(kprob).astype(np.float32))
