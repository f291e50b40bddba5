"""Wireframe decoding, stated once in numpy: the specification wf3d_wireframe_decode (csrc/evalpost.hip) is held to
exactly, and the path wf3d.postprocess.decode_wireframes takes for CPU tensors.  No GPU, no torch.

One forward pass gives V vertex slots, an existence probability per slot and a probability per candidate pair.
`decode_wireframe` turns one sample of it into a wireframe of vertices that exist, are distinct and are connected:

  1. alive     slot i is alive iff i < c = clamp(count, 0, V), its three coordinates are finite, its existence is not
               NaN and (existence_threshold is None or existence[i] > existence_threshold, compared in float32).
               A non-finite coordinate or a NaN existence below c sets NONFINITE in the status.
  2. merging   greedy suppression.  The alive slots are visited by (existence descending, slot ascending), floats
               compared as values (-0.0 ties with 0.0).  A visited slot becomes a representative unless an earlier
               representative lies within the radius, d2 <= r2; then it is merged into the FIRST such representative in
               visiting order.  d2 = (dx dx + dy dy) + dz dz in float64 on the widened float32 coordinates, every
               operation rounded on its own; r2 = float64(merge_radius) ** 2.  None merges nothing, 0.0 coincident
               vertices only.  A merged vertex keeps its representative's coordinates unchanged, so every segment end
               point stays a row of the vertex array.
  3. edges     candidate e = (i, j), i < j < c, e < max_e in the model's lexicographic pair order over the first c
               slots, survives iff both ends are alive, edge_probs[e] > edge_threshold (float32; NaN and equality do not
               pass) and rep(i) != rep(j).  It lands on the unordered pair of representatives; a pair's probability is
               the maximum over the candidates that land on it (0.0 above -0.0).
  4. output    the representatives in ascending slot order (drop_isolated: only those that are an end of an output
               edge); edges (a, b), a < b, in the new indices and lexicographic order; each edge's two end points,
               higher z first (equal z: vertex b first).
"""
import numpy as np

NONFINITE = 1                    # WF3D_DECODE_NONFINITE of include/wf3d.h


def squared_distance(a, b):
    """(dx dx + dy dy) + dz dz in float64 from two float32 points: the association of pt_dist in csrc/evalmetrics.hip."""
    d = np.asarray(a, dtype=np.float32).astype(np.float64) - np.asarray(b, dtype=np.float32).astype(np.float64)
    return float((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def visiting_order(existence, alive):
    """The alive slots by (existence descending, slot ascending); -0.0 and 0.0 tie, as values do."""
    return sorted((i for i in range(len(alive)) if alive[i]), key=lambda i: (-float(existence[i]), i))


def decode_wireframe(vertices, existence, edge_probs, count, *, existence_threshold=0.5, edge_threshold=0.5,
                     merge_radius=None, drop_isolated=False):
    """vertices [V, 3], existence [V], edge_probs [max_e] float32, count an integer ->
    dict(vertices float32 [n, 3], slots int64 [n], edges int64 [k, 2], seg float32 [k, 2, 3], kprob float32 [k],
         status int, rep int64 [V]: every alive slot's representative slot, -1 for a slot that is not alive)."""
    vertices = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    existence = np.asarray(existence, dtype=np.float32).reshape(-1)
    edge_probs = np.asarray(edge_probs, dtype=np.float32).reshape(-1)
    for name, t in (("existence_threshold", existence_threshold), ("edge_threshold", edge_threshold), ("merge_radius", merge_radius)):
        if t is not None and np.isnan(t):
            raise ValueError(f"decode_wireframe: {name} is NaN")
    if edge_threshold is None:
        raise ValueError("decode_wireframe: edge_threshold must be a number")
    V, max_e = vertices.shape[0], edge_probs.shape[0]
    if existence.shape[0] != V:
        raise ValueError(f"decode_wireframe: {V} vertices, {existence.shape[0]} existence values")
    c = min(max(int(count), 0), V)
    # 1. alive slots
    finite = np.isfinite(vertices).all(axis=1) & ~np.isnan(existence)
    status = 0 if finite[:c].all() else NONFINITE
    alive = finite & (np.arange(V) < c)
    if existence_threshold is not None:
        with np.errstate(invalid="ignore"):
            alive &= existence > np.float32(existence_threshold)
    # 2. greedy suppression
    rep = np.full(V, -1, dtype=np.int64)
    reps = []                                                    # in visiting order
    r2 = None if merge_radius is None or merge_radius < 0 else float(np.float64(merge_radius) * np.float64(merge_radius))
    for i in visiting_order(existence, alive):
        rep[i] = i
        if r2 is not None:
            for k in reps:
                if squared_distance(vertices[i], vertices[k]) <= r2:
                    rep[i] = k
                    break
        if rep[i] == i:
            reps.append(i)
    # 3. edges: the maximum probability per unordered pair of representatives
    best = {}
    thr = np.float32(edge_threshold)
    e = 0
    for i in range(c):
        for j in range(i + 1, c):
            if e >= max_e:
                break
            p = edge_probs[e]
            e += 1
            if not (alive[i] and alive[j] and p > thr and rep[i] != rep[j]):
                continue
            key = (min(rep[i], rep[j]), max(rep[i], rep[j]))
            old = best.get(key)
            if old is None or p > old or (p == old and not np.signbit(p)):
                best[key] = p
    # 4. output
    used = {k for key in best for k in key}
    slots = [i for i in sorted(reps) if not drop_isolated or i in used]
    new = {slot: n for n, slot in enumerate(slots)}
    out_v = vertices[slots].reshape(-1, 3)
    edges = np.array(sorted((new[a], new[b]) for a, b in best), dtype=np.int64).reshape(-1, 2)
    kprob = np.array([best[(slots[a], slots[b])] for a, b in edges], dtype=np.float32)
    seg = np.empty((len(edges), 2, 3), dtype=np.float32)
    for k, (a, b) in enumerate(edges):
        a_first = out_v[a, 2] > out_v[b, 2]
        seg[k, 0], seg[k, 1] = (out_v[a], out_v[b]) if a_first else (out_v[b], out_v[a])
    return {"vertices": out_v.copy(), "slots": np.array(slots, dtype=np.int64), "edges": edges, "seg": seg, "kprob": kprob,
            "status": status, "rep": rep}


def decode_batch(vertices, existence, edge_probs, counts, **options):
    """decode_wireframe per sample, in the arrays wf3d_wireframe_decode writes: dict(nverts int32 [B], dverts float32
    [B, V, 3] (zero rows behind the live ones), slots int32 [B, V] (-1 behind them), koff int32 [B + 1], pairs int32
    [K, 2], seg float32 [K, 2, 3], kprob float32 [K], status int32 [B])."""
    vertices = np.asarray(vertices, dtype=np.float32)
    B, V = vertices.shape[:2]
    out = {"nverts": np.zeros(B, np.int32), "dverts": np.zeros((B, V, 3), np.float32), "slots": np.full((B, V), -1, np.int32),
           "koff": np.zeros(B + 1, np.int32), "status": np.zeros(B, np.int32)}
    pairs, seg, kprob = [np.empty((0, 2), np.int32)], [np.empty((0, 2, 3), np.float32)], [np.empty(0, np.float32)]
    for s in range(B):
        w = decode_wireframe(vertices[s], existence[s], edge_probs[s], counts[s], **options)
        n = len(w["slots"])
        out["nverts"][s], out["status"][s] = n, w["status"]
        out["dverts"][s, :n], out["slots"][s, :n] = w["vertices"], w["slots"]
        out["koff"][s + 1] = out["koff"][s] + len(w["edges"])
        pairs.append(w["edges"].astype(np.int32))
        seg.append(w["seg"])
        kprob.append(w["kprob"])
    out.update(pairs=np.concatenate(pairs), seg=np.concatenate(seg), kprob=np.concatenate(kprob))
    return out
