"""The resident data set kernels of csrc/cloud.hip restated in plain numpy, in np.longdouble where the kernels compute in
float64: the reference of tests/test_cloud_kernels_gpu.py.  Reads nothing from the library; tests/test_cloud_model.py holds
it to Building3DReconstructionDataset and wf3d.targets.train_targets on the fixture data.

  normalize_model   wf3d_cloud_normalize: colour / 256, centroid and max-norm of xyz per cloud, (v - c) / md
  gather_model      wf3d_cloud_sample (choice [B, P]) and wf3d_cloud_pack (out_first, capacity): rows of a float64 table,
                    flips and z-rotation in longdouble, ONE rounding to float32
  targets_model     wf3d_wireframe_targets: train_targets(..., full_width=True) from resident wireframes

A parameter block that breaks include/wf3d.h's rules is answered as the header says: zeros where the cloud index or the
position inside the cloud falls outside the resident clouds (a negative position is outside), counts of 0 for an unknown
cloud, and a wireframe of c_s > V vertices as its first V vertices."""
import numpy as np

LD = np.longdouble


def normalize_model(raw, first, C, color_lo, color_hi, normalize):
    """raw [rows, C] float64, first [nclouds + 1] -> (rows [rows, C], centroid [nclouds, 3], max_distance [nclouds]), all
    longdouble.  A cloud of no rows has NaN centroid / max_distance (nothing to pin); a cloud of one row has
    max_distance 0 and NaN xyz, as numpy's 0 / 0.  normalize = 0: centroid / max_distance are None."""
    raw = np.asarray(raw, dtype=np.float64).reshape(-1, C)
    first = [int(f) for f in first]
    assert color_lo >= 3 or color_hi <= color_lo, "the colour columns come after xyz"
    out = raw.astype(LD)
    out[:, color_lo:color_hi] /= LD(256)
    if not normalize:
        return out, None, None
    ncl = len(first) - 1
    cen, md = np.full((ncl, 3), np.nan, dtype=LD), np.full(ncl, np.nan, dtype=LD)
    for i in range(ncl):
        lo, hi = first[i], first[i + 1]
        if hi == lo:
            continue
        xyz = out[lo:hi, :3]
        cen[i] = xyz.sum(axis=0) / LD(hi - lo)
        d = xyz - cen[i]
        md[i] = np.sqrt((d * d).sum(axis=1)).max()
        with np.errstate(invalid="ignore", divide="ignore"):
            out[lo:hi, :3] = d / md[i]
    return out, cen, md


def _augmented(rows64, aug_b):
    """float32 rows of float64 rows [n, C] under aug_b = (flip_x, flip_y, cos t, sin t): longdouble, one rounding"""
    fx, fy, c, s = (LD(v) for v in aug_b)
    r = np.asarray(rows64, dtype=np.float64).astype(LD)
    x, y = fx * r[:, 0], fy * r[:, 1]
    out = r.copy()
    with np.errstate(invalid="ignore"):
        out[:, 0] = x * c - y * s
        out[:, 1] = x * s + y * c
    return out.astype(np.float32)


def gather_model(norm64, first, cloud, rows_or_choice, aug, out_first=None, capacity=None):
    """norm64 [rows, C] float64 (the table as read back from the device), first [nclouds + 1], cloud [B], aug [B, 4].
    Sampled form (out_first is None): rows_or_choice = choice [B, P], positions inside cloud[b] -> points [B, P, C] float32.
    Packed form: rows_or_choice is None, out_first [B + 1] ascending, capacity -> (points [capacity, C] float32,
    point_counts [B] int64): sample b owns the output rows out_first[b] .. out_first[b+1]-1 below out_first[B] and
    `capacity`, and output row r of it is position r - out_first[b] of cloud[b].
    Zeros for a cloud index outside 0 .. nclouds-1 and for a position outside 0 .. n-1; point_counts 0 for such a cloud."""
    norm64 = np.asarray(norm64, dtype=np.float64)
    C = norm64.shape[1]
    first = [int(f) for f in first]
    ncl, B = len(first) - 1, len(cloud)
    aug = np.asarray(aug, dtype=np.float64).reshape(B, 4)

    def rows_of(b, pos):
        out = np.zeros((len(pos), C), dtype=np.float32)
        cl = int(cloud[b])
        if 0 <= cl < ncl:
            n = first[cl + 1] - first[cl]
            ok = (pos >= 0) & (pos < n)
            out[ok] = _augmented(norm64[first[cl] + pos[ok]], aug[b])
        return out

    if out_first is None:
        choice = np.asarray(rows_or_choice, dtype=np.int64).reshape(B, -1)
        return np.stack([rows_of(b, choice[b]) for b in range(B)])
    assert rows_or_choice is None
    out_first = [int(f) for f in out_first]
    assert len(out_first) == B + 1 and all(a <= b for a, b in zip(out_first, out_first[1:])), "out_first ascends"
    points = np.zeros((capacity, C), dtype=np.float32)
    counts = np.zeros(B, dtype=np.int64)
    for b in range(B):
        cl = int(cloud[b])
        if 0 <= cl < ncl:
            counts[b] = first[cl + 1] - first[cl]
        lo, hi = max(out_first[b], 0), min(out_first[b + 1], out_first[B], capacity)
        if hi > lo:
            points[lo:hi] = rows_of(b, np.arange(lo, hi, dtype=np.int64) - out_first[b])
    return points, counts


def pair_index(i, j, c):
    """position of pair (i, j), i < j < c, among the pairs of c vertices in lexicographic order"""
    return i * c - i * (i + 1) // 2 + (j - i - 1)


def targets_model(wf_vertices, wf_edges, vfirst, efirst, cloud, aug, V):
    """wf_vertices [sum c, 3] float64, wf_edges [sum e, 2] int, vfirst / efirst [nclouds + 1], cloud [B], aug [B, 4] ->
    dict(vertices [B, V, 3] f32, vertex_existence [B, V] f32, vertex_counts [B] int64, edge_labels [B, V(V-1)/2] f32):
    train_targets(..., full_width=True) of the samples' wireframes, the vertices augmented like the points.  c_s > V:
    the first V vertices, labels among the pairs of V vertices, vertex_counts = c_s.  Unknown cloud: zeros, count 0."""
    wf_vertices = np.asarray(wf_vertices, dtype=np.float64).reshape(-1, 3)
    wf_edges = np.asarray(wf_edges, dtype=np.int64).reshape(-1, 2)
    vfirst, efirst = [int(f) for f in vfirst], [int(f) for f in efirst]
    ncl, B = len(vfirst) - 1, len(cloud)
    aug = np.asarray(aug, dtype=np.float64).reshape(B, 4)
    verts = np.zeros((B, V, 3), dtype=np.float32)
    exist = np.zeros((B, V), dtype=np.float32)
    counts = np.zeros(B, dtype=np.int64)
    labels = np.zeros((B, V * (V - 1) // 2), dtype=np.float32)
    for b in range(B):
        cl = int(cloud[b])
        if not 0 <= cl < ncl:
            continue
        cs = vfirst[cl + 1] - vfirst[cl]
        counts[b] = cs
        c = min(cs, V)
        if c:
            verts[b, :c] = _augmented(wf_vertices[vfirst[cl]:vfirst[cl] + c], aug[b])
        exist[b, :c] = 1.0
        for a, d in wf_edges[efirst[cl]:efirst[cl + 1]].tolist():
            i, j = min(a, d), max(a, d)
            if 0 <= i < j < c:
                labels[b, pair_index(i, j, c)] = 1.0
    return {"vertices": verts, "vertex_existence": exist, "vertex_counts": counts, "edge_labels": labels}
