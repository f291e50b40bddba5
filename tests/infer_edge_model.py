"""A numpy statement of what the forward-only edge head's two kernels compute besides arithmetic (include/wf3d.h,
"FORWARD-ONLY edge head"): the live rows of each block of the walk, and which pair of which sample a global edge row is.
The reference of tests/test_infer_edge_stream_gpu.py, checked against edge_index_lists in
tests/test_infer_edge_stream.py."""
import numpy as np


def block_live(total, rows, Re, nblocks):
    """blive[k] = clamp(total - k * rows, 0, min(rows, Re - k * rows)), int32 [nblocks]."""
    k = np.arange(nblocks, dtype=np.int64)
    cap = np.maximum(np.minimum(rows, Re - k * rows), 0)
    return np.minimum(np.maximum(int(total) - k * rows, 0), cap).astype(np.int32)


def edge_offsets(counts):
    """eoff [B + 1]: sample s owns the edge rows eoff[s] .. eoff[s + 1] - 1, its c(c - 1)/2 pairs; a sample with fewer
    than 2 vertices owns none."""
    c = np.asarray(counts, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(c * (c - 1) // 2)])


def edge_row(counts, e):
    """Global edge row e -> (sample, i, j), or None at or past the live total.  The sample is the one whose rows hold e
    (samples without rows are never the answer); (i, j) is pair e - eoff[s] of its c vertices in lexicographic order:
    i is the largest first vertex whose pairs start at or before it, offset(i) = i (2c - i - 1) / 2."""
    eoff = edge_offsets(counts)
    if not 0 <= e < eoff[-1]:
        return None
    s = int(np.searchsorted(eoff, e, side="right")) - 1
    c, r = int(counts[s]), int(e - eoff[s])
    i = 0
    while (i + 1) * (2 * c - i - 2) // 2 <= r:
        i += 1
    return s, i, r - i * (2 * c - i - 1) // 2 + i + 1


def block_rows(counts, e0, n):
    """[(sample, i, j) or None] of the rows e0 .. e0 + n - 1: what one block of the walk works on."""
    return [edge_row(counts, e) for e in range(e0, e0 + n)]
