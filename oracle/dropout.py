"""Host restatement of the HIP path's dropout masks.

TEST INFRASTRUCTURE ONLY.  Every dropout mask of the edge head is a pure function of (seed, row, column): the kernels
never store one, they recompute the bit where they need it (csrc/wf3d_common.h, wf3d_keep).  This module computes the
same bits in numpy, so that a test can build the exact masks a forward drew and hand them to the fp64 oracle
(oracle/reference_cpu.py, `drop=`), or check a kernel's zeros element by element.

    keep(seed, row, col, p)   the kernels' keep bit, uint32 arithmetic, bit for bit
    thresh_scale(p)           the threshold and the fp32 scale the C ABI derives from a float drop_p
    site_seeds(seed)          the four per-site seeds EdgeFn.forward derives from the seed it draws
    edge_head_masks(...)      per-sample, pre-scaled masks of all four sites in the oracle's `drop=` format

Rows follow the ragged layout of wf3d.ops.EdgeMeta: sample s owns vertex rows voff[s] .. voff[s+1]-1 and edge rows
eoff[s] .. eoff[s+1]-1 (pairs i < j in lexicographic order).  Attention rows are (voff[s] + i) * heads + h for query i
and head h, columns the key index j within the sample.
"""
import numpy as np

# the sites in the order EdgeFn.forward gives them seeds (k = 1..4) and EdgePredictor._dropout_ps lists their p
SITES = ("vertex_proj.5", "attention", "edge_mlp.3", "edge_mlp.7")

_U = np.uint32
_GOLDEN = 0x9E3779B9


def thresh_scale(p):
    """(thresh, scale) as the C entry points derive them: drop_p crosses the ABI as a float, thresh =
    (uint32)((double)drop_p * 2^32), scale = 1.0f / (1.0f - drop_p) in fp32.  p = 0 gives thresh 0 (no mask)."""
    p32 = np.float32(p)
    if not 0.0 <= float(p32) < 1.0:
        raise ValueError(f"drop_p must be in [0, 1), got {p}")
    thresh = int(float(np.float64(p32)) * 4294967296.0) if p32 > 0 else 0
    scale = np.float32(1.0) / (np.float32(1.0) - p32)
    return thresh, scale


def hash32(seed, row, col):
    """The uint32 hash wf3d_keep compares against the threshold (arrays broadcast)."""
    row = np.asarray(row).astype(np.int64).astype(_U)
    col = np.asarray(col).astype(np.int64).astype(_U)
    with np.errstate(over="ignore"):
        h = _U(int(seed) & 0xFFFFFFFF) ^ (row * _U(0x9E3779B1)) ^ (col * _U(0x85EBCA77) + _U(0x27D4EB2F))
        h = h ^ (h >> _U(16))
        h = h * _U(0x7FEB352D)
        h = h ^ (h >> _U(15))
        h = h * _U(0x846CA68B)
        h = h ^ (h >> _U(16))
    return h


def keep(seed, row, col, p):
    """Bool keep-bit of element (row, col) under `seed` at drop probability p (all True for p = 0)."""
    thresh, _ = thresh_scale(p)
    if thresh == 0:
        return np.ones(np.broadcast(np.asarray(row), np.asarray(col)).shape, dtype=bool)
    return hash32(seed, row, col) >= _U(thresh)


def scaled(seed, row, col, p, dtype=np.float64):
    """The multiplicative mask the kernels apply: keep * scale (fp32 scale, as the kernels compute it), 0 where dropped."""
    _, scale = thresh_scale(p)
    return np.where(keep(seed, row, col, p), dtype(scale), dtype(0))


def site_seeds(seed):
    """sd[k-1] = (seed + 0x9E3779B9 * k) mod 2^32, k = 1..4, for the sites in SITES order (wf3d/functional.py, EdgeFn)."""
    return [(int(seed) + _GOLDEN * k) & 0xFFFFFFFF for k in range(1, 5)]


def offsets(counts):
    """(voff, eoff) of EdgeMeta for these vertex counts."""
    voff, eoff = [0], [0]
    for c in counts:
        voff.append(voff[-1] + c)
        eoff.append(eoff[-1] + c * (c - 1) // 2)
    return voff, eoff


def vertex_rows(voff_s, v, width, seed, p):
    """[v, width] mask of one sample's vertex rows voff_s .. voff_s + v - 1."""
    r = np.arange(voff_s, voff_s + v)[:, None]
    return scaled(seed, r, np.arange(width)[None, :], p)


def attention_weights(voff_s, v, heads, seed, p):
    """[heads, v, v] mask on one sample's softmax weights: [h, i, j] at row (voff_s + i) * heads + h, column j."""
    h = np.arange(heads)[:, None, None]
    i = np.arange(v)[None, :, None]
    j = np.arange(v)[None, None, :]
    return scaled(seed, (voff_s + i) * heads + h, j, p)


def edge_rows(eoff_s, v, width, seed, p):
    """[v(v-1)/2, width] mask of one sample's edge rows eoff_s .. (pairs i < j, lexicographic)."""
    e = v * (v - 1) // 2
    r = np.arange(eoff_s, eoff_s + e)[:, None]
    return scaled(seed, r, np.arange(width)[None, :], p)


def edge_head_masks(seed, counts, ps, hidden, heads, s0=0, s1=None):
    """Per sample, {site: pre-scaled mask} of one EdgeFn forward with drop seed `seed` and site probabilities `ps`
    (SITES order), in the shapes oracle.reference_cpu.edge_forward(drop=...) takes for a one-sample batch:
    vertex_proj.5 [1, v, hidden], attention [1, heads, v, v], edge_mlp.3 [E, hidden], edge_mlp.7 [E, hidden // 2].
    A site with p = 0 is left out (no mask).  `counts` are the whole batch's; [s0, s1) selects the samples returned
    (default all), their rows placed by the batch-global offsets, so that a large batch's masks can be built a few
    samples at a time."""
    sd = site_seeds(seed)
    voff, eoff = offsets(counts)
    out = []
    for s in range(s0, len(counts) if s1 is None else s1):
        v = counts[s]
        m = {}
        if ps[0] > 0:
            m[SITES[0]] = vertex_rows(voff[s], v, hidden, sd[0], ps[0])[None]
        if ps[1] > 0:
            m[SITES[1]] = attention_weights(voff[s], v, heads, sd[1], ps[1])[None]
        if ps[2] > 0:
            m[SITES[2]] = edge_rows(eoff[s], v, hidden, sd[2], ps[2])
        if ps[3] > 0:
            m[SITES[3]] = edge_rows(eoff[s], v, hidden // 2, sd[3], ps[3])
        out.append(m)
    return out
