"""Seeded fp32 cost matrices for the assignment solver's tests (test_loss_assign_model.py on the CPU,
test_loss_assign_forms_gpu.py on the device).  Every generator returns float32 [B, V, V]; EXACT names those whose
entries are integers or dyadic fractions, so that any sum of V of them is exact in float64 and two optimal totals
must be equal, not merely close."""
import zlib

import numpy as np

SQUARE = ("gauss", "gauss_minus_100", "gauss_scaled", "product", "ints_0_3", "constant", "rank_one", "perm_matrix")
WIREFRAME = ("wf_lattice", "wf_shifted")
EXACT = {"product", "ints_0_3", "constant", "rank_one", "perm_matrix", "wf_lattice"}


def _rng(name, V, salt=0):
    return np.random.default_rng([zlib.crc32(name.encode()), V, salt])


def assert_optimal_permutation(C, c4r, exact):
    """c4r is a permutation of 0..V-1 whose total on C (float32 values, summed in float64) is scipy's: equal when the
    costs are integers or dyadic, within 1e-12 relative (tests/test_loss.py's bound) otherwise."""
    from scipy.optimize import linear_sum_assignment
    V = C.shape[0]
    assert sorted(int(c) for c in c4r) == list(range(V)), "not a permutation"
    C64 = C.astype(np.float64)
    ri, ci = linear_sum_assignment(C64)
    ours, ref = C64[np.arange(V), c4r].sum(), C64[ri, ci].sum()
    if exact:
        assert ours == ref, (ours, ref)
    else:
        assert abs(ours - ref) <= 1e-12 * max(1.0, abs(ref)), (ours, ref)


def product_optimum(V):
    """sum_k k (V + 1 - k): ascending rows meet descending columns (rearrangement inequality), unique as the factors are distinct."""
    return V * (V + 1) * (V + 2) // 6


def square_costs(name, V, B):
    rng = _rng(name, V)
    if name == "gauss":
        C = rng.standard_normal((B, V, V))
    elif name == "gauss_minus_100":
        C = rng.standard_normal((B, V, V)).astype(np.float32) - np.float32(100.0)
    elif name == "gauss_scaled":
        C = rng.standard_normal((B, V, V)) * 10.0 ** rng.uniform(-6.0, 6.0, (B, V, V))
    elif name == "product":
        C = np.stack([np.outer(rng.permutation(V) + 1, rng.permutation(V) + 1) for _ in range(B)])
    elif name == "ints_0_3":
        C = rng.integers(0, 4, (B, V, V))
    elif name == "constant":
        C = np.broadcast_to(rng.integers(-3, 4, (B, 1, 1)) + 0.5, (B, V, V))
    elif name == "rank_one":
        C = rng.integers(-4, 5, (B, V, 1)) + rng.integers(-4, 5, (B, 1, V))
    elif name == "perm_matrix":
        C = np.ones((B, V, V))
        for b in range(B):
            C[b, np.arange(V), rng.permutation(V)] = 0.0
    else:
        raise KeyError(name)
    return np.ascontiguousarray(C, dtype=np.float32)


def wireframe_inputs(name, V, counts, salt=0):
    """(pred vertices [B, V, 3], pred existence [B, V], target vertices [B, V, 3], counts int64 [B]), float32."""
    rng = _rng(name, V, salt)
    B = len(counts)
    if name == "wf_lattice":            # coordinates on a 0.5 grid in [-1, 1], existence on a 0.25 grid: exact costs, full of ties
        pv, tv = rng.integers(-2, 3, (B, V, 3)) * 0.5, rng.integers(-2, 3, (B, V, 3)) * 0.5
        pe = rng.integers(0, 5, (B, V)) * 0.25
    elif name == "wf_shifted":          # fp32 spacing at 1000 is 6e-5: differences of Gaussians quantised to it
        pv, tv = rng.standard_normal((B, V, 3)) + 1000.0, rng.standard_normal((B, V, 3)) + 1000.0
        pe = rng.uniform(0.0, 1.0, (B, V))
    elif name == "wf_gauss":
        pv, tv = rng.standard_normal((B, V, 3)), rng.standard_normal((B, V, 3))
        pe = rng.uniform(0.0, 1.0, (B, V))
    else:
        raise KeyError(name)
    return pv.astype(np.float32), pe.astype(np.float32), tv.astype(np.float32), np.asarray(counts, dtype=np.int64)


def wireframe_cost(pv, pe, tv, counts):
    """loss_cost_kernel in numpy fp32, same association: ((|dx| + |dy|) + |dz|) + |e - 1| for t < count, e for the dummy
    columns.  Additions, subtractions and fabs only, so it equals the device's matrix bit for bit (NaN where a coordinate is)."""
    B, V, _ = pv.shape
    d = np.abs(pv[:, :, None, :] - tv[:, None, :V, :])
    real = ((d[..., 0] + d[..., 1]) + d[..., 2]) + np.abs(pe - np.float32(1.0))[:, :, None]
    dummy = np.broadcast_to(pe[:, :, None], (B, V, V))
    return np.where(np.arange(V)[None, None, :] < counts[:, None, None], real, dummy).astype(np.float32)


def random_counts(name, V, B):
    """B counts in 0..V, V and 0 among them."""
    c = _rng(name + ".counts", V).integers(0, V + 1, B)
    c[0] = V
    if B > 1:
        c[1] = 0
    return c.astype(np.int64)


def partial_permutation_holes(C, salt):
    """C [B, V, V] with NaN / +inf written at the positions of a partial permutation (at most one per row and per
    column, between 1 and V // 2 of them, alternating NaN and +inf): the finite entries still hold a perfect matching."""
    C = C.copy()
    B, V, _ = C.shape
    rng = _rng("holes", V, salt)
    for b in range(B):
        k = int(rng.integers(1, V // 2 + 1))
        rows, cols = rng.permutation(V)[:k], rng.permutation(V)[:k]
        C[b, rows, cols] = np.where(np.arange(k) % 2 == 0, np.float32(np.nan), np.float32(np.inf))
    return C
