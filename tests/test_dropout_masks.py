"""Statistical gates on the dropout hash the kernels use (csrc/wf3d_common.h, wf3d_keep), through its host restatement
oracle/dropout.py (which tests/test_dropout_gpu.py holds bit for bit to every kernel that applies a mask).

These pin the QUALITY of the masks, not their bits: any replacement hash has to pass them too.  Each rate is compared
with the Bernoulli expectation at 5 standard deviations, with the exact keep probability of the integer threshold
(1 - thresh / 2^32) as the mean:
  - the drop rate at p in {0.05, 0.1, 0.5, 0.9} over >= 10^7 draws;
  - the four site seeds derived from one drop seed give independent masks on the (row, column) ranges the sites share;
  - adjacent rows, adjacent columns and the `heads` attention rows of one query are independent;
  - no two mask rows repeat over cfg5's 1,044,480 edge rows (B = 32, V = 256);
  - seeds with the top bit set behave like the others.
"""
import numpy as np
import pytest

import helpers  # noqa: F401  (sets sys.path)
from oracle import dropout as D

SEEDS = [0x12345678, 0x9E3779B9, 0xFFFFFFFF, 0x80000000, 7]      # three of them >= 2^31
CFG5_EDGE_ROWS = 32 * (256 * 255 // 2)


def p_exact(p):
    return D.thresh_scale(p)[0] / 2.0 ** 32


def within(count, n, prob, k=5.0):
    """|count - n prob| <= k sigma of Binomial(n, prob)."""
    sd = np.sqrt(n * prob * (1 - prob))
    return abs(count - n * prob) <= k * sd, (count / n, prob, (count - n * prob) / sd)


def dropped(seed, rows, cols, p):
    return ~D.keep(seed, rows, cols, p)


def test_threshold_and_scale_follow_the_c_abi():
    """drop_p crosses the ABI as a float: thresh = (uint32)((double)(float)p * 2^32), scale = 1.0f / (1.0f - (float)p)."""
    for p in (0.05, 0.1, 0.2, 0.3, 0.5, 0.9, 1e-9, 0.999):
        t, s = D.thresh_scale(p)
        p32 = np.float32(p)
        assert t == int(float(p32) * 4294967296.0) and 0 < t < 2 ** 32
        assert s.dtype == np.float32 and s == np.float32(1) / (np.float32(1) - p32)
    assert D.thresh_scale(0.0)[0] == 0 and D.keep(1, np.arange(9), 3, 0.0).all()
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            D.thresh_scale(bad)


def test_site_seeds_are_the_golden_ratio_steps_mod_2_32():
    assert D.site_seeds(0) == [0x9E3779B9, (2 * 0x9E3779B9) & 0xFFFFFFFF, (3 * 0x9E3779B9) & 0xFFFFFFFF,
                               (4 * 0x9E3779B9) & 0xFFFFFFFF]
    big = (1 << 63) - 5                                  # torch's random_() draws up to 2^63 - 1
    assert D.site_seeds(big) == [(big + k * 0x9E3779B9) % 2 ** 32 for k in range(1, 5)]


@pytest.mark.parametrize("p", [0.05, 0.1, 0.5, 0.9])
@pytest.mark.parametrize("seed", [0x12345678, 0xC0FFEE01])
def test_keep_rate_is_binomial(p, seed):
    rows, cols = np.arange(4000)[:, None], np.arange(2560)[None, :]          # 10.24 M draws
    d = int(dropped(seed, rows, cols, p).sum())
    ok, info = within(d, rows.size * cols.size, p_exact(p))
    assert ok, info


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", SEEDS)
def test_site_seeds_give_pairwise_independent_masks(p, seed):
    """Every pair of the four sites on the index ranges they share: vertex / edge rows 0 .. 16383 by columns 0 .. 511
    (vertex_proj.5 at H = 512, edge_mlp.3 / .7 at 512 / 256 wide) and attention rows 0 .. 16383 (Rv * heads at cfg5) by
    key columns 0 .. 255.  Joint drop rate p^2."""
    sd = D.site_seeds(seed)
    rows, cols = np.arange(16384)[:, None], np.arange(512)[None, :]
    m = [dropped(s, rows, cols, p) for s in sd]
    q = p_exact(p)
    for a in range(4):
        for b in range(a + 1, 4):
            ok, info = within(int((m[a] & m[b]).sum()), m[a].size, q * q)
            assert ok, (a, b, info)
            ok, info = within(int((m[a][:, :256] & m[b][:, :256]).sum()), m[a][:, :256].size, q * q)
            assert ok, (a, b, "attention columns", info)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", SEEDS)
def test_adjacent_rows_columns_and_heads_are_independent(p, seed):
    q = p_exact(p)
    rows, cols = np.arange(8193)[:, None], np.arange(513)[None, :]
    m = dropped(seed, rows, cols, p)
    n = 8192 * 512
    ok, info = within(int((m[:-1, :-1] & m[1:, :-1]).sum()), n, q * q)          # (r, c) with (r + 1, c)
    assert ok, ("rows", info)
    ok, info = within(int((m[:-1, :-1] & m[:-1, 1:]).sum()), n, q * q)          # (r, c) with (r, c + 1)
    assert ok, ("columns", info)
    ok, info = within(int((m[:-1, :-1] & m[1:, 1:]).sum()), n, q * q)           # diagonal neighbour
    assert ok, ("diagonal", info)
    # attention: rows (query * heads + h) of one query, heads = 8, against every other head of the same query
    heads, queries, keys = 8, 2048, 256
    qi = np.arange(queries)[:, None, None]
    h = np.arange(heads)[None, :, None]
    j = np.arange(keys)[None, None, :]
    a = dropped(seed, qi * heads + h, j, p)                                      # [query, head, key]
    for h1 in range(heads):
        for h2 in range(h1 + 1, heads):
            ok, info = within(int((a[:, h1] & a[:, h2]).sum()), queries * keys, q * q)
            assert ok, ("heads", h1, h2, info)


def test_no_two_edge_mask_rows_repeat_at_cfg5():
    """1,044,480 edge rows (cfg5) of the first 64 columns at p = 0.5: 64 random bits per row, so a repeat among ~10^6
    rows would have probability ~3e-8 for an ideal hash; any repeat is a structural defect (a period in the row index)."""
    seed = D.site_seeds(0x5EED5EED)[2]
    cols = np.arange(64)[None, :]
    keys = []
    for r0 in range(0, CFG5_EDGE_ROWS, 1 << 17):
        rows = np.arange(r0, min(r0 + (1 << 17), CFG5_EDGE_ROWS))[:, None]
        keys.append(np.packbits(D.keep(seed, rows, cols, 0.5), axis=1).view(np.uint64).reshape(-1))
    keys = np.concatenate(keys)
    assert keys.size == CFG5_EDGE_ROWS
    assert np.unique(keys).size == keys.size


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_seeds_with_the_top_bit_set_behave_like_the_others(p):
    """seed and seed ^ 2^31 give independent masks, each at the binomial rate."""
    q = p_exact(p)
    rows, cols = np.arange(4096)[:, None], np.arange(1024)[None, :]
    for lo in (0x00000001, 0x1234ABCD, 0x7FFFFFFF):
        hi = lo | 0x80000000
        a, b = dropped(lo, rows, cols, p), dropped(hi, rows, cols, p)
        for m in (a, b):
            ok, info = within(int(m.sum()), m.size, q)
            assert ok, (hex(lo), info)
        ok, info = within(int((a & b).sum()), a.size, q * q)
        assert ok, (hex(lo), "joint", info)
