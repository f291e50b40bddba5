"""Farthest-point sampling as wf3d.sampling states it — fps_start, fps_order, fps_indices: the specification
csrc/cloud.hip's cloud_fps_kernel is held to bit for bit on the GPU (tests/test_cloud_fps_gpu.py) — without a GPU.
Everything is exact: integer indices, and distances on coordinates whose squares float64 holds exactly."""
import numpy as np
import pytest

from wf3d.sampling import choice_indices, fmix32, fps_indices, fps_order, fps_start, mulhi, sample_keys

LATTICE = np.array([(i // 16, (i // 4) % 4, i % 4) for i in range(64)], dtype=np.float64)       # row i = (x, y, z), z fastest
# From row 21 = (1, 1, 1).  By hand: the farthest is (3, 3, 3) = row 63 alone (r = 12).  Then d = 9 at (0, 3, 3), (3, 0, 3)
# and (3, 3, 0) = rows 15, 51, 60 — each 9 from both picks — and less everywhere else: the LOWEST index, 15, is next,
# then 51 and 60 (still 9: they are 18 from row 15).  Then d = 6 at rows 3, 12, 48 in index order, and so on; from the
# 20th pick every remaining d is 1 and the rest follow in ascending order.  The list is the output of a plain Python
# double loop over integer distances (strict `>` while scanning upwards), not of the code under test.
LATTICE_ORDER_FROM_21 = [21, 63, 15, 51, 60, 3, 12, 48, 0, 42, 6, 9, 18, 23, 24, 29, 33, 36, 53, 1, 2, 4, 5, 7, 8, 10, 11, 13, 14,
                         16, 17, 19, 20, 22, 25, 26, 27, 28, 30, 31, 32, 34, 35, 37, 38, 39, 40, 41, 43, 44, 45, 46, 47, 49, 50,
                         52, 54, 55, 56, 57, 58, 59, 61, 62]


def _clouds():
    rng = np.random.RandomState(5)
    return {"gauss": rng.standard_normal((97, 3)), "lattice": LATTICE, "same": np.tile([[0.25, -1.5, 3.0]], (33, 1)),
            "clusters": np.repeat(np.array([[0.0, 0.0, 0.0], [1.0, 2.0, -1.0]]), [20, 21], axis=0),
            "utm": np.array([5e5, 5.4e6, 300.0]) + rng.uniform(-20, 20, (64, 3))}


@pytest.mark.parametrize("name", sorted(_clouds()))
def test_full_order_is_a_permutation_and_shorter_orders_are_its_prefixes(name):
    xyz = _clouds()[name]
    n = xyz.shape[0]
    for start in (0, n // 3, n - 1):
        full = fps_order(xyz, start, n)
        assert full.dtype == np.int64 and full[0] == start and sorted(full.tolist()) == list(range(n))
        for L in (1, 2, n // 2, n - 1):
            assert np.array_equal(fps_order(xyz, start, L), full[:L])


def test_lattice_order_pins_the_lowest_index_among_equals():
    assert fps_order(LATTICE, 21, 64).tolist() == LATTICE_ORDER_FROM_21
    # the same cloud far from the origin and scaled by a power of two: the same exact distances, the same order
    assert fps_order(LATTICE * 0.125 + 4096.0, 21, 64).tolist() == LATTICE_ORDER_FROM_21


def test_identical_points_come_in_index_order_after_the_start():
    xyz = _clouds()["same"]
    n = xyz.shape[0]
    for start in (0, 7, n - 1):
        assert fps_order(xyz, start, n).tolist() == [start] + [i for i in range(n) if i != start]


def test_distances_are_rounded_operation_by_operation():
    """r = (xx + yy) + zz: from the origin, row 2 = (1.25, 1, 2^27) has xx + yy = 2.5625, more than half an ulp (4) of
    zz = 2^54, so r = 2^54 + 4 and it beats row 1 = (0, 0, 2^27), r = 2^54.  As xx + (yy + zz) both terms would be
    absorbed one by one, the two rows would tie and row 1 would win by index."""
    xyz = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 2.0 ** 27], [1.25, 1.0, 2.0 ** 27]])
    assert 1.5625 + (1.0 + 2.0 ** 54) == 2.0 ** 54 and (1.5625 + 1.0) + 2.0 ** 54 == 2.0 ** 54 + 4.0
    assert fps_order(xyz, 0, 2).tolist() == [0, 2]


def test_indices_repeat_cyclically_when_the_cloud_is_shorter():
    xyz = _clouds()["gauss"][:11]
    for seed, b in ((0, 0), (12345, 3), (0xFFFFFFFF, 4095)):
        start = fps_start(seed, b, 11)
        order = fps_order(xyz, start, 11)
        for P in (1, 10, 11, 12, 23, 40):
            idx = fps_indices(seed, b, xyz, P)
            assert idx.dtype == np.int64 and idx.shape == (P,)
            assert np.array_equal(idx, order[np.arange(P) % 11])
    assert np.array_equal(fps_indices(9, 2, xyz[:1], 5), np.zeros(5, dtype=np.int64))


def _fmix32_int(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    return x ^ (x >> 16)


@pytest.mark.parametrize("seed", [0, 1, 12345, 0xFFFFFFFF])
def test_start_is_the_random_samplers_offset_a(seed):
    for b in (0, 1, 17, 4095):
        for n in (1, 2, 3, 64, 65, 1276, 14039, (1 << 31) - 1):
            key = int(sample_keys([seed], b)[0][0])
            assert key == _fmix32_int(_fmix32_int(seed + 0x9E3779B9) ^ (((b + 1) * 0x85EBCA6B) & 0xFFFFFFFF))
            a = (_fmix32_int(key ^ 0xB5297A4D) * n) >> 32                 # choice_indices' `a`, in Python integers
            assert fps_start(seed, b, n) == a == int(mulhi(fmix32(np.uint64(key ^ 0xB5297A4D)), n)) and 0 <= a < n
    # a is where choice_indices starts its walk: with n = P = 1 both samplers take row 0
    assert fps_start(seed, 0, 1) == 0 and choice_indices(seed, 0, 1, 1).tolist() == [0]


def test_start_is_uniform():
    n = 10
    counts = np.bincount([fps_start(s, 0, n) for s in range(4000)], minlength=n)
    assert abs(counts - 400).max() < 5 * np.sqrt(400 * 0.9)             # a binomial count within five standard deviations


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_rows_end_in_range(bad):
    xyz = _clouds()["gauss"][:40].copy()
    xyz[13, 1] = bad
    for start in (0, 13):
        full = fps_order(xyz, start, 40)
        assert sorted(full.tolist()) == list(range(40))
        # a NaN r lowers nothing: the row keeps +inf and is the first pick after the start
        assert start == 13 or full[1] == 13
    xyz[27] = np.nan
    idx = fps_indices(3, 1, xyz, 100)
    assert idx.min() >= 0 and idx.max() < 40 and sorted(idx[:40].tolist()) == list(range(40))


def test_limits():
    xyz = _clouds()["gauss"]
    for kw in (dict(start=0, L=0), dict(start=0, L=98), dict(start=97, L=1), dict(start=-1, L=1)):
        with pytest.raises(ValueError, match="fps_order"):
            fps_order(xyz, **kw)
    with pytest.raises(ValueError, match="fps_order"):
        fps_order(xyz[:, :2], 0, 1)
    with pytest.raises(ValueError, match="fps_indices"):
        fps_indices(0, 0, xyz, 0)
    with pytest.raises(ValueError, match="fps_indices"):
        fps_indices(0, 0, xyz[:0], 4)
    for n in (0, 1 << 31):
        with pytest.raises(ValueError, match="fps_start"):
            fps_start(0, 0, n)
