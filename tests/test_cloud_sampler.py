"""The device sampler's index function, wf3d.sampling.choice_indices — the specification csrc/cloud.hip's sampler kernels
are held to on the GPU (tests/test_cloud_sampler_gpu.py) — and the host plan of a sampled fixed-size batch
(datasets.building3d.packed_plan with num_points), without a GPU.

Deterministic: seed words are 0 .. S-1, not random.  The statistical bounds are those of the ideal distribution, not
fitted ones: a binomial count within 5 standard deviations, a chi-square statistic below dof + 5 sqrt(2 dof) (its mean
plus five of its standard deviations).  Pair statistics are asserted from n = 64 up only: a 6-round Feistel network on
the few bits of a smaller n is visibly not a uniform random permutation."""
import functools
import os
import types

import numpy as np
import pytest

import helpers as H

ROOT = os.path.join(H.GOLDEN, "building3d")
S = 20000
SIZES = list(range(1, 70)) + [255, 256, 257, 1023, 1025, 4096, 4097, 14039]
SEEDS = [0, 1, 12345, 0xFFFFFFFF]
INCLUSION = [(2, 1), (3, 2), (5, 3), (16, 4), (17, 5), (64, 16), (65, 16), (1000, 100), (1276, 256)]


def chi_bound(dof):
    return dof + 5.0 * np.sqrt(2.0 * dof)


@functools.lru_cache(maxsize=None)
def _draws(n, P):
    """choice_indices(s, 0, n, P) for s = 0 .. S-1, computed once: int64 [S, P]"""
    from wf3d.sampling import choice_indices_many
    idx = choice_indices_many(np.arange(S), 0, n, P)
    idx.setflags(write=False)
    return idx


# ---------------------------------------------------------------------------------------------------------------------
# without replacement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_permutation_and_prefixes(seed):
    from wf3d.sampling import choice_indices
    for n in SIZES:
        full = choice_indices(seed, 3, n, n)
        assert full.dtype == np.int64 and full.shape == (n,)
        assert sorted(full.tolist()) == list(range(n)), n
        for P in {1, n // 2, n - 1} - {0, n}:
            part = choice_indices(seed, 3, n, P)
            assert part.shape == (P,) and len(set(part.tolist())) == P and 0 <= part.min() and part.max() < n, (n, P)
            assert np.array_equal(part, full[:P]), (n, P)           # a position's index does not depend on P while P <= n


def test_many_is_the_scalar_function():
    from wf3d.sampling import choice_indices, choice_indices_many
    words = [0, 7, 0x80000000, 0xFFFFFFFF]
    for b, n, P in ((0, 5, 3), (2, 1276, 64), (1, 3, 300), (4095, 65, 65)):
        many = choice_indices_many(words, b, n, P)
        assert many.shape == (len(words), P)
        for w, row in zip(words, many):
            assert np.array_equal(choice_indices(w, b, n, P), row)
    assert np.array_equal(choice_indices(-1, 0, 100, 10), choice_indices(0xFFFFFFFF, 0, 100, 10))     # an int32 word's bits
    for bad in ((0, 4), (1 << 31, 4), (4, 0)):
        with pytest.raises(ValueError):
            choice_indices(0, 0, *bad)


def test_cycle_walk_is_bounded():
    """The walks of a whole permutation visit every value of the Feistel domain at most once: 4^h < 4 n applications for
    n indices (fewer than 4 per index), and no walk longer than the 4^h - n values outside [0, n) plus one."""
    from wf3d.sampling import choice_indices_many, half_bits
    seen = 0
    for n in SIZES:
        domain = 4 ** half_bits(n)
        assert n <= domain < 4 * n or n == 1 == domain
        for seed in SEEDS:
            _, longest, total = choice_indices_many([seed], 3, n, n, return_walks=True)
            assert n <= total <= domain and 1 <= longest <= domain - n + 1, (n, seed)
            seen = max(seen, longest)
    print(f"longest cycle walk: {seen} applications")


@pytest.mark.parametrize("n,P", INCLUSION, ids=str)
def test_inclusion_frequencies(n, P):
    idx = _draws(n, P)
    assert idx.min() >= 0 and idx.max() < n
    assert (np.sort(idx, axis=1)[:, 1:] != np.sort(idx, axis=1)[:, :-1]).all()            # distinct in every draw
    p = P / n
    count = np.bincount(idx.ravel(), minlength=n)
    z = np.abs(count - S * p) / np.sqrt(S * p * (1 - p))
    print(f"n = {n}, P = {P}: largest inclusion deviation {z.max():.2f} sd")
    assert z.max() < 5.0


@pytest.mark.parametrize("n,P", INCLUSION, ids=str)
def test_first_position_is_uniform(n, P):
    first = np.bincount(_draws(n, P)[:, 0], minlength=n)
    chi = float(((first - S / n) ** 2 / (S / n)).sum())
    print(f"n = {n}: first-position chi-square {chi:.1f} at dof {n - 1}")
    assert chi < chi_bound(n - 1)


@pytest.mark.parametrize("n", [64, 65])
def test_first_pair_is_uniform(n):
    idx = _draws(n, 16)
    table = np.bincount(idx[:, 0] * n + idx[:, 1], minlength=n * n).reshape(n, n)
    assert np.trace(table) == 0
    cells = table[~np.eye(n, dtype=bool)]
    expect = S / cells.size
    chi = float(((cells - expect) ** 2 / expect).sum())
    print(f"n = {n}: (first, second) chi-square {chi:.0f} at dof {cells.size - 1}")
    assert chi < chi_bound(cells.size - 1)


# ---------------------------------------------------------------------------------------------------------------------
# with replacement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,P", [(1, 8), (3, 300), (17, 300)], ids=str)
def test_replacement(n, P):
    from wf3d.sampling import choice_indices_many
    idx = choice_indices_many(np.arange(2000), 0, n, P)
    assert idx.shape == (2000, P) and idx.min() >= 0 and idx.max() < n
    count = np.bincount(idx.ravel(), minlength=n)
    expect = 2000 * P / n
    chi = float(((count - expect) ** 2 / expect).sum())
    print(f"n = {n}, P = {P}: chi-square {chi:.1f} at dof {n - 1}")
    assert chi <= chi_bound(n - 1)
    if n > 1:
        assert len({tuple(r) for r in idx[:50].tolist()}) == 50


# ---------------------------------------------------------------------------------------------------------------------
# samples of one batch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,P", [(1276, 256), (100, 100), (17, 300)], ids=str)
def test_samples_of_a_batch_differ(n, P):
    from wf3d.sampling import choice_indices
    for seed in SEEDS:
        lists = {tuple(choice_indices(seed, b, n, P).tolist()) for b in range(32)}
        assert len(lists) == 32
    assert not np.array_equal(choice_indices(0, 0, n, P), choice_indices(1, 0, n, P))


# ---------------------------------------------------------------------------------------------------------------------
# the host plan of a sampled batch
# ---------------------------------------------------------------------------------------------------------------------
def _ds0(augment):
    from datasets import Building3DReconstructionDataset
    cfg = types.SimpleNamespace(root_dir=ROOT, num_points=0, use_color=True, use_intensity=True, normalize=True, augment=augment)
    return Building3DReconstructionDataset(cfg, split_set="train")


def _sizes(ds):
    from datasets.building3d import load_wireframe
    return [ds[i]["point_clouds"].shape[0] for i in range(len(ds))], [load_wireframe(f)[0].shape[0] for f in ds.wireframe_files]


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("seed,indices", [(5, [0, 1]), (6, [1, 1, 0])], ids=str)
def test_plan_draws_what_the_packed_plan_draws(augment, seed, indices):
    from datasets.building3d import packed_plan
    ds = _ds0(augment)
    n, nv = _sizes(ds)
    draw = ds._draw_augmentation if augment else None
    np.random.seed(seed)
    idx_p, _, aug_p = packed_plan(n, nv, indices, draw)
    after_packed = np.random.random()
    np.random.seed(seed)
    idx_s, out_first, aug_s = packed_plan(n, nv, indices, draw, num_points=300)
    assert np.random.random() == after_packed                         # the same draws: no choice draws
    assert idx_s == idx_p and np.array_equal(aug_s, aug_p)
    assert out_first.dtype == np.int32 and out_first.tolist() == [b * 300 for b in range(len(indices) + 1)]
    # no row capacity: P far below and far above the clouds' lengths, and a capacity argument is not consulted
    assert packed_plan(n, nv, indices, None, num_points=1)[1].tolist() == list(range(len(indices) + 1))
    assert packed_plan(n, nv, indices, None, capacity=256, num_points=100000)[1][-1] == 100000 * len(indices)


def test_plan_refusals_come_before_any_draw():
    from datasets.building3d import packed_plan
    ds = _ds0(True)
    n, nv = _sizes(ds)
    big = nv.index(8)
    np.random.seed(3)
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match="a wireframe has 8 vertices, more than max_vertices = 4"):
        packed_plan(n, nv, [big], ds._draw_augmentation, max_vertices=4, num_points=64)
    with pytest.raises(IndexError, match="index out of range for 2 clouds"):
        packed_plan(n, nv, [0, 2], ds._draw_augmentation, num_points=64)
    with pytest.raises(ValueError, match="empty batch"):
        packed_plan(n, nv, [], ds._draw_augmentation, num_points=64)
    with pytest.raises(ValueError, match=r"B \* num_points < 2\^31"):
        packed_plan(n, nv, [0, 1], ds._draw_augmentation, num_points=1 << 30)
    with pytest.raises(ValueError, match="num_points >= 1"):
        packed_plan(n, nv, [0, 1], ds._draw_augmentation, num_points=-1)
    assert np.array_equal(np.random.get_state()[1], state)
