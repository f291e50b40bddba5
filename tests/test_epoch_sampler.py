"""The epoch sampler's specification (wf3d/sampling.py: epoch_order, epoch_batch, epoch_cos_sin) and the host side of
datasets.building3d.EpochSampler.  No GPU: the kernel is held to this specification in tests/test_epoch_sampler_gpu.py."""
import types

import numpy as np
import pytest
import torch

KEYS = (0, 1, 0x9E3779B97F4A7C15, 0xDEADBEEF12345678, (1 << 64) - 1)


def test_mix64_is_the_documented_splitmix64_step():
    from wf3d.sampling import mix64
    M = (1 << 64) - 1
    for key in KEYS:
        for n in (0, 1, 5, (1 << 33) + 1, M):
            z = (key + (n + 1) * 0x9E3779B97F4A7C15) & M
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
            assert int(mix64(key, n)[0]) == z ^ (z >> 31)
    assert mix64(7, [0, 1, 2]).tolist() == [int(mix64(7, n)[0]) for n in range(3)]
    # splitmix64's published first outputs for seed 0 (Steele, Lea, Flood): the stream of key 0
    assert [int(mix64(0, n)[0]) for n in range(2)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]


@pytest.mark.parametrize("D", [1, 2, 5, 17, 64, 65, 300])
def test_epoch_order_is_a_permutation_and_epochs_differ(D):
    from wf3d.sampling import epoch_order
    for key in KEYS:
        orders = [epoch_order(key, e, D) for e in range(6)]
        for o in orders:
            assert o.dtype == np.int64 and sorted(o.tolist()) == list(range(D))
        if D >= 17:                                                # 6 of >= 17! orders: a repeat would be a defect
            assert len({tuple(o.tolist()) for o in orders}) == 6
    if D >= 17:
        assert not np.array_equal(epoch_order(KEYS[0], 0, D), epoch_order(KEYS[1], 0, D))


def test_drop_last():
    from wf3d.sampling import epoch_batch, epoch_order, epoch_steps
    D, B, W = 65, 8, 2
    assert epoch_steps(D, B, W, 0) == 4
    key = KEYS[3]
    for e in (0, 1, 5):
        seen = []
        for s in range(4):
            for r in range(W):
                got = epoch_batch(key, e * 4 + s, D, B, W, r)
                assert (got["epoch"], got["step"]) == (e, s)
                assert got["slots"].tolist() == list(range(s * 16 + r * 8, s * 16 + r * 8 + 8))
                seen += got["order"].tolist()
        assert len(set(seen)) == 64 == len(seen)                   # 64 of the 65 members, each once: one is dropped
        assert seen == epoch_order(key, e, D)[:64].tolist()
    assert epoch_batch(key, 4, D, B, W, 0)["epoch"] == 1           # t = S: the next epoch begins


@pytest.mark.parametrize("W", [2, 3])
def test_rank_shards_are_disjoint_and_their_union_is_the_single_rank_batch(W):
    from wf3d.sampling import epoch_batch
    D, B, key = 300, 7, KEYS[2]
    for t in (0, 3, 13, 14, 15, (1 << 33) + 1):
        whole = epoch_batch(key, t, D, W * B, 1, 0)
        parts = [epoch_batch(key, t, D, B, W, r) for r in range(W)]
        order = np.concatenate([p["order"] for p in parts])
        assert len(set(order.tolist())) == W * B
        assert np.array_equal(order, whole["order"])
        assert np.array_equal(np.concatenate([p["slots"] for p in parts]), whole["slots"])
        assert np.concatenate([p["aug"] for p in parts]).tobytes() == whole["aug"].tobytes()
        # the row seed is per (step, rank)
        assert len({int(p["seed_words"][0]) for p in parts}) == W
        for p in parts:
            s = int(p["seed_words"][0])
            assert p["seed_words"].dtype == np.uint32
            assert p["seed_words"].tolist() == [(s + k * 0x9E3779B9) & 0xFFFFFFFF for k in range(5)]


def test_augmentation_draws():
    from wf3d.sampling import epoch_augmentation, epoch_batch
    aug, angle = epoch_augmentation(KEYS[3], 2, np.arange(4000))
    for col in (0, 1):
        assert set(aug[:, col].tolist()) == {-1.0, 1.0}
        assert 1700 < int((aug[:, col] < 0).sum()) < 2300           # a fair coin: 2000 +- 6.7 sigma (sigma = 31.6)
    assert 900 < int(((aug[:, 0] < 0) & (aug[:, 1] < 0)).sum()) < 1100           # the two bits are not one bit
    assert float(np.abs(angle).max()) <= np.pi / 36
    assert angle.min() < -0.08 and angle.max() > 0.08                # the range is used
    # another epoch, another draw for the same slot
    assert not np.array_equal(epoch_augmentation(KEYS[3], 3, np.arange(64))[1], angle[:64])
    off = epoch_batch(KEYS[3], 9, 300, 8, augment=False)
    assert off["aug"].tolist() == [[1.0, 1.0, 1.0, 0.0]] * 8 and not off["angle"].any()


def test_cos_and_sin_polynomials():
    """within 1e-14 of numpy on +-pi/36: a dozen roundings of at most 2^-53 each leave a tenfold margin, and the
    truncation is below 1e-25"""
    from wf3d.sampling import epoch_cos_sin
    t = np.concatenate([np.linspace(-np.pi / 36, np.pi / 36, 28000), [0.0, -np.pi / 36, np.pi / 36]])
    c, s = epoch_cos_sin(t)
    assert float(np.abs(c - np.cos(t)).max()) < 1e-14 and float(np.abs(s - np.sin(t)).max()) < 1e-14
    assert float(np.abs(c * c + s * s - 1.0).max()) < 1e-14
    assert epoch_cos_sin(0.0) == (1.0, 0.0)
    # the recurrences as the issue states them, on scalars
    for v in (0.0871, -0.031, np.pi / 36):
        x, ps, pc = np.float64(v) * np.float64(v), np.float64(1.0), np.float64(1.0)
        for k in (13, 11, 9, 7, 5, 3):
            ps = 1.0 - x * ps / (k * (k - 1))
        for k in (12, 10, 8, 6, 4, 2):
            pc = 1.0 - x * pc / (k * (k - 1))
        got = epoch_cos_sin(v)
        assert float(got[0]) == float(pc) and float(got[1]) == float(np.float64(v) * ps)


def _fake_cache(n_clouds, augment=True):
    """what EpochSampler reads of a DeviceCloudCache on the host"""
    return types.SimpleNamespace(n=[10 + k for k in range(n_clouds)], device=torch.device("cpu"),
                                 ds=types.SimpleNamespace(augment=augment))


def test_batch_at_is_a_pure_function_of_key_and_t():
    from datasets.building3d import EpochSampler
    from wf3d.sampling import epoch_batch
    cache = _fake_cache(40)
    members = [39 - k for k in range(0, 40, 2)] + [3, 3]               # a split, in another order, one cloud twice
    a, b = EpochSampler(cache, 4, members, seed=77), EpochSampler(cache, 4, members, seed=77)
    assert a.steps_per_epoch == 5 and a.key == 77
    for t in (0, 4, 5, 11, (1 << 33) + 1):
        x, y, again = a.batch_at(t), b.batch_at(t), a.batch_at(t)
        spec = epoch_batch(77, t, 22, 4)
        for got in (x, y, again):
            assert got["cloud"].dtype == np.int32 and got["cloud"].tolist() == [members[i] for i in spec["order"]]
            assert got["aug"].tobytes() == spec["aug"].tobytes() and got["seed_words"].tolist() == spec["seed_words"].tolist()
    assert a.batch_at(0)["cloud"].tolist() != EpochSampler(cache, 4, members, seed=78).batch_at(0)["cloud"].tolist()
    # seed=None: keyed from torch's CPU generator, so torch.manual_seed reproduces it
    torch.manual_seed(5)
    k1 = EpochSampler(cache, 4).key
    torch.manual_seed(5)
    assert EpochSampler(cache, 4).key == k1 and 0 <= k1 < 1 << 64
    # the block of a batch: the layout of include/wf3d.h, both out_first forms
    block = a.block_at(7, num_points=9).numpy()
    spec = a.batch_at(7)
    assert block.size == 40 * 4 + 4 and block[:128].tobytes() == spec["aug"].tobytes()
    assert block[128:144].view(np.int32).tolist() == spec["cloud"].tolist()
    assert block[144:].view(np.int32).tolist() == [0, 9, 18, 27, 36]
    rows = [cache.n[i] for i in spec["cloud"]]
    assert a.block_at(7).numpy()[144:].view(np.int32).tolist() == [0] + np.cumsum(rows).tolist()


def test_limits_are_refused():
    from datasets.building3d import EpochSampler
    from wf3d.sampling import epoch_batch, epoch_steps
    for D, B, W, r in ((0, 1, 1, 0), (1 << 31, 1, 1, 0), (10, 0, 1, 0), (10000, 4097, 1, 0), (10, 2, 2, -1), (10, 2, 2, 2),
                       (10, 2, 0, 0), (10, 6, 2, 0), (5, 6, 1, 0)):
        with pytest.raises(ValueError, match="epoch sampler"):
            epoch_steps(D, B, W, r)
        with pytest.raises(ValueError, match="epoch sampler"):
            epoch_batch(1, 0, D, B, W, r)
    assert epoch_steps(10, 5, 2, 1) == 1 and epoch_steps((1 << 31) - 1, 4096, 1, 0) == ((1 << 31) - 1) // 4096
    cache = _fake_cache(12)
    with pytest.raises(ValueError, match="world > 1 needs an explicit integer seed"):
        EpochSampler(cache, 2, world=2, rank=0)
    with pytest.raises(ValueError, match="seed must be an integer or None"):
        EpochSampler(cache, 2, seed=True)
    with pytest.raises(TypeError):
        EpochSampler(cache, 2, world=2, seed=1.5)
    with pytest.raises(ValueError, match="world \\* B = 16 passes the 12 member clouds"):
        EpochSampler(cache, 8, world=2, rank=1, seed=3)
    with pytest.raises(ValueError, match="0 <= rank < world"):
        EpochSampler(cache, 2, world=2, rank=2, seed=3)
    with pytest.raises(ValueError, match="1 <= D"):
        EpochSampler(cache, 1, members=[])
    assert EpochSampler(cache, 3, world=2, rank=1, seed=3).steps_per_epoch == 2
