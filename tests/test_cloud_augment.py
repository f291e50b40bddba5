"""The augmentation extension of the sampled forms — random scale, per-point jitter, random point dropout — as
wf3d/sampling.py specifies it: configuration checks, the dropout rule, the jitter's arithmetic and statistics, and the
world-size invariance of the per-(epoch, slot) values.  No GPU; tests/test_cloud_augment_gpu.py holds the kernels to
these functions bit for bit.

The statistical bounds are 5 sigma of the estimator over n samples of a unit-variance value with excess kurtosis -0.3
(Irwin-Hall of four): sd(mean) = 1 / sqrt(n), sd(var) = sqrt((kurtosis - 1) / n) = sqrt(1.7 / n), sd(correlation) =
1 / sqrt(n); the dropped fraction of n rows has sd sqrt(drop (1 - drop) / n)."""
import numpy as np
import pytest

from wf3d import sampling as S

FULL = {"scale": (0.8, 1.25), "anisotropic": True, "jitter_sigma": 0.01, "jitter_clip": 0.05, "max_dropout": 0.875}


def test_check_augment_accepts_each_key_and_fills_the_rest():
    assert S.check_augment(None) is None and S.check_augment({}) is None
    identity = {"scale": (1.0, 1.0), "anisotropic": False, "jitter_sigma": 0.0, "jitter_clip": np.inf, "max_dropout": 0.0}
    for key, value in FULL.items():
        cfg = {key: value}
        got = S.check_augment(cfg)
        assert got == dict(identity, **{key: value}) and got is not cfg and cfg == {key: value}
    assert S.check_augment(FULL) == FULL
    assert S.check_augment({"scale": [2, 2]})["scale"] == (2.0, 2.0)                   # lo == hi, integers
    assert S.check_augment({"jitter_clip": np.inf})["jitter_clip"] == np.inf
    assert S.check_augment({"max_dropout": 1})["max_dropout"] == 1.0
    assert S.augment_cfg8(FULL).tolist() == [0.8, 1.25, 1.0, 0.01, 0.05, 0.875, 0.0, 0.0]
    assert S.augment_cfg8(None).tolist() == [1.0, 1.0, 0.0, 0.0, np.inf, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("cfg", [
    {"scale": (0.0, 1.0)}, {"scale": (-1.0, 1.0)}, {"scale": (1.2, 1.1)}, {"scale": (1.0, np.inf)}, {"scale": (np.nan, 1.0)},
    {"scale": 1.0}, {"scale": (1.0, 1.1, 1.2)}, {"anisotropic": 1}, {"anisotropic": "yes"},
    {"jitter_sigma": -0.01}, {"jitter_sigma": np.inf}, {"jitter_sigma": np.nan}, {"jitter_sigma": True},
    {"jitter_clip": 0.0}, {"jitter_clip": -1.0}, {"jitter_clip": np.nan}, {"jitter_clip": None},
    {"max_dropout": -0.1}, {"max_dropout": 1.5}, {"max_dropout": np.nan}, {"max_dropout": "half"},
    {"translate": 0.1}, [("scale", (1.0, 1.0))], "scale"])
def test_check_augment_rejects(cfg):
    with pytest.raises(ValueError, match="augment"):
        S.check_augment(cfg)


def test_constants_are_pinned_and_distinct():
    keys = (S.KEY_FLIP, S.KEY_ANGLE, S.KEY_ROWS, S.KEY_SCALE, S.KEY_SCALE + 1, S.KEY_SCALE + 2, S.KEY_DROPOUT, S.KEY_JITTER, S.KEY_DROP)
    assert len(set(keys)) == len(keys) and all(0 < k < 1 << 64 for k in keys)
    assert (S.KEY_SCALE, S.KEY_DROPOUT, S.KEY_JITTER, S.KEY_DROP) == (0xA54FF53A5F1D36F1, 0x510E527FADE682D1,
                                                                     0x9B05688C2B3E6C1F, 0x1F83D9ABFB41BD6B)
    assert S.JITTER_C.hex() == "0x1.bb67ae8584caap-16" and S.JITTER_C == np.sqrt(3.0) * 2.0 ** -16
    assert S.JITTER_MAX <= 3.4641


def test_dropout_rule():
    p = np.arange(4096)
    for word, b in ((0, 0), (0xDEADBEEF, 3), (1 << 31, 4095)):
        assert not S.dropped(word, b, p, 0.0).any()                                    # drop = 0 drops nothing
        d1 = S.dropped(word, b, p, 1.0)
        assert not d1[0] and d1[1:].all()                                              # drop = 1: every row but row 0
        assert not S.dropped(word, b, p, np.nan).any()
        for drop in (0.25, 0.5, 0.99):
            d = S.dropped(word, b, p, drop)
            assert not d[0] and S.dropped(word, b, 0, drop) is False
            eff = S.effective_rows(word, b, p.size, drop)
            assert (eff[d] == 0).all() and (eff[~d] == p[~d]).all()                    # a dropped row's p_eff is 0
            assert bool(d[7]) == S.dropped(word, b, 7, drop)                           # scalar and vector forms agree
        # monotone in drop: one uniform value per row decides
        assert not (S.dropped(word, b, p, 0.25) & ~S.dropped(word, b, p, 0.5)).any()
    # the rule, spelled out for one row
    key, key2 = S.sample_keys([77], 2)
    K = (int(key[0]) << 32) | int(key2[0])
    u = float(int(S.mix64(K ^ S.KEY_DROP, 5)[0]) >> 11) * 2.0 ** -53
    assert S.dropped(77, 2, 5, np.nextafter(u, 1.0)) and not S.dropped(77, 2, 5, u)


@pytest.mark.parametrize("drop", [0.1, 0.5, 0.875])
def test_dropped_fraction(drop):
    n = 1 << 16
    for word, b in ((1, 0), (0x9E3779B9, 1), (0xFFFFFFFF, 31)):
        frac = S.dropped(word, b, np.arange(1, n + 1), drop).mean()
        print(f"drop {drop} word {word:#x} b {b}: fraction {frac:.5f}, bound {5 * np.sqrt(drop * (1 - drop) / n):.5f}")
        assert abs(frac - drop) <= 5 * np.sqrt(drop * (1 - drop) / n)


def test_augment_point_arithmetic():
    xyz = np.array([[-0.0, 0.0, -0.0], [0.3, -0.7, 0.1], [1.0 / 3.0, 2.0 / 3.0, -1.0 / 7.0]])
    g = np.array([[1.0, -2.0, 3.0], [0.25, -0.25, 3.4], [-3.4, 0.0, 1.0 / 3.0]])
    # sigma = 0 adds nothing: -0.0 keeps its sign, and an identity row is fp32(xyz)
    out = S.augment_point(xyz, S.EXT_IDENTITY, g)
    assert out.dtype == np.float32 and np.array_equal(out.view(np.int32), xyz.astype(np.float32).view(np.int32))
    assert np.signbit(out[0]).tolist() == [True, False, True]
    # sigma > 0 adds even a zero jitter: -0.0 + 0.0 = +0.0
    assert not np.signbit(S.augment_point(xyz[0], (1, 1, 1, 1e-3, np.inf, 0, 0, 0), np.zeros(3))).any()
    # every operation rounded on its own, one rounding to fp32
    ext = np.array([1.1, 0.9, 1.3, 1.0, 0.5, 0.0, 0.0, 0.0])
    want = np.empty((3, 3), dtype=np.float32)
    for i in range(3):
        for k in range(3):
            prod = np.float64(xyz[i, k]) * ext[k]
            j = min(max(np.float64(1.0) * g[i, k], -0.5), 0.5)
            want[i, k] = np.float32(prod + j)
    got = S.augment_point(xyz, ext, g)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert got[0].tolist() == [0.5, -0.5, 0.5]                                         # the clip binds on both sides
    # a NaN scale, sigma or clip gives NaNs; a broadcast over leading axes
    for k in (0, 3, 4):
        bad = ext.copy()
        bad[k] = np.nan
        assert np.isnan(S.augment_point(xyz, bad, g)).any()
    assert S.augment_point(xyz[None].repeat(2, 0), ext, g[None].repeat(2, 0)).shape == (2, 3, 3)


def test_jitter_noise_definition():
    key, key2 = S.sample_keys([123456789], 5)
    K = ((int(key[0]) << 32) | int(key2[0])) ^ S.KEY_JITTER
    for p in (0, 1, 4095, (1 << 31) - 1):
        want = []
        for k in range(3):
            z = int(S.mix64(K, 3 * p + k)[0])
            total = (z & 0xFFFF) + ((z >> 16) & 0xFFFF) + ((z >> 32) & 0xFFFF) + (z >> 48)
            want.append(float(total - 131070) * S.JITTER_C)
        assert S.jitter_noise(123456789, 5, p).tolist() == want
    many = S.jitter_noise(123456789, 5, np.array([0, 1, 4095]))
    assert many.shape == (3, 3) and many[2].tolist() == S.jitter_noise(123456789, 5, 4095).tolist()
    assert not np.array_equal(S.jitter_noise(123456789, 5, 9), S.jitter_noise(123456789, 6, 9))       # keyed by b
    assert not np.array_equal(S.jitter_noise(123456789, 5, 9), S.jitter_noise(123456790, 5, 9))       # and by the word


@pytest.mark.parametrize("word,b", [(0, 0), (0x9E3779B9, 7), (0xFFFFFFFF, 4095)])
def test_jitter_noise_statistics(word, b):
    n = 1 << 20
    g = S.jitter_noise(word, b, np.arange(n))
    assert g.shape == (n, 3)
    tol = 5 / np.sqrt(n)
    assert np.abs(g).max() <= 3.4641
    for k in range(3):
        x = g[:, k]
        mean, var = x.mean(), x.var()
        lag = np.mean(x[:-1] * x[1:])
        cross = np.mean(x * g[:, (k + 1) % 3])
        print(f"word {word:#x} b {b} axis {k}: mean {mean:.2e} var - 1 {var - 1:.2e} lag-1 {lag:.2e} cross {cross:.2e} "
              f"(bounds {tol:.2e}, {5 * np.sqrt(1.7 / n):.2e})")
        assert abs(mean) <= tol
        assert abs(var - 1.0) <= 5 * np.sqrt(1.7 / n)
        assert abs(lag) <= tol and abs(cross) <= tol
    flat = g.reshape(-1)                                           # consecutive counters: k to k + 1, and across points
    assert abs(np.mean(flat[:-1] * flat[1:])) <= 5 / np.sqrt(flat.size - 1)


def test_epoch_ext_depends_on_epoch_and_slot_only():
    key, D, B = 0x1234ABCD5678EF01, 40, 4
    S1 = S.epoch_steps(D, 2 * B)                                   # world 1, batch 2 B: the same steps as world 2, batch B
    assert S1 == S.epoch_steps(D, B, 2, 0) == 5
    for t in (0, 3, S1 - 1, S1, 2 * S1 + 1):
        whole = S.epoch_batch(key, t, D, 2 * B, augment_ext=FULL)
        halves = [S.epoch_batch(key, t, D, B, 2, r, augment_ext=FULL) for r in (0, 1)]
        assert whole["ext"].shape == (2 * B, 8) and whole["ext"].dtype == np.float64
        assert np.array_equal(np.concatenate([h["ext"] for h in halves]), whole["ext"])
        assert np.array_equal(np.concatenate([h["aug"] for h in halves]), whole["aug"])
        ext = whole["ext"]
        assert ((0.8 <= ext[:, :3]) & (ext[:, :3] <= 1.25)).all() and not (ext[:, 0] == ext[:, 1]).any()
        assert (ext[:, 3] == 0.01).all() and (ext[:, 4] == 0.05).all() and (ext[:, 6:] == 0).all()
        assert ((0 <= ext[:, 5]) & (ext[:, 5] <= 0.875)).all()
        assert np.array_equal(ext, S.epoch_augment_ext(key, whole["epoch"], whole["slots"], FULL))
    # the same slots in the next epoch: other values
    a, b = S.epoch_batch(key, S1 - 1, D, 2 * B, augment_ext=FULL), S.epoch_batch(key, 2 * S1 - 1, D, 2 * B, augment_ext=FULL)
    assert np.array_equal(a["slots"], b["slots"]) and a["epoch"] + 1 == b["epoch"]
    assert not (a["ext"][:, [0, 1, 2, 5]] == b["ext"][:, [0, 1, 2, 5]]).any()
    # isotropic: one scale for the three axes; parts that are not configured are the identity's
    iso = S.epoch_batch(key, 3, D, B, augment_ext={"scale": (0.5, 2.0)})["ext"]
    assert (iso[:, 0] == iso[:, 1]).all() and (iso[:, 1] == iso[:, 2]).all() and len(set(iso[:, 0])) == B
    assert (iso[:, 3] == 0).all() and np.isinf(iso[:, 4]).all() and (iso[:, 5] == 0).all()
    only_jitter = S.epoch_batch(key, 3, D, B, augment_ext={"jitter_sigma": 0.02})["ext"]
    assert np.array_equal(only_jitter, np.tile([1.0, 1.0, 1.0, 0.02, np.inf, 0.0, 0.0, 0.0], (B, 1)))
    # no configuration: no entry, and the rest of the batch is what it was
    plain = S.epoch_batch(key, 3, D, B)
    assert "ext" not in plain and "ext" not in S.epoch_batch(key, 3, D, B, augment_ext={})
    with_ext = S.epoch_batch(key, 3, D, B, augment_ext=FULL)
    assert all(np.array_equal(plain[k], with_ext[k]) for k in plain)
    # the value, spelled out for one slot
    c = (with_ext["epoch"] << 32) + int(with_ext["slots"][2])
    u = float(int(S.mix64(key ^ (S.KEY_SCALE + 1), c)[0]) >> 11) * 2.0 ** -53
    assert with_ext["ext"][2, 1] == 0.8 + u * (1.25 - 0.8)
    ud = float(int(S.mix64(key ^ S.KEY_DROPOUT, c)[0]) >> 11) * 2.0 ** -53
    assert with_ext["ext"][2, 5] == ud * 0.875


def test_host_rows_and_draw_counts():
    assert S.ext_draws(None) == (0, 0) and S.ext_draws({"jitter_sigma": 0.1}) == (0, 0)
    assert S.ext_draws({"scale": (0.9, 1.1)}) == (1, 0) and S.ext_draws(FULL) == (3, 1)
    assert S.ext_draws({"scale": (1.0, 1.0), "max_dropout": 0.5}) == (0, 1)
    assert S.ext_row({"jitter_sigma": 0.1}).tolist() == [1, 1, 1, 0.1, np.inf, 0, 0, 0]
    row = S.ext_row(FULL, [0.0, 0.5, 0.25], 0.5)
    assert row.tolist() == [0.8, 0.8 + 0.5 * (1.25 - 0.8), 0.8 + 0.25 * (1.25 - 0.8), 0.01, 0.05, 0.4375, 0.0, 0.0]
    assert S.ext_row({"scale": (0.5, 1.5)}, [0.75]).tolist() == [1.25, 1.25, 1.25, 0.0, np.inf, 0.0, 0.0, 0.0]
