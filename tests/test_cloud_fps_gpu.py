"""Farthest-point sampling on the GPU — wf3d_cloud_sample_fps, and DeviceCloudCache's sampler="fps" in batch(),
sampled_buffers / stage / fill / fill_epoch and under capture — against its specification, wf3d.sampling.fps_indices, and
against the EXISTING gather kernel (wf3d_cloud_sample) handed the specification's rows.  The specification is bit for
bit (float64, every operation rounded on its own, the lowest index among equal distances), so every comparison is exact
equality: there is no tolerance.

Cloud lengths: around the wave (63 .. 65), around every workgroup size (255 .. 257, 1023 .. 1025), where the workgroup
grows (2048 | 2049, 4096 | 4097 rows: 8 rows per thread), and the register tier's limit FPS_REG_ROWS | + 1, where d
moves to the workspace.  Every launch also runs b = 0 .. B-1 on the same cloud: another start row each."""
import functools
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402

GOLDEN_ROOT = os.path.join(H.GOLDEN, "building3d")
SMALL = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
AUG = np.array([[-1.0, 1.0, np.cos(0.05), np.sin(0.05)], [1.0, -1.0, np.cos(-0.08), np.sin(-0.08)],
                [-1.0, -1.0, np.cos(0.02), np.sin(0.02)], [1.0, 1.0, 1.0, 0.0], [1.0, -1.0, np.cos(0.07), np.sin(0.07)]])
SAMPLED_KEYS = {"points", "vertices", "vertex_existence", "edge_labels", "vertex_counts", "params", "params_host", "params_copied",
                "sample_words"}


def dev():
    return torch.device("cuda:0")


def _rows(xyz, C, seed=0):
    """[n, C] float64 rows: xyz and C - 3 further columns"""
    xyz = np.asarray(xyz, dtype=np.float64)
    return np.ascontiguousarray(np.concatenate([xyz, np.random.RandomState(seed).uniform(0, 1, (xyz.shape[0], C - 3))], axis=1))


def _block(cloud_ids, aug, P):
    from datasets import DeviceCloudCache
    B = len(cloud_ids)
    block = torch.zeros(40 * B + 4, dtype=torch.uint8)
    v_aug, v_cloud, v_first = DeviceCloudCache._block_views(block, B)
    v_aug[:], v_cloud[:], v_first[:] = aug, cloud_ids, np.arange(B + 1) * P
    return block.to(dev())


def _launch(clouds, cloud_ids, word, aug, P, max_rows=None, want_idx=True):
    """wf3d_cloud_sample_fps on `clouds` (a list of [n, C] arrays; n = 0 allowed) -> (points, idx_out, code): every output
    poisoned first, the workspace sized by the library"""
    from wf3d import _lib
    from wf3d.ops import _stream
    lib, C, B = _lib.load(), clouds[0].shape[1], len(cloud_ids)
    first = np.zeros(len(clouds) + 1, dtype=np.int64)
    np.cumsum([c.shape[0] for c in clouds], out=first[1:])
    norm = torch.from_numpy(np.concatenate(clouds, axis=0)).to(dev())
    max_rows = max_rows or max(c.shape[0] for c in clouds)
    nbytes = lib.wf3d_cloud_sample_fps_ws_bytes(B, max_rows)
    assert (nbytes > 0) == (max_rows > _lib.DEFINES["WF3D_FPS_REG_ROWS"])
    ws = torch.full((max(nbytes, 1),), 0xA5, dtype=torch.uint8, device=dev())
    words = torch.tensor([word - (1 << 32) if word >= 1 << 31 else word, 1, 2, 3, 4], dtype=torch.int32, device=dev())
    points = torch.full((B, P, C), 7.0, dtype=torch.float32, device=dev())
    idx = torch.full((B, P), -7, dtype=torch.int32, device=dev())
    firsts = torch.from_numpy(first).to(dev())
    code = lib.wf3d_cloud_sample_fps(norm.data_ptr(), firsts.data_ptr(), len(clouds), _block(cloud_ids, aug, P).data_ptr(),
                                     words.data_ptr(), B, P, C, points.data_ptr(), idx.data_ptr() if want_idx else None, max_rows,
                                     ws.data_ptr() if nbytes else None, nbytes, _stream())
    torch.cuda.synchronize()
    return points, idx, code, (norm, firsts)


def _gathered(norm, firsts, cloud_ids, choice, aug, C):
    """the EXISTING host-choice kernel on the given rows"""
    from wf3d import _lib
    from wf3d.ops import _stream
    B, P = choice.shape
    ids = torch.tensor(cloud_ids, dtype=torch.int32, device=dev())
    ch = torch.from_numpy(np.ascontiguousarray(choice.astype(np.int32))).to(dev())
    ag = torch.from_numpy(np.ascontiguousarray(aug)).to(dev())
    out = torch.full((B, P, C), 5.0, dtype=torch.float32, device=dev())
    _lib.check(_lib.load().wf3d_cloud_sample(norm.data_ptr(), firsts.data_ptr(), ids.data_ptr(), ch.data_ptr(), ag.data_ptr(), B, P, C,
                                             out.data_ptr(), _stream()), "cloud_sample")
    torch.cuda.synchronize()
    return out


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _model(word, clouds, cloud_ids, P):
    from wf3d.sampling import fps_indices
    return np.stack([fps_indices(word, b, clouds[i][:, :3], P) for b, i in enumerate(cloud_ids)])


def _check(clouds, cloud_ids, word, P, max_rows=None, aug=None):
    B, C = len(cloud_ids), clouds[0].shape[1]
    aug = AUG[:B] if aug is None else aug
    points, idx, code, (norm, firsts) = _launch(clouds, cloud_ids, word, aug, P, max_rows)
    assert code == 0
    want = _model(word, clouds, cloud_ids, P)
    got = idx.cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want), (np.argwhere(got != want)[:4].tolist(), P, max_rows)
    assert _same_bits(points, _gathered(norm, firsts, cloud_ids, want, aug, C))
    return points, idx


@functools.lru_cache(maxsize=None)
def _gauss(n, C=8):
    return _rows(np.random.RandomState(n).standard_normal((n, 3)), C, n)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the entry point on synthetic clouds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SMALL)
def test_indices_and_points_are_the_specification(n):
    cloud = _gauss(n)
    for P in sorted({P for P in (1, n - 1, n, n + 3, 2 * n + 1) if P >= 1}):
        _check([cloud], [0, 0, 0], 1000 + n, P)


@pytest.mark.parametrize("max_rows", [257, 2049, 4097])
def test_every_workgroup_size_on_a_short_cloud(max_rows):
    """256, 512 and 1024 threads on 257 rows: most waves own no row at all, one owns a single row"""
    _check([_gauss(257)], [0, 0], 77, 260, max_rows=max_rows)
    _check([_gauss(1)], [0, 0], 78, 3, max_rows=max_rows)


@pytest.mark.parametrize("n", [2048, 2049, 4096, 4097])
def test_where_the_workgroup_grows(n):
    _check([_gauss(n)], [0, 0], 5 + n, 16)


def test_register_limit_and_the_workspace_tier():
    from datasets.building3d import FPS_REG_ROWS
    from wf3d import _lib
    assert FPS_REG_ROWS == _lib.DEFINES["WF3D_FPS_REG_ROWS"] == 8192
    for n in (FPS_REG_ROWS, FPS_REG_ROWS + 1):
        _check([_gauss(n)], [0, 0], 9 + n, 16)
    # both tiers in one launch: a short cloud keeps its registers when the longest resident cloud needs the workspace
    clouds = [_gauss(FPS_REG_ROWS + 1), _gauss(257)]
    _check(clouds, [1, 0, 1], 31, 16)
    # ... and a cloud longer than the caller said is written as zeros, like an empty one
    points, idx, code, _ = _launch(clouds, [1, 0], 31, AUG[:2], 16, max_rows=FPS_REG_ROWS)
    assert code == 0 and not bool(points[1].any()) and not bool(idx[1].any()) and bool(points[0].any())
    assert np.array_equal(idx[0].cpu().numpy(), _model(31, clouds, [1], 16)[0])


def _families():
    rng = np.random.RandomState(3)
    n = 257
    grid = np.array([(i // 49, (i // 7) % 7, i % 7) for i in range(343)], dtype=np.float64)[:n]
    return {"gauss": rng.standard_normal((n, 3)),
            "lattice": grid,                                                                   # exact ties in every round
            "same": np.tile([[0.3, -0.7, 0.1]], (n, 1)),
            "clusters": np.repeat(np.array([[0.0, 0.5, 0.0], [1.0, -2.0, 0.25]]), [128, 129], axis=0),
            "utm": np.array([5.0e5, 5.4e5, 4.9e5]) + rng.uniform(-30.0, 30.0, (n, 3))}         # un-normalised: the low bits decide


@pytest.mark.parametrize("C", [8, 4])
@pytest.mark.parametrize("family", sorted(_families()))
def test_coordinate_families(family, C):
    cloud = _rows(_families()[family], C, 1)
    for P in (257, 260):
        _, idx = _check([cloud], [0, 0, 0], 4242, P)
        assert sorted(idx[0, :257].tolist()) == list(range(257))                               # coincident rows too: a permutation


def test_non_finite_rows_end_and_stay_in_range():
    xyz = _families()["gauss"].copy()
    xyz[100, 2], xyz[7, 0], xyz[200] = np.nan, np.inf, -np.inf
    _, idx = _check([_rows(xyz, 4, 1)], [0, 0], 6, 300)
    assert 0 <= int(idx.min()) and int(idx.max()) < 257


def test_mixed_batch_with_samples_that_have_no_source():
    clouds = [_gauss(65, 4), np.zeros((0, 4)), _gauss(1025, 4), _gauss(2, 4)]
    ids = [2, 7, 0, 1, 3]                                      # 7: outside the resident clouds; 1: an empty cloud
    P = 70
    for want_idx in (True, False):
        points, idx, code, (norm, firsts) = _launch(clouds, ids, 2024, AUG, P, want_idx=want_idx)
        assert code == 0
        live = [0, 2, 4]
        from wf3d.sampling import fps_indices                  # the specification keys a sample by its position in the batch
        want = np.stack([fps_indices(2024, b, clouds[ids[b]][:, :3], P) for b in live])
        full = np.zeros((5, P), dtype=np.int64)
        full[live] = want
        ref = _gathered(norm, firsts, [ids[b] if b in live else 0 for b in range(5)], full, AUG, 4)
        for b in (1, 3):
            ref[b] = 0.0
        assert _same_bits(points, ref)
        if want_idx:
            assert np.array_equal(idx.cpu().numpy(), full)
        else:
            assert bool((idx == -7).all())                     # NULL: not written


def test_argument_checks_launch_nothing():
    from wf3d import _lib
    lib = _lib.load()
    norm = torch.from_numpy(_gauss(65)).to(dev())
    first = torch.tensor([0, 65], dtype=torch.int64, device=dev())
    words = torch.zeros(5, dtype=torch.int32, device=dev())
    points = torch.full((2, 8, 8), 7.0, dtype=torch.float32, device=dev())
    idx = torch.full((2, 8), -7, dtype=torch.int32, device=dev())
    args = dict(norm=norm.data_ptr(), first=first.data_ptr(), nclouds=1, params=_block([0, 0], AUG[:2], 8).data_ptr(),
                words=words.data_ptr(), B=2, P=8, C=8, points=points.data_ptr(), idx=idx.data_ptr(), max_rows=65, ws=None, ws_bytes=0)

    def code(**kw):
        a = dict(args, **kw)
        return lib.wf3d_cloud_sample_fps(a["norm"], a["first"], a["nclouds"], a["params"], a["words"], a["B"], a["P"], a["C"],
                                         a["points"], a["idx"], a["max_rows"], a["ws"], a["ws_bytes"], None)
    for kw in (dict(P=0), dict(B=0), dict(B=4096, P=1 << 19), dict(points=None), dict(B=4097), dict(C=2), dict(nclouds=0),
               dict(max_rows=0), dict(words=None), dict(params=None), dict(norm=args["norm"] + 8), dict(idx=args["idx"] + 2),
               dict(max_rows=8193), dict(max_rows=8193, ws=args["norm"], ws_bytes=16)):
        assert code(**kw) == _lib.DEFINES["WF3D_ERR_ARG"], kw
        assert b"wf3d_cloud_sample_fps" in lib.wf3d_last_error()
    torch.cuda.synchronize()
    assert bool((points == 7.0).all()) and bool((idx == -7).all())
    assert lib.wf3d_cloud_sample_fps_ws_bytes(2, 8192) == 0 and lib.wf3d_cloud_sample_fps_ws_bytes(2, 8193) >= 2 * 8193 * 12
    assert code() == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. DeviceCloudCache on the fixture clouds
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair(split, P, augment=True):
    from datasets import Building3DReconstructionDataset, DeviceCloudCache
    cfg = types.SimpleNamespace(root_dir=GOLDEN_ROOT, num_points=P, normalize=True, augment=augment, use_color=True, use_intensity=True)
    ds = Building3DReconstructionDataset(cfg, split_set=split)
    torch.manual_seed(17 + P)
    return ds, DeviceCloudCache(ds, dev())


@functools.lru_cache(maxsize=None)
def _xyz(split, P, i):
    """cloud i's normalised xyz as it lies in the cache"""
    cache = _pair(split, P)[1]
    lo = int(cache.first[i])
    return cache.norm[lo:lo + cache.n[i], :3].cpu().numpy()


def _cache_model(split, P, ids, word0):
    from wf3d.sampling import fps_indices
    return np.stack([fps_indices(word0, b, _xyz(split, P, i), P) for b, i in enumerate(ids)])


def _word0(words):
    return int(words[0]) & 0xFFFFFFFF


def _specified_points(cache, ids, rows, aug):
    return _gathered(cache.norm, cache.first, ids, rows, aug, cache.ncol)


@pytest.mark.parametrize("split,ids", [("train", [1, 0, 1]), ("test", [0])])
def test_batch_returns_the_rows_it_took(split, ids):
    P = 96
    ds, cache = _pair(split, P)
    np.random.seed(5)
    dev_batch = cache.batch(ids, sampler="device")
    assert "point_indices" not in dev_batch
    state = cache.sample_generator.get_state()
    np.random.seed(5)
    got = cache.batch(ids, sampler="fps")
    after = np.random.random()
    np.random.seed(5)
    aug = np.array([(fx, fy, np.cos(t), np.sin(t)) for fx, fy, t in (ds._draw_augmentation() for _ in ids)])
    assert np.random.random() == after                                  # the augmentation draws only
    assert int(cache.sample_generator.get_state()[1]) == int(state[1]) + 1      # one seed word
    assert set(got) == set(dev_batch) | {"point_indices"}
    for k in set(dev_batch) - {"point_clouds"}:                          # the host fields: the same augmentation draws
        a, b = got[k], dev_batch[k]
        assert all(torch.equal(x, y) for x, y in zip(a, b)) if isinstance(a, list) else torch.equal(a, b), k
    idx = got["point_indices"]
    assert idx.is_cuda and idx.dtype == torch.int32 and tuple(idx.shape) == (len(ids), P)
    want = _cache_model(split, P, ids, _word0(cache.last_sample_words))
    assert np.array_equal(idx.cpu().numpy(), want)
    assert all(len(set(r.tolist())) == P for r in want)                 # every fixture cloud is longer than P: distinct rows
    assert _same_bits(got["point_clouds"], _specified_points(cache, ids, want, aug))


def test_unknown_samplers_are_refused():
    ds, cache = _pair("train", 96)
    for call in (lambda: cache.batch([0], sampler="farthest"), lambda: cache.sampled_buffers(2, 8, sampler="numpy")):
        with pytest.raises(ValueError, match="sampler must be") as e:
            call()
        assert "'device'" in str(e.value) and "'fps'" in str(e.value) and "'numpy'" in str(e.value)


def test_stage_and_fill_fps_buffers_and_device_buffers_are_unchanged():
    from wf3d.sampling import choice_indices
    P, ids = 96, [1, 0]
    ds, cache = _pair("train", P)
    plain = cache.sampled_buffers(2, 8)
    assert set(plain) == SAMPLED_KEYS and set(cache.sampled_buffers(2, 8, sampler="device")) == SAMPLED_KEYS
    buf = cache.sampled_buffers(2, 8, sampler="fps")
    assert set(buf) == SAMPLED_KEYS | {"sampler", "point_indices"} and buf["sampler"] == "fps"       # no cloud needs a workspace
    assert buf["point_indices"].dtype == torch.int32 and tuple(buf["point_indices"].shape) == (2, P)
    buf["points"].fill_(7.0)
    buf["point_indices"].fill_(-7)
    for b in (plain, buf):
        np.random.seed(12)
        cache.stage(b, ids)
        cache.fill(b)
    torch.cuda.synchronize()
    aug = cache._block_views(buf["params_host"], 2)[0].copy()
    assert torch.equal(plain["params_host"], buf["params_host"])
    want = _cache_model("train", P, ids, _word0(buf["sample_words"]))
    assert np.array_equal(buf["point_indices"].cpu().numpy(), want)
    assert _same_bits(buf["points"], _specified_points(cache, ids, want, aug))
    for k in ("vertices", "vertex_existence", "edge_labels", "vertex_counts"):
        assert torch.equal(plain[k], buf[k]), k
    # sampler="device": the random sampler's rows under its own word, as before
    rows = np.stack([choice_indices(_word0(plain["sample_words"]), b, cache.n[i], P) for b, i in enumerate(ids)])
    assert _same_bits(plain["points"], _specified_points(cache, ids, rows, aug))


def test_fill_epoch_starts_follow_the_epochs_seed_words():
    P = 96
    ds, cache = _pair("train", P)
    sampler = cache.epoch_sampler(2, seed=99)
    buf = cache.sampled_buffers(2, 8, sampler="fps")
    taken = []
    for t in range(2):
        cache.fill_epoch(buf, sampler)
        torch.cuda.synchronize()
        spec = sampler.batch_at(t)
        assert torch.equal(buf["params"].cpu(), sampler.block_at(t, P))
        assert np.array_equal(buf["sample_words"].cpu().numpy().view(np.uint32), spec["seed_words"])
        ids = spec["cloud"].tolist()
        want = _cache_model("train", P, ids, int(spec["seed_words"][0]))
        assert np.array_equal(buf["point_indices"].cpu().numpy(), want)
        assert _same_bits(buf["points"], _specified_points(cache, ids, want, spec["aug"]))
        taken.append(dict(zip(ids, want)))
    # the sample of a cloud differs from epoch to epoch by its start only: the same order from another row
    from wf3d.sampling import fps_order
    for i in (0, 1):
        for rows in (taken[0][i], taken[1][i]):
            assert np.array_equal(rows, fps_order(_xyz("train", P, i), int(rows[0]), P))
    assert any(taken[0][i][0] != taken[1][i][0] for i in (0, 1))


def test_captured_fill_draws_afresh_on_every_replay():
    P, ids = 96, [0, 1, 1]
    ds, cache = _pair("train", P)
    buf = cache.sampled_buffers(3, 8, sampler="fps")
    np.random.seed(3)
    cache.stage(buf, ids)
    cache.fill(buf)                                                      # warm up, eager
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cache.fill(buf)
    aug = cache._block_views(buf["params_host"], 3)[0].copy()
    shots = []
    for _ in range(2):
        buf["point_indices"].fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        word0 = _word0(buf["sample_words"])
        want = _cache_model("train", P, ids, word0)
        assert np.array_equal(buf["point_indices"].cpu().numpy(), want)
        assert _same_bits(buf["points"], _specified_points(cache, ids, want, aug))
        shots.append((word0, buf["point_indices"].clone()))
    assert shots[0][0] != shots[1][0] and not torch.equal(shots[0][1], shots[1][1])
