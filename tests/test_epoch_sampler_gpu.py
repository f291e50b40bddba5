"""Resident epochs on the GPU: wf3d_cloud_epoch_params against its specification (wf3d.sampling.epoch_batch) byte for
byte, and DeviceCloudCache.fill_epoch / EpochSampler against the EXISTING kernels run on a block the host built from that
specification — every buffer tensor bit for bit — eagerly and under one capture replayed across epochs.

Clouds: the tiny data set of tests/test_cloud_sampler_gpu.py (1, 2, 5, 16, 17, 64, 65 and 300 rows, 4-vertex wireframes) and
the fixture clouds of tests/golden/building3d.  A member table may name a cloud more than once, so D (the members) is
independent of the resident clouds."""
import functools
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402

GOLDEN_ROOT = os.path.join(H.GOLDEN, "building3d")
TINY_ROWS = (1, 2, 5, 16, 17, 64, 65, 300)
TENSOR_KEYS = ("points", "point_counts", "vertices", "vertex_existence", "edge_labels", "vertex_counts", "params", "sample_words")
COLUMNS = {8: dict(use_color=True, use_intensity=True), 3: dict(use_color=False, use_intensity=False)}
KEY = 0xC0FFEE1234567891                                              # bit 63 set: the state holds it as a negative int64
T_BIG = (1 << 33) + 1


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tiny_root(tmp_path_factory):
    from datasets.building3d import save_wireframe
    root = tmp_path_factory.mktemp("tiny_building3d_epochs")
    os.makedirs(root / "train" / "xyz")
    os.makedirs(root / "train" / "wireframe")
    rng = np.random.RandomState(11)
    for k, rows in enumerate(TINY_ROWS):
        cloud = np.concatenate([rng.uniform(-1.0, 1.0, (rows, 3)), rng.randint(0, 256, (rows, 4)).astype(np.float64),
                                rng.uniform(0.0, 1.0, (rows, 1))], axis=1)
        np.savetxt(root / "train" / "xyz" / f"{k + 1}.xyz", cloud, fmt="%.17g")
        save_wireframe(rng.uniform(-1.0, 1.0, (4, 3)), [(0, 1), (1, 2), (2, 3), (0, 3)], str(root / "train" / "wireframe" / f"{k + 1}.obj"))
    return str(root)


@functools.lru_cache(maxsize=None)
def _cache(root, P, C, augment):
    from datasets import Building3DReconstructionDataset, DeviceCloudCache
    cfg = types.SimpleNamespace(root_dir=root, num_points=P, normalize=root == GOLDEN_ROOT, augment=augment, **COLUMNS[C])
    torch.manual_seed(7)
    return DeviceCloudCache(Building3DReconstructionDataset(cfg, split_set="train"), dev())


def _as_int64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= 1 << 63 else x


def _poisoned(buf):
    for k, t in buf.items():
        if torch.is_tensor(t) and k != "params_host":
            t.fill_(7.0 if t.dtype.is_floating_point else (249 if t.dtype == torch.uint8 else -7))
    return buf


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _spec_block(key, t, members, rows, B, W, r, P, augment):
    """(the bytes of the parameter block of include/wf3d.h, the five seed words) of batch t, from the specification alone"""
    from wf3d.sampling import epoch_batch
    spec = epoch_batch(key, t, len(members), B, W, r, augment)
    cloud = np.asarray(members, dtype=np.int32)[spec["order"]]
    if P:
        out_first = np.arange(B + 1, dtype=np.int64) * P
    else:
        out_first = np.concatenate([[0], np.cumsum([rows[i] if 0 <= i < len(rows) else 0 for i in cloud])])
    return spec["aug"].tobytes() + cloud.tobytes() + out_first.astype(np.int32).tobytes(), spec["seed_words"]


def _targets(cache, buf):
    from wf3d import _lib
    from wf3d.ops import _stream
    B, V = buf["vertices"].shape[0], buf["vertices"].shape[1]
    _lib.check(_lib.load().wf3d_wireframe_targets(
        cache.wf_vertices.data_ptr(), cache.wf_edges.data_ptr(), cache.vfirst.data_ptr(), cache.efirst.data_ptr(), len(cache.n),
        buf["params"].data_ptr(), B, V, buf["vertices"].data_ptr(), buf["vertex_existence"].data_ptr(),
        buf["vertex_counts"].data_ptr(), buf["edge_labels"].data_ptr(), _stream()), "wireframe_targets")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the params kernel alone
# ---------------------------------------------------------------------------------------------------------------------
# every (D, B, W) of D in {1, 5, 64, 65, 1000}, B in {1, 3, 64, 4096}, W in {1, 2, 3} with W * B <= D, and — B = 4096 fits none
# of those D — the smallest D that holds W batches of 4096 and leaves a dropped tail
SHAPES = [(D, B, W) for D in (1, 5, 64, 65, 1000) for B in (1, 3, 64) for W in (1, 2, 3) if W * B <= D]
SHAPES += [(4097, 4096, 1), (8200, 4096, 2), (12300, 4096, 3)]


@pytest.mark.parametrize("D,B,W", SHAPES)
def test_params_kernel_is_the_specification(tiny_root, D, B, W):
    from wf3d import _lib
    from wf3d.ops import _stream
    lib = _lib.load()
    cache = _cache(tiny_root, 7, 8, True)
    members = np.random.RandomState(D + B).randint(0, len(cache.n), D).astype(np.int32)
    members_dev = torch.from_numpy(members).to(dev())
    S = D // (W * B)
    params = torch.empty(40 * B + 4, dtype=torch.uint8, device=dev())
    words = torch.empty(5, dtype=torch.int32, device=dev())
    ranks = sorted({0, W - 1})
    for t in sorted({0, S - 1, S, 3 * S + S // 2, T_BIG}):             # both sides of an epoch boundary; t past 2^33
        for r in ranks:
            for P, augment in ((0, 1), (7, 1), (0, 0), (7, 0)) if t in (S, T_BIG) else ((0, 1), (7, 1)):
                params.fill_(249)
                words.fill_(-7)
                state = torch.tensor([_as_int64(KEY), _as_int64(t)], dtype=torch.int64, device=dev())
                _lib.check(lib.wf3d_cloud_epoch_params(state.data_ptr(), members_dev.data_ptr(), D, cache.first.data_ptr(), len(cache.n),
                                                       B, W, r, P, augment, params.data_ptr(), words.data_ptr(), _stream()), "epoch_params")
                want_block, want_words = _spec_block(KEY, t, members, cache.n, B, W, r, P, bool(augment))
                case = (t, r, P, augment)
                assert state.tolist() == [_as_int64(KEY), _as_int64(t + 1)], case
                assert params.cpu().numpy().tobytes() == want_block, case
                assert words.cpu().numpy().view(np.uint32).tolist() == want_words.tolist(), case


def test_params_kernel_argument_checks(tiny_root):
    from wf3d import _lib
    lib = _lib.load()
    cache = _cache(tiny_root, 7, 8, True)
    members = torch.arange(8, dtype=torch.int32, device=dev())
    state = torch.tensor([5, 3], dtype=torch.int64, device=dev())
    params = torch.full((40 * 4 + 4 + 8,), 249, dtype=torch.uint8, device=dev())
    words = torch.full((6,), -7, dtype=torch.int32, device=dev())
    args = dict(state=state.data_ptr(), members=members.data_ptr(), D=8, first=cache.first.data_ptr(), nclouds=8, B=4, world=2,
                rank=1, P=7, augment=1, params=params.data_ptr(), words=words.data_ptr())

    def code(**kw):
        a = dict(args, **kw)
        return lib.wf3d_cloud_epoch_params(a["state"], a["members"], a["D"], a["first"], a["nclouds"], a["B"], a["world"], a["rank"],
                                           a["P"], a["augment"], a["params"], a["words"], None)
    for kw in (dict(D=0), dict(B=0), dict(world=0), dict(rank=2), dict(rank=-1), dict(P=-1), dict(augment=2), dict(nclouds=0),
               dict(B=5), dict(world=3), dict(D=7), dict(B=4096, D=8192, P=1 << 19), dict(state=None), dict(members=None),
               dict(first=None), dict(params=None), dict(words=None), dict(params=args["params"] + 4),
               dict(state=args["state"] + 4), dict(words=args["words"] + 2)):
        assert code(**kw) == _lib.DEFINES["WF3D_ERR_ARG"], kw
        assert b"wf3d_cloud_epoch_params" in lib.wf3d_last_error()
    assert code(B=4097, D=1 << 20) == _lib.DEFINES["WF3D_ERR_UNSUPPORTED"] and b"B > 4096" in lib.wf3d_last_error()
    torch.cuda.synchronize()
    assert state.tolist() == [5, 3] and bool((params == 249).all()) and bool((words == -7).all())      # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------
# 2. the sampler's state
# ---------------------------------------------------------------------------------------------------------------------
def _read_block(cache, buf):
    """(aug, cloud, out_first) of the block on the device"""
    return tuple(v.copy() for v in cache._block_views(buf["params"].cpu(), buf["vertices"].shape[0]))


def test_state_advances_and_seeks(tiny_root):
    cache = _cache(tiny_root, 7, 8, True)
    sampler = cache.epoch_sampler(3, seed=KEY)
    assert sampler.steps_per_epoch == 2 and sampler.state.is_cuda and sampler.state.dtype == torch.int64
    assert sampler.get_state().tolist() == [_as_int64(KEY), 0]
    buf = _poisoned(cache.sampled_buffers(3, 8))
    shots = []
    for t in range(5):
        cache.fill_epoch(buf, sampler)
        assert sampler.get_state().tolist() == [_as_int64(KEY), t + 1]
        aug, cloud, first = _read_block(cache, buf)
        spec = sampler.batch_at(t)
        assert cloud.tolist() == spec["cloud"].tolist() and aug.tobytes() == spec["aug"].tobytes() and first.tolist() == [0, 7, 14, 21]
        assert buf["sample_words"].cpu().numpy().view(np.uint32).tolist() == spec["seed_words"].tolist()
        shots.append({k: buf[k].clone() for k in TENSOR_KEYS if k in buf})
    saved = sampler.get_state()
    sampler.set_state(torch.tensor([_as_int64(KEY), 2]))
    cache.fill_epoch(buf, sampler)
    assert all(_same_bits(buf[k], shots[2][k]) for k in shots[2]) and int(sampler.get_state()[1]) == 3
    sampler.seek(2, 0)                                                # epoch 2, step 0: t = 4
    cache.fill_epoch(buf, sampler)
    assert all(_same_bits(buf[k], shots[4][k]) for k in shots[4])
    sampler.seek(0, 1)
    cache.fill_epoch(buf, sampler)
    assert all(_same_bits(buf[k], shots[1][k]) for k in shots[1])
    sampler.set_state(saved)
    assert sampler.get_state().tolist() == [_as_int64(KEY), 5]
    # another key through set_state: batch_at follows it
    sampler.set_state(torch.tensor([99, T_BIG]))
    cache.fill_epoch(buf, sampler)
    assert sampler.key == 99 and _read_block(cache, buf)[1].tolist() == sampler.batch_at(T_BIG)["cloud"].tolist()
    with pytest.raises(ValueError, match="0 <= step < 2"):
        sampler.seek(0, 2)
    with pytest.raises(ValueError, match=r"\[key, t\]"):
        sampler.set_state(torch.zeros(3, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------------------------------
# 3. fill_epoch against the existing kernels on a block the host built
# ---------------------------------------------------------------------------------------------------------------------
def _host_built(cache, sampler, buf, t):
    """the spec's block and seed words copied into `buf`, then the existing launches"""
    sampled = "sample_words" in buf
    buf["params"].copy_(sampler.block_at(t, buf["points"].shape[1] if sampled else 0))
    if sampled:
        buf["sample_words"].copy_(torch.from_numpy(sampler.batch_at(t)["seed_words"].view(np.int32)))
        cache._sample(buf["params"], buf["sample_words"], buf["points"])
        _targets(cache, buf)
    else:
        cache.fill(buf)


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("form,C,P", [("sampled", 8, 7), ("sampled", 8, 300), ("sampled", 3, 64), ("packed", 8, 7), ("packed", 3, 7)])
def test_fill_epoch_is_the_existing_kernels_on_the_specified_block(tiny_root, form, C, P, augment):
    cases = [(tiny_root, 3, [7, 0, 3, 3, 1, 6, 2, 5, 4, 0, 7], 2, 1), (tiny_root, 8, None, 1, 0), (GOLDEN_ROOT, 1, None, 1, 0),
             (GOLDEN_ROOT, 2, [1, 0, 1, 1, 0], 1, 0)]
    for root, B, members, W, r in cases:
        cache = _cache(root, P, C, augment)
        sampler = cache.epoch_sampler(B, members, world=W, rank=r, seed=KEY + B)
        rows = sorted(cache.n[i] for i in (members if members is not None else range(len(cache.n))))
        make = (lambda: cache.sampled_buffers(B, 8)) if form == "sampled" else (lambda: cache.packed_buffers(B, 256 * (sum(rows[-B:]) // 256 + 1), 8))
        got, want = _poisoned(make()), _poisoned(make())
        S = sampler.steps_per_epoch
        for t in (0, S - 1, S, 2 * S + 1):
            sampler.seek(t // S, t % S)
            cache.fill_epoch(got, sampler)
            _host_built(cache, sampler, want, t)
            for k in TENSOR_KEYS:
                if k in got:
                    assert _same_bits(got[k], want[k]), (root == GOLDEN_ROOT, B, t, k)
            assert not bool((got["points"] == 7.0).any()) and not bool((got["vertices"] == 7.0).any())
            if form == "packed":
                assert got["point_counts"].tolist() == [cache.n[i] for i in sampler.batch_at(t)["cloud"]]
                assert sampler.seed_words.cpu().numpy().view(np.uint32).tolist() == sampler.batch_at(t)["seed_words"].tolist()


# ---------------------------------------------------------------------------------------------------------------------
# 4. one capture, nothing between replays
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sampled", "packed"])
def test_one_capture_walks_the_epochs(tiny_root, form):
    cache = _cache(tiny_root, 7, 8, True)
    B = 4
    sampler = cache.epoch_sampler(B, seed=KEY)
    S = sampler.steps_per_epoch
    assert S == 2
    buf = cache.sampled_buffers(B, 8) if form == "sampled" else cache.packed_buffers(B, 512, 8)
    want = cache.sampled_buffers(B, 8) if form == "sampled" else cache.packed_buffers(B, 512, 8)
    cache.fill_epoch(buf, sampler)                                    # eager once: t = 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cache.fill_epoch(buf, sampler)
    t0 = int(sampler.get_state()[1])
    assert t0 == 1                                                    # a capture runs nothing
    clouds = []
    for i in range(2 * S + 1):
        graph.replay()
        torch.cuda.synchronize()
        cloud = _read_block(cache, buf)[1]
        assert cloud.tolist() == sampler.batch_at(t0 + i)["cloud"].tolist(), i
        clouds.append(cloud.tolist())
        if i in (0, 2 * S):
            _host_built(cache, sampler, want, t0 + i)
            for k in TENSOR_KEYS:
                if k in buf:
                    assert _same_bits(buf[k], want[k]), (i, k)
    assert int(sampler.get_state()[1]) == t0 + 2 * S + 1
    # t = 2, 3 are epoch 1 whole: every member exactly once (W = 1, D % B == 0)
    assert sorted(clouds[1] + clouds[2]) == list(range(8))
    assert sorted(sampler.batch_at(0)["cloud"].tolist() + clouds[0]) == list(range(8))


def test_two_ranks_in_one_process(tiny_root):
    cache = _cache(tiny_root, 7, 8, True)
    B = 2
    ranks = [cache.epoch_sampler(B, world=2, rank=r, seed=31) for r in (0, 1)]
    whole = cache.epoch_sampler(2 * B, seed=31)
    bufs = [cache.sampled_buffers(B, 8) for _ in ranks]
    wbuf = cache.sampled_buffers(2 * B, 8)
    assert ranks[0].steps_per_epoch == whole.steps_per_epoch == 2
    for t in range(5):
        for s, b in zip(ranks, bufs):
            cache.fill_epoch(b, s)
        cache.fill_epoch(wbuf, whole)
        parts = [_read_block(cache, b) for b in bufs]
        waug, wcloud, _ = _read_block(cache, wbuf)
        assert not set(parts[0][1].tolist()) & set(parts[1][1].tolist())
        assert parts[0][1].tolist() + parts[1][1].tolist() == wcloud.tolist()
        assert parts[0][0].tobytes() + parts[1][0].tobytes() == waug.tobytes()
        # the targets depend on the cloud and its augmentation only: the ranks' rows are the single rank's
        for k in ("vertices", "vertex_existence", "edge_labels", "vertex_counts"):
            assert _same_bits(torch.cat([bufs[0][k], bufs[1][k]]), wbuf[k]), (t, k)
        assert int(bufs[0]["sample_words"][0]) != int(bufs[1]["sample_words"][0])


# ---------------------------------------------------------------------------------------------------------------------
# 5. the once-only checks
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(tiny_root):
    tiny = _cache(tiny_root, 7, 8, True)
    fixture = _cache(GOLDEN_ROOT, 64, 8, True)
    most = max(fixture.nv)
    cases = [(tiny, tiny.packed_buffers(2, 256, 8), dict(B=2), ValueError, "the 2 largest member clouds hold 365 points, above the capacity of 256 rows"),
             (fixture, fixture.sampled_buffers(1, most - 1), dict(B=1), ValueError, f"a wireframe has {most} vertices, more than max_vertices = {most - 1}"),
             (fixture, fixture.packed_buffers(1, 4096, most - 1), dict(B=1), ValueError, f"more than max_vertices = {most - 1}"),
             (tiny, tiny.sampled_buffers(2, 8), dict(B=2, members=[0, 1, 8, 2]), IndexError, "member out of range for 8 clouds"),
             (tiny, tiny.sampled_buffers(2, 8), dict(B=2, members=[0, -1, 2]), IndexError, "member out of range for 8 clouds"),
             (tiny, tiny.sampled_buffers(3, 8), dict(B=2), ValueError, "a sampler of 2 clouds per batch for buffers of 3"),
             (fixture, tiny.sampled_buffers(2, 8), dict(B=2), ValueError, "belongs to another cache")]
    for cache, buf, kw, exc, msg in cases:
        sampler = (tiny if "another" in msg else cache).epoch_sampler(seed=3, **kw)
        _poisoned(buf)
        sampler.seed_words.fill_(-7)
        torch.cuda.synchronize()
        before = {k: t.clone() for k, t in buf.items() if torch.is_tensor(t)}
        for _ in range(2):                                            # a refused pair is checked again, and refused again
            with pytest.raises(exc, match=msg):
                cache.fill_epoch(buf, sampler)
        torch.cuda.synchronize()
        assert sampler.get_state().tolist() == [3, 0] and bool((sampler.seed_words == -7).all())
        assert all(torch.equal(before[k], buf[k]) for k in before)
    # the capacity of exactly the B largest members is enough, whatever the other members hold
    sampler = tiny.epoch_sampler(2, members=np.argsort(tiny.n)[:7].tolist(), seed=3)      # all but the cloud of 300 rows
    buf = tiny.packed_buffers(2, 256, 8)                              # 65 + 64 rows
    for _ in range(5):
        tiny.fill_epoch(buf, sampler)
    with pytest.raises(ValueError, match="world > 1 needs an explicit integer seed"):
        tiny.epoch_sampler(2, world=2, rank=1)
    # a sampler allocates its state: not inside a capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tiny.fill_epoch(buf, sampler)
        with pytest.raises(RuntimeError, match="must be created before a graph capture starts"):
            tiny.epoch_sampler(2, seed=3)
