"""The device sampler of DeviceCloudCache on the GPU — batch(sampler="device"), and sampled_buffers / stage / fill into the
static buffers of a captured step — against its specification: the EXISTING gather kernel (wf3d_cloud_sample) fed with
wf3d.sampling.choice_indices under the seed word the device drew, and the same augmentation block.  Both kernels do the
same float64 arithmetic with one rounding, so every comparison of points is bit for bit; so are the targets against
the packed form's fill, and the host fields against collate_batch.

Clouds: a tiny data set of 1, 2, 5, 16, 17, 64, 65 and 300 rows (where the Feistel half-width changes, where the cycle
walk is longest, and n < P), and the fixture clouds of tests/golden/building3d."""
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
TARGET_KEYS = ("vertices", "vertex_existence", "edge_labels", "vertex_counts")
PS = [1, 7, 64, 300]
COLUMNS = {8: dict(use_color=True, use_intensity=True), 3: dict(use_color=False, use_intensity=False)}


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tiny_root(tmp_path_factory):
    """<root>/train/{xyz, wireframe}: clouds of TINY_ROWS rows x 8 columns (building-sized coordinates, colours 0..255), each
    with a 4-vertex wireframe"""
    from datasets.building3d import save_wireframe
    root = tmp_path_factory.mktemp("tiny_building3d")
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
def _pair(root, P, C, augment):
    """(data set with num_points = P, the cache built from it).  The tiny clouds are used as they are (a cloud of one row
    has no max-norm to divide by); the fixture clouds are normalised."""
    from datasets import Building3DReconstructionDataset, DeviceCloudCache
    cfg = types.SimpleNamespace(root_dir=root, num_points=P, normalize=root == GOLDEN_ROOT, augment=augment, **COLUMNS[C])
    ds = Building3DReconstructionDataset(cfg, split_set="train")
    torch.manual_seed(1000 * P + 10 * C + augment)                   # the key of the cache's sample stream: a reproducible run
    return ds, DeviceCloudCache(ds, dev())


def _batches(tiny_root):
    """(root, indices): every tiny cloud, some twice, in no order; the fixture clouds"""
    return [(tiny_root, [7, 0, 3, 3, 1, 6, 2, 5, 4, 0, 7]), (GOLDEN_ROOT, [1, 0, 1])]


def _draw_aug(ds, B):
    """the augmentation draws of a batch of B samples, in the order every form of the cache makes them"""
    from datasets.building3d import rotz
    draws = [ds._draw_augmentation() if ds.augment else (1.0, 1.0, 0.0) for _ in range(B)]
    aug = np.array([(fx, fy, np.cos(t), np.sin(t)) for fx, fy, t in draws], dtype=np.float64).reshape(B, 4)
    return draws, aug, rotz


def _specified_points(cache, idxs, word0, aug, P):
    """the specification: wf3d_cloud_sample (the host-choice kernel) on choice_indices(word0, b, n_b, P)"""
    from wf3d import _lib
    from wf3d.ops import _stream
    from wf3d.sampling import choice_indices
    B = len(idxs)
    choice = np.stack([choice_indices(word0, b, cache.n[i], P) for b, i in enumerate(idxs)])
    for b, i in enumerate(idxs):
        assert 0 <= choice[b].min() and choice[b].max() < cache.n[i]
        assert cache.n[i] < P or len(set(choice[b].tolist())) == P
    ids = torch.tensor(idxs, dtype=torch.int32, device=dev())
    ch = torch.from_numpy(choice.astype(np.int32)).to(dev())
    ag = torch.from_numpy(np.ascontiguousarray(aug)).to(dev())
    out = torch.full((B, P, cache.ncol), 5.0, dtype=torch.float32, device=dev())
    _lib.check(_lib.load().wf3d_cloud_sample(cache.norm.data_ptr(), cache.first.data_ptr(), ids.data_ptr(), ch.data_ptr(),
                                             ag.data_ptr(), B, P, cache.ncol, out.data_ptr(), _stream()), "cloud_sample")
    return out


def _word0(words):
    return int(words[0]) & 0xFFFFFFFF


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same_fields(got, want):
    assert set(got) == set(want)
    for k in want:
        if isinstance(want[k], list):
            assert len(got[k]) == len(want[k]) and all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(got[k], want[k])), k
        else:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


def _poisoned(buf):
    for k, t in buf.items():
        if torch.is_tensor(t) and k != "params_host":
            t.fill_(7.0 if t.dtype.is_floating_point else (249 if t.dtype == torch.uint8 else -7))
    return buf


# ---------------------------------------------------------------------------------------------------------------------
# 1. batch(sampler="device")
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("C", [8, 3])
@pytest.mark.parametrize("P", PS)
def test_device_batch_is_the_specification(tiny_root, P, C, augment):
    for root, idxs in _batches(tiny_root):
        ds, cache = _pair(root, P, C, augment)
        B = len(idxs)
        np.random.seed(31)
        got = cache.batch(idxs, sampler="device")
        after_device = np.random.random()
        words = cache.last_sample_words
        assert words.is_cuda and words.dtype == torch.int32 and tuple(words.shape) == (5,)
        np.random.seed(31)
        draws, aug, rotz = _draw_aug(ds, B)
        assert np.random.random() == after_device                     # the augmentation draws and nothing else: no choice draws
        want = ds.collate_batch([cache._item(i, fx, fy, rotz(t)) for i, (fx, fy, t) in zip(idxs, draws)])
        pc = got.pop("point_clouds")
        _same_fields(got, want)
        assert pc.is_cuda and pc.is_contiguous() and tuple(pc.shape) == (B, P, C)
        assert _same_bits(pc, _specified_points(cache, idxs, _word0(words), aug, P))
        again = cache.batch(idxs, sampler="device")["point_clouds"]   # the next word of the stream
        assert _word0(cache.last_sample_words) != _word0(words)
        assert P * C < 24 or not torch.equal(again, pc)


def test_batch_keywords_and_refusals(tiny_root):
    from datasets import Building3DReconstructionDataset, DeviceCloudCache
    ds, cache = _pair(GOLDEN_ROOT, 64, 8, True)
    with pytest.raises(ValueError, match="sampler must be 'numpy' or 'device'"):
        cache.batch([0], sampler="torch")
    with pytest.raises(IndexError, match="index out of range for 2 clouds"):
        cache.batch([0, 2], sampler="device")
    # the default is the numpy sampler, and it leaves the device stream alone
    state = cache.sample_generator.get_state()
    np.random.seed(8)
    a = cache.batch([0, 1])["point_clouds"]
    np.random.seed(8)
    b = cache.batch([0, 1], sampler="numpy")["point_clouds"]
    assert torch.equal(a, b) and torch.equal(cache.sample_generator.get_state(), state)
    # the cache's stream is not the dropout stream
    from wf3d.random import default_generator
    assert cache.sample_generator is not default_generator(dev())
    assert cache.sample_generator.state.data_ptr() != default_generator(dev()).state.data_ptr()
    # a data set without num_points: batch() keeps its refusal in both forms, sampled_buffers needs a size
    cfg = types.SimpleNamespace(root_dir=GOLDEN_ROOT, num_points=0, normalize=True, augment=False, **COLUMNS[8])
    cache0 = DeviceCloudCache(Building3DReconstructionDataset(cfg, split_set="train"), dev())
    for kw in ({}, {"sampler": "device"}):
        with pytest.raises(ValueError, match=r"DeviceCloudCache needs dataset.num_points \(fixed-size batches\)"):
            cache0.batch([0], **kw)
    with pytest.raises(ValueError, match="needs num_points or dataset.num_points"):
        cache0.sampled_buffers(2, 8)
    assert tuple(cache0.sampled_buffers(2, 8, num_points=40)["points"].shape) == (2, 40, 8)
    assert tuple(cache.sampled_buffers(2, 8)["points"].shape) == (2, 64, 8)
    with pytest.raises(ValueError, match="1 <= B <= 4096"):
        cache.sampled_buffers(4097, 8)


# ---------------------------------------------------------------------------------------------------------------------
# 2. stage + fill into poisoned buffers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("C", [8, 3])
@pytest.mark.parametrize("P", PS)
def test_stage_and_fill_overwrite_poisoned_buffers(tiny_root, P, C, augment):
    for root, idxs in _batches(tiny_root):
        ds, cache = _pair(root, P, C, augment)
        B, V = len(idxs), 8
        buf = _poisoned(cache.sampled_buffers(B, V))
        assert set(buf) == {"points", *TARGET_KEYS, "params", "params_host", "params_copied", "sample_words"}
        assert buf["params_host"].is_pinned() and buf["sample_words"].dtype == torch.int32 and tuple(buf["sample_words"].shape) == (5,)
        np.random.seed(21)
        info = cache.stage(buf, idxs)
        after_stage = np.random.random()
        cache.fill(buf)
        # the packed form of the same batch under the same np.random seed: the same draws, the same targets, the same info
        packed = _poisoned(cache.packed_buffers(B, 256 * ((sum(cache.n[i] for i in idxs) + 255) // 256), V))
        np.random.seed(21)
        info_packed = cache.stage(packed, idxs)
        assert np.random.random() == after_stage
        cache.fill(packed)
        _same_fields(info, info_packed)
        for k in TARGET_KEYS:
            assert _same_bits(buf[k], packed[k]) if buf[k].dtype == torch.float32 else torch.equal(buf[k], packed[k]), k
        assert not bool((buf["vertices"] == 7.0).any()) and not bool((buf["edge_labels"] == 7.0).any())
        # the block: the packed block's aug and cloud, out_first = b * P
        assert torch.equal(buf["params"].cpu(), buf["params_host"])
        v_aug, v_cloud, v_first = cache._block_views(buf["params_host"], B)
        p_aug, p_cloud, _ = cache._block_views(packed["params_host"], B)
        assert np.array_equal(v_aug, p_aug) and np.array_equal(v_cloud, p_cloud) and v_first.tolist() == [b * P for b in range(B + 1)]
        # every element of points, against the specification
        assert tuple(buf["points"].shape) == (B, P, C) and buf["points"].is_contiguous()
        assert _same_bits(buf["points"], _specified_points(cache, idxs, _word0(buf["sample_words"]), v_aug, P))


def test_stage_refusals_touch_nothing():
    ds, cache = _pair(GOLDEN_ROOT, 64, 8, True)
    big = [os.path.basename(f) for f in ds.pc_files].index("100.xyz")              # 8 vertices
    cases = [(cache.sampled_buffers(1, 4), [big], ValueError, "a wireframe has 8 vertices, more than max_vertices = 4"),
             (cache.sampled_buffers(2, 8), [0, 2], IndexError, "index out of range for 2 clouds"),
             (cache.sampled_buffers(2, 8), [0], ValueError, "1 clouds for buffers of 2")]
    for buf, idxs, exc, msg in cases:
        _poisoned(buf)["params_host"].fill_(3)
        torch.cuda.synchronize()
        before = {k: t.clone() for k, t in buf.items() if torch.is_tensor(t)}
        np.random.seed(1)
        with pytest.raises(exc, match=msg):
            cache.stage(buf, idxs)
        assert np.random.random() == np.random.RandomState(1).random_sample()         # nothing drawn
        torch.cuda.synchronize()
        assert all(torch.equal(before[k], buf[k]) for k in before)
    # no row capacity: both fixture clouds (2780 rows) into 2 x 64
    cache.stage(cache.sampled_buffers(2, 8), [0, 1])


def test_blocks_the_host_did_not_build_give_zero_rows(tiny_root):
    """cloud indices outside the resident clouds, written into the block by hand on the device, and (through the entry
    point, with a row-offset table of its own) an empty cloud: those samples are zeros, the others as specified"""
    from wf3d import _lib
    from wf3d.ops import _stream
    for C, P in ((8, 300), (8, 7), (3, 300)):
        ds, cache = _pair(tiny_root, P, C, True)
        idxs, bad = [7, 5, 2, 6, 0], {1: len(cache.n), 3: -1}
        B = len(idxs)
        buf = _poisoned(cache.sampled_buffers(B, 8))
        np.random.seed(2)
        cache.stage(buf, idxs)
        torch.cuda.synchronize()
        cloud = buf["params"][32 * B:36 * B].view(torch.int32)
        for b, value in bad.items():
            cloud[b] = value
        cache.fill(buf)
        torch.cuda.synchronize()
        want = _specified_points(cache, idxs, _word0(buf["sample_words"]), cache._block_views(buf["params_host"], B)[0], P)
        for b in bad:
            want[b] = 0.0
        assert _same_bits(buf["points"], want)
        # cloud 0 empty, cloud 1 = the resident rows of tiny cloud idxs[0]
        lo, n = int(cache.first[idxs[0]]), cache.n[idxs[0]]
        first = torch.tensor([lo, lo, lo + n], dtype=torch.int64, device=dev())
        block = buf["params"].clone()
        block[32 * B:36 * B].view(torch.int32).copy_(torch.tensor([1, 0, 1, 0, 2], dtype=torch.int32))
        out = torch.full((B, P, C), 7.0, dtype=torch.float32, device=dev())
        _lib.check(_lib.load().wf3d_cloud_sample_dev(cache.norm.data_ptr(), first.data_ptr(), 2, block.data_ptr(),
                                                     buf["sample_words"].data_ptr(), B, P, C, out.data_ptr(), _stream()), "cloud_sample_dev")
        assert _same_bits(out[0], want[0])                            # sample 0: the same rows under the same key
        assert not bool((out[2] == 7.0).any()) and bool((out[2] != 0).any())
        for b in (1, 3, 4):
            assert _same_bits(out[b], torch.zeros(P, C, device=dev()))


def test_argument_checks():
    from wf3d import _lib
    lib = _lib.load()
    ds, cache = _pair(GOLDEN_ROOT, 64, 8, True)
    buf = cache.sampled_buffers(2, 8)
    args = dict(norm=cache.norm.data_ptr(), first=cache.first.data_ptr(), nclouds=2, params=buf["params"].data_ptr(),
                words=buf["sample_words"].data_ptr(), B=2, P=64, C=8, points=buf["points"].data_ptr())

    def code(**kw):
        a = dict(args, **kw)
        return lib.wf3d_cloud_sample_dev(a["norm"], a["first"], a["nclouds"], a["params"], a["words"], a["B"], a["P"], a["C"],
                                         a["points"], None)
    for kw in (dict(B=0), dict(B=4097), dict(P=0), dict(C=2), dict(C=17), dict(nclouds=0), dict(B=4096, P=1 << 19),
               dict(words=None), dict(params=None), dict(points=None), dict(params=args["params"] + 4),
               dict(points=args["points"] + 8), dict(norm=args["norm"] + 8)):
        assert code(**kw) == _lib.DEFINES["WF3D_ERR_ARG"], kw
        assert b"wf3d_cloud_sample_dev" in lib.wf3d_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# 3. one capture, fresh samples on every replay
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,P", [(8, 7), (8, 300), (3, 64)])
def test_captured_fill_samples_afresh_and_replays_from_a_saved_state(tiny_root, C, P):
    ds, cache = _pair(tiny_root, P, C, True)
    batches = ([7, 0, 3, 5], [6, 6, 2, 7], [1, 4, 7, 5])
    buf = cache.sampled_buffers(4, 8)
    np.random.seed(3)
    cache.stage(buf, batches[0])
    cache.fill(buf)                                                   # eager once
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cache.fill(buf)
    saved = cache.sample_generator.get_state()

    def run():
        shots = []
        for k, idxs in enumerate(batches):
            np.random.seed(40 + k)
            cache.stage(buf, idxs)
            graph.replay()
            torch.cuda.synchronize()
            aug = cache._block_views(buf["params_host"], 4)[0].copy()
            word0 = _word0(buf["sample_words"])
            assert _same_bits(buf["points"], _specified_points(cache, idxs, word0, aug, P))
            shots.append((word0, buf["points"].clone(), buf["vertices"].clone()))
        return shots

    first = run()
    assert len({w for w, _, _ in first}) == 3
    assert not torch.equal(first[0][1], first[1][1]) and not torch.equal(first[1][1], first[2][1])
    assert int(cache.sample_generator.get_state()[1]) == int(saved[1]) + 3
    cache.sample_generator.set_state(saved)
    for a, b in zip(first, run()):
        assert a[0] == b[0] and _same_bits(a[1], b[1]) and _same_bits(a[2], b[2])
    # the same staged block under another word: other rows, the same augmentation
    np.random.seed(42)
    cache.stage(buf, batches[2])
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(buf["vertices"], first[2][2]) and not torch.equal(buf["points"], first[2][1])


# ---------------------------------------------------------------------------------------------------------------------
# 4. the dense forward takes the buffer as it is
# ---------------------------------------------------------------------------------------------------------------------
def test_dense_forward_takes_the_points_buffer():
    from models.PointCloudToWireframe import PointCloudToWireframe
    ds, cache = _pair(GOLDEN_ROOT, 300, 8, True)
    buf = cache.sampled_buffers(3, 16)
    np.random.seed(9)
    cache.stage(buf, [0, 1, 1])
    cache.fill(buf)
    assert buf["points"].is_contiguous() and buf["points"].dtype == torch.float32 and tuple(buf["points"].shape) == (3, 300, 8)
    torch.manual_seed(0)
    model = PointCloudToWireframe(8, 16).to(dev()).train()
    out = model(buf["points"], buf["vertex_counts"])
    assert all(torch.isfinite(out[k]).all() for k in ("vertices", "existence_probabilities", "edge_probs"))
