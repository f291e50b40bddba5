"""DeviceCloudCache's packed form on the GPU — packed_batch, and stage + fill into the static buffers of a captured step —
against the project's host pipeline on the fixture clouds of tests/golden/building3d: Building3DReconstructionDataset with
num_points = 0, collate_packed and wf3d.targets.train_targets, which tests/test_dataset.py holds to the reference's fixtures.

Floats within that file's 1e-6 for device batches against host batches, for the same cause (fp64 sums of the normalisation in
another order, the rotation written out instead of np.dot; one rounding to fp32 on both sides); integers, labels, existence
and every zero exact."""
import functools
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402

ROOT = os.path.join(H.GOLDEN, "building3d")
TOL = 1e-6
TARGET_KEYS = ("vertices", "vertex_existence", "edge_labels", "vertex_counts")


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _pair(augment, use_color=True, use_intensity=True):
    """(host data set with num_points = 0, the cache built from it)"""
    from datasets import Building3DReconstructionDataset, DeviceCloudCache
    cfg = types.SimpleNamespace(root_dir=ROOT, num_points=0, use_color=use_color, use_intensity=use_intensity, normalize=True,
                                augment=augment)
    ds = Building3DReconstructionDataset(cfg, split_set="train")
    return ds, DeviceCloudCache(ds, dev())


def _host(ds, seed, idxs):
    np.random.seed(seed)
    return ds.collate_packed([ds[i] for i in idxs])


def _check_host_fields(got, want, keys):
    for k in keys:
        if isinstance(want[k], list):
            assert len(got[k]) == len(want[k]), k
            for a, b in zip(got[k], want[k]):
                assert a.dtype == b.dtype and a.shape == b.shape and float((a - b).abs().max()) < TOL, k
        else:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            assert np.allclose(got[k].numpy(), want[k].numpy(), rtol=0, atol=TOL), k


def _poisoned(cache, B, capacity, V):
    buf = cache.packed_buffers(B, capacity, V)
    for k, t in buf.items():
        if torch.is_tensor(t) and k != "params_host":
            t.fill_(7.0 if t.dtype.is_floating_point else (249 if t.dtype == torch.uint8 else -7))
    return buf


def _snapshot(buf):
    torch.cuda.synchronize()
    return {k: t.clone() for k, t in buf.items() if torch.is_tensor(t)}


def _check_points(buf, want, capacity):
    pts, total = buf["points"].cpu(), want["point_clouds"].shape[0]
    assert pts.shape == (capacity, want["point_clouds"].shape[1]) and pts.dtype == torch.float32
    err = float((pts[:total] - want["point_clouds"]).abs().max())
    print(f"points: {total} rows of {capacity}, max |device - host| = {err:.3e}")
    assert err < TOL                                                  # every row of every cloud: both sides of each boundary
    assert torch.equal(pts[total:].view(torch.int32), torch.zeros(capacity - total, pts.shape[1], dtype=torch.int32))
    assert buf["point_counts"].dtype == torch.int64 and torch.equal(buf["point_counts"].cpu(), want["point_counts"])


# ---------------------------------------------------------------------------------------------------------------------
# 1. packed_batch against the host
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("augment", [False, True])
def test_packed_batch_equals_host_collate_packed(augment):
    ds, cache = _pair(augment)
    with pytest.raises(ValueError, match=r"DeviceCloudCache needs dataset.num_points \(fixed-size batches\)"):
        cache.batch([0])                                              # the fixed-size form keeps its refusal
    for seed, idxs in ((5, [0, 1]), (6, [1, 1, 0])):
        want = _host(ds, seed, idxs)
        np.random.seed(seed)
        got = cache.packed_batch(idxs)
        after_device = np.random.random()
        _host(ds, seed, idxs)
        assert np.random.random() == after_device                     # np.random consumed as the host items consume it
        assert set(got) == set(want)
        pc = got["point_clouds"]
        assert pc.is_cuda and pc.dtype == torch.float32 and tuple(pc.shape) == (int(want["point_counts"].sum()), 8)
        assert float((pc.cpu() - want["point_clouds"]).abs().max()) < TOL
        assert got["point_counts"].dtype == torch.int64 and torch.equal(got["point_counts"], want["point_counts"])
        _check_host_fields(got, want, [k for k in want if k not in ("point_clouds", "point_counts")])
    # forward_packed takes the batch as is
    from models.PointCloudToWireframe import PointCloudToWireframe
    model = PointCloudToWireframe(8, 16).to(dev()).train()
    out = model.forward_packed(got["point_clouds"], got["point_counts"], torch.tensor([len(v) for v in got["wf_vertices"]]))
    assert torch.isfinite(out["vertices"]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. + 3. stage + fill into poisoned buffers: points, counts and targets
# ---------------------------------------------------------------------------------------------------------------------
def _check_targets(buf, want, V):
    from wf3d.targets import train_targets
    ref = train_targets(want["wf_vertices"], want["wf_edges"], V, full_width=True)
    for k in ("vertex_existence", "edge_labels", "vertex_counts"):
        got = buf[k].cpu()
        assert got.dtype == ref[k].dtype and got.shape == ref[k].shape and torch.equal(got, ref[k]), k
    assert float(ref["edge_labels"].sum()) == sum(len(e) for e in want["wf_edges"])          # the fixtures' edges are all valid pairs
    got = buf["vertices"].cpu()
    assert got.shape == ref["vertices"].shape
    err = float((got - ref["vertices"]).abs().max())
    print(f"target vertices: max |device - host| = {err:.3e}")
    assert err < TOL
    for s, c in enumerate(ref["vertex_counts"].tolist()):
        assert torch.equal(got[s, c:].view(torch.int32), torch.zeros(V - c, 3, dtype=torch.int32))


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("idxs,capacity,V", [([0, 1, 1, 0, 1], 7168, 8), ([0, 1, 1, 0, 1], 7168, 16), ([0, 1], 2816, 8)], ids=str)
def test_stage_and_fill_overwrite_poisoned_buffers(augment, idxs, capacity, V):
    ds, cache = _pair(augment)
    want = _host(ds, 21, idxs)
    assert capacity != 2816 or capacity - want["point_clouds"].shape[0] == 36          # a zero tail shorter than a workgroup's rows
    buf = _poisoned(cache, len(idxs), capacity, V)
    np.random.seed(21)
    info = cache.stage(buf, idxs)
    cache.fill(buf)
    assert set(info) == {"scan_idx", "centroid", "max_distance"}
    _check_host_fields(info, want, info)
    _check_points(buf, want, capacity)
    _check_targets(buf, want, V)
    assert buf["params"].numel() == len(idxs) * (4 + 4 + 32) + 4 and buf["params_host"].is_pinned()
    assert torch.equal(buf["params"].cpu(), buf["params_host"])


# ---------------------------------------------------------------------------------------------------------------------
# 4. column modes: the generic path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_color,C", [(False, 3), (True, 7)])
def test_column_modes(use_color, C):
    ds, cache = _pair(True, use_color, False)
    idxs, capacity = [0, 1, 1, 0, 1], 7168
    want = _host(ds, 22, idxs)
    assert want["point_clouds"].shape[1] == C
    buf = _poisoned(cache, len(idxs), capacity, 8)
    np.random.seed(22)
    cache.stage(buf, idxs)
    cache.fill(buf)
    _check_points(buf, want, capacity)
    _check_targets(buf, want, 8)
    np.random.seed(22)
    got = cache.packed_batch(idxs)
    assert tuple(got["point_clouds"].shape) == tuple(want["point_clouds"].shape)
    assert float((got["point_clouds"].cpu() - want["point_clouds"]).abs().max()) < TOL


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals leave the buffers as they were
# ---------------------------------------------------------------------------------------------------------------------
def test_stage_refusals_touch_nothing():
    ds, cache = _pair(True)
    big = [os.path.basename(f) for f in ds.pc_files].index("100.xyz")              # 8 vertices
    cases = [(_poisoned(cache, 2, 2560, 8), [0, 1], ValueError, "hold 2780 points, above the capacity of 2560 rows"),
             (_poisoned(cache, 1, 2560, 4), [big], ValueError, "a wireframe has 8 vertices, more than max_vertices = 4"),
             (_poisoned(cache, 2, 2816, 8), [0, 2], IndexError, "index out of range for 2 clouds"),
             (_poisoned(cache, 2, 2816, 8), [0], ValueError, "1 clouds for buffers of 2")]
    for buf, idxs, exc, msg in cases:
        buf["params_host"].fill_(3)
        before = _snapshot(buf)
        np.random.seed(1)
        with pytest.raises(exc, match=msg):
            cache.stage(buf, idxs)
        assert np.random.random() == np.random.RandomState(1).random_sample()         # nothing drawn
        after = _snapshot(buf)
        assert set(before) == set(after) and all(torch.equal(before[k], after[k]) for k in before)
    with pytest.raises(ValueError, match="multiple of 256"):
        cache.packed_buffers(2, 2780, 8)


# ---------------------------------------------------------------------------------------------------------------------
# 6. one capture: fill + step, replayed on a batch staged after the capture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,idxs,first", [(5, [0, 1], [1, 1]), (6, [1, 1, 0], [0, 0, 1])], ids=str)
def test_one_capture_of_fill_and_step(seed, idxs, first):
    """fill + forward_packed + loss + backward captured once on batch `first`; then stage `idxs` (outside) and replay.  Loss
    and every parameter gradient equal the eager run of the same calls on the same staged block bit for bit.  A capture
    holds one B, so each of the two index lists gets the capture of its own B.  Dropout is off, as in the other
    capture-against-eager tests: the two runs then need no common mask seeds."""
    from losses.WireframeLoss import WireframeLoss
    from models.PointCloudToWireframe import PointCloudToWireframe
    ds, cache = _pair(True)
    cap, V = 4352, 16
    torch.manual_seed(0)
    m = PointCloudToWireframe(8, V).to(dev())
    m.set_dropout(0.0)
    m.train().set_edge_layout("padded")
    crit = WireframeLoss(vertex_weight=3.0, edge_weight=1.0, existence_weight=1.5, assignment="device")
    buf = cache.packed_buffers(len(idxs), cap, V)
    held = {}

    def step():
        for p in m.parameters():
            p.grad = None
        cache.fill(buf)
        out = m.forward_packed(buf["points"], buf["point_counts"], buf["vertex_counts"], capacity=cap)
        res = crit(out, {k: buf[k] for k in TARGET_KEYS})
        res["total_loss"].backward()
        held["loss"], held["status"] = res["total_loss"], out["point_status"]

    np.random.seed(4)
    cache.stage(buf, first)
    s = torch.cuda.Stream(dev())
    s.wait_stream(torch.cuda.current_stream(dev()))
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream(dev()).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    assert len(grads) == 76
    graph.replay()
    torch.cuda.synchronize()
    loss_first = held["loss"].clone()

    want = _host(ds, seed, idxs)
    np.random.seed(seed)
    cache.stage(buf, idxs)
    graph.replay()
    torch.cuda.synchronize()
    assert held["status"].tolist() == [0]
    _check_points(buf, want, cap)
    got_loss, got = held["loss"].clone(), {n: g.clone() for n, g in grads.items()}
    assert torch.isfinite(got_loss).all() and not torch.equal(got_loss, loss_first)
    step()                                               # eager, on the same staged block
    torch.cuda.synchronize()
    assert held["status"].tolist() == [0]
    assert torch.equal(got_loss, held["loss"]), (float(got_loss), float(held["loss"]))
    for n, p in m.named_parameters():
        if p.grad is not None:
            assert torch.equal(got[n], p.grad), n
    m.set_edge_layout("ragged")
