"""Packed batches in the capacity form on the GPU: the device-built chunk table against the host's, its clamping, the
segmented pools on it, PointCloudToWireframe.forward_packed(capacity=) with device counts against host counts, the golden
file and the fp64 oracle, and one graph capture replayed on batches of other point counts.  Helpers and tolerances are
those of tests/test_packed_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402
import test_packed_gpu as TP  # noqa: E402
from test_packed_gpu import OUT_KEYS, TOL, TOL_OUT, dev, mode, ops  # noqa: E402,F401

ODD = [255, 256, 257, 1, 513]


def _table(lay):
    return (lay.d_rows.cpu().numpy(), lay.d_cchunk.cpu().numpy(), lay.d_chunks.cpu().numpy().reshape(-1, 4))


def _assert_equals_host(d, host):
    rows, cchunk, chunks = _table(d)
    assert np.array_equal(rows, host.offsets) and np.array_equal(cchunk, host.chunk_offsets)
    assert chunks.shape == host.chunks.shape and np.array_equal(chunks, host.chunks)
    assert (d.chunk_rows, d.nchunk, d.nchunk_bwd, d.M_pad) == (host.chunk_rows, host.nchunk, host.nchunk_bwd, host.M_pad)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the builder equals the host
# ---------------------------------------------------------------------------------------------------------------------
BUILD_CASES = [(ODD, 1536, [1, 1, 1, 1, 1]), (ODD, 2048, [513, 1, 2, 256, 255]), ([256, 512, 768], 1536, [1, 2, 3]),
               ([300], 512, [512]), ([14039, 1276, 64], 3 * 14080, [1276, 1276, 1276]), ([4096] * 32, 131072, [1] * 32),
               ([1 + (7 * i) % 23 for i in range(700)], 16384, [1] * 700)]          # more clouds than threads


@pytest.mark.parametrize("counts,capacity,shorter", BUILD_CASES, ids=lambda v: None)
def test_builder_equals_host_table(ops, counts, capacity, shorter):
    d = ops.DevicePackedLayout(len(counts), capacity, dev())
    for dtype in (torch.int64, torch.int32):
        for c in (counts, shorter):                  # the second build reuses the buffers with fewer live rows
            d.d_rows.fill_(-7), d.d_cchunk.fill_(-7), d.d_chunks.fill_(-7), d.status.fill_(-7)
            d.build(torch.tensor(c, dtype=dtype, device=dev()))
            _assert_equals_host(d, ops.PackedLayout(c, capacity=capacity))
            assert d.status.tolist() == [0]
    d.build(torch.tensor(counts, device=dev()))      # without the fill: nothing stale survives a longer list either
    _assert_equals_host(d, ops.PackedLayout(counts, capacity=capacity))


# ---------------------------------------------------------------------------------------------------------------------
# 2. clamping, and a cloud of no rows
# ---------------------------------------------------------------------------------------------------------------------
def _check_tiles(d):
    """what every table holds, clamped or not: chunks tile 0 .. capacity once, cloud chunks lie inside their clouds"""
    rows, cchunk, chunks = _table(d)
    live = chunks[chunks[:, 3] > chunks[:, 2]]
    assert live[0, 2] == 0 and live[-1, 3] == d.capacity and np.array_equal(live[1:, 2], live[:-1, 3])
    assert np.all(chunks[:, 3] - chunks[:, 2] <= d.chunk_rows) and np.all(chunks[:, 3] >= chunks[:, 2])
    assert np.all(chunks[cchunk[-1]:, 0] == -1) and np.all(chunks[:cchunk[-1], 0] >= 0)
    for b in range(d.B):
        mine = chunks[cchunk[b]:cchunk[b + 1]]
        assert np.all(mine[:, 0] == b) and np.all(mine[:, 1] == rows[b])
        assert (len(mine) == 0) == (rows[b] == rows[b + 1])
        assert len(mine) == 0 or (mine[0, 2] == rows[b] and mine[-1, 3] == rows[b + 1])


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_builder_clamps(ops, dtype):
    def build(counts, capacity):
        d = ops.DevicePackedLayout(len(counts), capacity, dev()).build(torch.tensor(counts, dtype=dtype, device=dev()))
        _check_tiles(d)
        return d.d_rows.tolist(), int(d.status)
    assert build([700, 900, 600], 1536) == ([0, 700, 1536, 1536], 3)
    assert build([5, 0, 7], 256) == ([0, 5, 5, 12], 2)
    assert build([5, -3, 7], 256) == ([0, 5, 5, 12], 2)
    assert build([256, 256], 512) == ([0, 256, 512], 0)
    assert build([2000], 1536) == ([0, 1536], 1)
    big = 2 ** 31 - 1 if dtype == torch.int32 else 2 ** 40
    assert build([big, big, 3], 512) == ([0, 512, 512, 512], 3)
    assert build([-big, 9, big], 512) == ([0, 0, 9, 512], 3)


def _model(V=6, seed=0):
    from models.PointCloudToWireframe import PointCloudToWireframe
    torch.manual_seed(seed)
    m = PointCloudToWireframe(8, V).to(dev())
    m.vertex_predictor.ensure_point_pool_proj(1024, dev())
    m.set_dropout(0.0)
    m.train()
    return m


def _grads(m):
    return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def _cot_loss(out, cot, idx=None):
    sel = (lambda t: t) if idx is None else (lambda t: t[idx])
    return sum((sel(out[k])[..., :cot[k].shape[-1]] * cot[k]).sum() for k in cot)


def test_zero_row_cloud_through_the_model(mode_fp32):
    """counts [5, 0, 7] on the device: sample 1 has no rows.  Its outputs are finite (pools of zeros), and with no cotangent
    on it every parameter gradient is that of the two-cloud batch [5, 7]."""
    m = _model()
    g = torch.Generator().manual_seed(1)
    pts = torch.zeros(256, 8)
    pts[:12] = torch.randn(12, 8, generator=g)
    pts = pts.to(dev())
    two = m.forward_packed(pts, [5, 7], torch.tensor([4, 2], device=dev()), capacity=256)
    cot = {k: torch.randn(two[k].shape, generator=g).to(dev()) for k in ("vertices", "existence_probabilities", "edge_probs")}
    _cot_loss(two, cot).backward()
    want = _grads(m)
    assert len(want) == 76
    for counts in ([5, 0, 7], [5, -3, 7]):
        m.zero_grad(set_to_none=True)
        out = m.forward_packed(pts, torch.tensor(counts, device=dev()), torch.tensor([4, 3, 2], device=dev()), capacity=256)
        assert out["point_status"].tolist() == [2]
        for k in OUT_KEYS:
            assert torch.isfinite(out[k]).all(), k
        idx = torch.tensor([0, 2], device=dev())
        for k, (a, b) in H.out_errs({k: out[k][idx][..., :two[k].shape[-1]] for k in OUT_KEYS}, two).items():
            assert a < TOL_OUT and b < TOL_OUT, (k, a, b)
        _cot_loss(out, cot, idx).backward()
        got = _grads(m)
        assert set(got) == set(want)
        errs = {n: H.elem_err(got[n].cpu().numpy(), want[n].cpu().numpy()) for n in want}
        bad = [(n, e) for n, e in errs.items() if not e <= TOL]
        assert not bad, bad
        assert all(torch.isfinite(v).all() for v in got.values())


@pytest.fixture
def mode_fp32():
    from wf3d import config
    old = (config.precision(), config.SPLIT_MIN_ROWS)
    config.set_precision("fp32")
    config.SPLIT_MIN_ROWS = 1
    yield
    config.set_precision(old[0])
    config.SPLIT_MIN_ROWS = old[1]


def test_zero_row_cloud_pools(ops):
    """the values include/wf3d.h states: pools 0, arg -1, cnt 1, nvalid 0; the backward and its column sum skip the cloud"""
    C = 64
    d = ops.DevicePackedLayout(3, 256, dev()).build(torch.tensor([5, 0, 7], device=dev()))
    g = torch.Generator().manual_seed(0)
    pf, valid = torch.randn(256, C, generator=g).to(dev()), torch.ones(256, device=dev())
    po = ops.pool4_seg_fwd(pf, valid, d)
    assert float(po.masked[1].abs().max()) == 0.0 and float(po.unmasked[1].abs().max()) == 0.0
    assert po.arg_m[1].tolist() == [-1] * C and po.arg_u[1].tolist() == [-1] * C
    assert po.cnt.tolist() == [5.0, 1.0, 7.0] and po.nvalid.tolist() == [5.0, 0.0, 7.0]
    cot = torch.randn(3, 4 * C, generator=g).to(dev())
    cots = (cot[:, :C], cot[:, C:2 * C], cot[:, 2 * C:3 * C], cot[:, 3 * C:])
    dpf = ops.pool4_seg_bwd(valid, po.cnt, po.arg_m, po.arg_u, *cots, None, d, C)
    assert torch.isfinite(dpf).all() and float(dpf[12:].abs().max()) == 0.0
    cs = ops.pool4_seg_bwd_colsum(po.nvalid, po.cnt, po.arg_m, po.arg_u, *cots, None, d, C)
    assert H.rel_err(cs.cpu().numpy(), dpf.double().sum(0).cpu().numpy()) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 3. the pools ignore dead entries and stale rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 48, 6])
def test_pools_ignore_dead_entries_and_stale_rows(ops, C):
    cap = 2048
    host = ops.PackedLayout.get(ODD, dev())                         # the plain layout: M_pad 1536, chunk_rows 256
    d = ops.DevicePackedLayout(len(ODD), cap, dev()).build(torch.tensor(ODD, device=dev()))
    assert host.chunk_rows == d.chunk_rows == 256 and host.capacity is None
    M = host.M
    g = torch.Generator().manual_seed(C)
    pf_h = torch.randn(host.M_pad, C, generator=g)
    pf_h[3, :] = pf_h[7, :] = 40.0                                  # ties
    valid_h = (torch.rand(host.M_pad, generator=g) > 0.2).float()
    pf_h[M:], valid_h[M:] = 0.0, 0.0
    direct_h = torch.randn(host.M_pad, C, generator=g)
    cot = torch.randn(len(ODD), 4 * C, generator=g).to(dev())
    cots = (cot[:, :C], cot[:, C:2 * C], cot[:, 2 * C:3 * C], cot[:, 3 * C:])

    def capacity_inputs(fill):
        pf, valid, direct = (torch.full((cap,) + t.shape[1:], fill) for t in (pf_h, valid_h, direct_h))
        pf[:M], valid[:M], direct[:M] = pf_h[:M], valid_h[:M], direct_h[:M]
        return pf.to(dev()), valid.to(dev()), direct.to(dev())

    pf_h, valid_h, direct_h = pf_h.to(dev()), valid_h.to(dev()), direct_h.to(dev())
    want = ops.pool4_seg_fwd(pf_h, valid_h, host)
    for fill in (0.0, 1e30):                                        # pad rows of pf / valid / dpf_direct hold anything
        pf, valid, direct = capacity_inputs(fill)
        po = ops.pool4_seg_fwd(pf, valid, d)
        for f in ("masked", "unmasked", "arg_m", "arg_u", "cnt", "nvalid"):
            assert torch.equal(getattr(po, f), getattr(want, f)), (f, fill)
        for dh, dc in ((None, None), (direct_h, direct)):
            forms = [False] + ([True] if C % 8 == 0 else [])
            for sx8 in forms:
                a = ops.pool4_seg_bwd(valid_h, want.cnt, want.arg_m, want.arg_u, *cots, dh, host, C, sx8=sx8)
                b = ops.pool4_seg_bwd(valid, po.cnt, po.arg_m, po.arg_u, *cots, dc, d, C, sx8=sx8)
                assert b.shape == (cap, C) and torch.equal(b[:M], a[:M]), (fill, sx8)
                assert torch.equal(b[M:].view(torch.int32), torch.zeros(cap - M, C, dtype=torch.int32, device=dev()))
            ca = ops.pool4_seg_bwd_colsum(want.nvalid, want.cnt, want.arg_m, want.arg_u, *cots, dh, host, C)
            cb = ops.pool4_seg_bwd_colsum(po.nvalid, po.cnt, po.arg_m, po.arg_u, *cots, dc, d, C, valid=valid)
            if dh is None:
                assert torch.equal(ca, cb)
            else:
                assert TP.rel(cb, ca) < 1e-5
    # the host table of the same capacity is the same table
    hc = ops.PackedLayout.get(ODD, dev(), cap)
    po = ops.pool4_seg_fwd(pf, valid, hc)
    assert torch.equal(po.masked, want.masked) and torch.equal(po.unmasked, want.unmasked)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the model: device counts equal host counts at the same capacity, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _capacity_batch(pcounts, cap, seed=3, fill=0.0):
    g = torch.Generator().manual_seed(seed)
    pts = torch.full((cap, 8), fill)
    pts[:sum(pcounts)] = torch.randn(sum(pcounts), 8, generator=g)
    return pts.to(dev())


def _loss(o):
    return o["vertices"].sum() + 2 * o["existence_probabilities"].sum() + 3 * o["edge_probs"].sum()


@pytest.mark.parametrize("mode", [("fp32", 1), ("bf16x3", 1), ("bf16x3", None)], indirect=True, ids=lambda m: f"{m[0]}-{m[1]}")
def test_device_counts_equal_host_counts_bitwise(mode):
    """capacity 1536 >= SPLIT_MIN_ROWS: with the default (None) the split GEMM routes run, the TN wgrad included"""
    from wf3d import config
    assert 1536 >= config.SPLIT_MIN_ROWS
    pcounts, cap = [300, 1, 700], 1536
    m = _model()
    pts = _capacity_batch(pcounts, cap)
    tc = torch.tensor([6, 2, 4], device=dev())
    for dtype in (torch.int64, torch.int32):
        res = []
        for counts in (pcounts, torch.tensor(pcounts, dtype=dtype, device=dev())):
            m.zero_grad(set_to_none=True)
            out = m.forward_packed(pts, counts, tc, capacity=cap)
            _loss(out).backward()
            res.append((out, _grads(m)))
        (oh, gh), (od, gd) = res
        assert "point_status" not in oh and od["point_status"].tolist() == [0]
        for k in OUT_KEYS:
            assert torch.equal(oh[k], od[k]), k
        assert oh["edge_indices"] == od["edge_indices"]
        assert set(gh) == set(gd) and len(gh) == 76
        for n in gh:
            assert torch.equal(gh[n], gd[n]), n
    # eval mode, padded edge layout
    m.eval().set_edge_layout("padded")
    with torch.no_grad():
        oh = m.forward_packed(pts, pcounts, capacity=cap)
        od = m.forward_packed(pts, torch.tensor(pcounts, device=dev()), capacity=cap)
    for k in OUT_KEYS + ("edge_counts", "edge_width", "actual_vertex_counts"):
        assert torch.equal(oh[k], od[k]), k
    enc_h = m.encoder.encode_packed(pts, pcounts, capacity=cap)
    enc_d = m.encoder.encode_packed(pts, torch.tensor(pcounts, device=dev()), capacity=cap)
    assert enc_d[1].shape == (cap, 512)                               # point_features: [capacity, C]
    for a, b in zip(enc_h, enc_d):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 5. capacity against the golden file and the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------
def _pad_to(points, cap, fill=0.0):
    out = torch.full((cap, points.shape[1]), fill, device=points.device)
    out[:points.shape[0]] = points
    return out


@pytest.mark.parametrize("mode", TP.FORCED[:2], indirect=True, ids=lambda m: m[0])
def test_capacity_forward_vs_golden(mode):
    gold, model, clouds, points, pcounts, counts, V, seed = TP.build_packed()
    cap = -(-sum(pcounts) // 256) * 256 + 512
    out = model.forward_packed(_pad_to(points, cap), torch.tensor(pcounts, device=dev()), counts.to(dev()), capacity=cap)
    assert out["point_status"].tolist() == [0]
    TP._check_outputs(out, gold, TOL_OUT)
    cot = TP._golden_cotangents(out, seed)
    loss = sum((out[k] * cot[k].to(dev())).sum() for k in cot)
    loss.backward()
    assert abs(loss.item() - float(gold["out.loss"])) < 1e-4 * max(1.0, abs(float(gold["out.loss"])))
    bad = H.check_grad_summaries(gold, [(n, p.grad) for n, p in model.named_parameters()], TP.TOL_GRAD)
    assert not bad, bad


def test_capacity_frozen_gradients_fp32_elementwise(monkeypatch):
    """tests/test_packed_gpu.py::test_frozen_gradients_packed_fp32_elementwise with the batch in a capacity buffer and the
    counts on the device: every element of every parameter gradient against the decision-frozen fp64 oracle.  capacity is
    the plain layout's M_pad (512), which the helper's per-point masks are sliced against."""
    from models.PointCloudToWireframe import PointCloudToWireframe
    plain, calls = PointCloudToWireframe.forward_packed, []

    def with_capacity(self, points, point_counts, target_vertex_counts=None):
        calls.append(1)
        pc = torch.tensor(point_counts, device=points.device)
        return plain(self, _pad_to(points, 512), pc, target_vertex_counts, capacity=512)

    monkeypatch.setattr(PointCloudToWireframe, "forward_packed", with_capacity)
    fwd, errs, seed = TP._run_frozen("fp32", [96, 37, 160], 12, [12, 2, 7], 1, False, 32)
    assert calls
    TP._report("fp32 capacity", fwd, errs, seed)
    for k, (a, b) in fwd.items():
        assert a < TOL and b < TOL, (k, a, b)
    assert len(errs) == 76
    bad = [(n, e) for n, e in errs.items() if not e <= TOL]
    assert not bad, bad


@pytest.mark.parametrize("mode", [("fp32", 1), ("bf16x3", None)], indirect=True, ids=lambda m: m[0])
def test_finite_garbage_in_pad_rows_changes_nothing(mode):
    pcounts, cap = [300, 1, 700], 1536
    m = _model()
    tc = torch.tensor([6, 2, 4], device=dev())
    pc = torch.tensor(pcounts, device=dev())
    res = []
    for fill in (0.0, 1e3):
        m.zero_grad(set_to_none=True)
        out = m.forward_packed(_capacity_batch(pcounts, cap, fill=fill), pc, tc, capacity=cap)
        _loss(out).backward()
        res.append((out, _grads(m)))
    for k in OUT_KEYS:
        assert torch.equal(res[0][0][k], res[1][0][k]), k
    for n in res[0][1]:
        assert torch.equal(res[0][1][n], res[1][1][n]), n
        assert torch.isfinite(res[1][1][n]).all(), n


# ---------------------------------------------------------------------------------------------------------------------
# 6. one capture, many batches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [("bf16x3", None)], indirect=True, ids=lambda m: m[0])
def test_one_capture_replays_batches_of_other_point_counts(mode):
    """forward + backward captured once with counts A, replayed after pack_into with counts B and with a full batch C: each
    replay equals the eager run on host counts at the same capacity bit for bit; no replay reads anything on the host.
    (The optimizer step is not part of this capture: tests/test_graph_step_gpu.py covers the capturable ClipAdam.)"""
    from wf3d.packed import pack_into
    cap, V = 1536, 6
    m = _model(V).set_edge_layout("padded")
    gen = torch.Generator().manual_seed(11)
    batches = {name: [torch.randn(n, 8, generator=gen) for n in c]
               for name, c in (("A", [300, 1, 700]), ("B", [10, 1200, 257]), ("C", [512, 1000, 24]))}
    assert sum(c.shape[0] for c in batches["C"]) == cap
    vcounts = {"A": [6, 2, 4], "B": [3, 6, 5], "C": [2, 2, 6]}
    points = torch.zeros(cap, 8, device=dev())
    counts = torch.zeros(3, dtype=torch.int64, device=dev())
    tcounts = torch.zeros(3, dtype=torch.int64, device=dev())

    def load(name):
        pack_into(points, counts, batches[name])
        tcounts.copy_(torch.tensor(vcounts[name]))

    def step():
        for p in m.parameters():
            p.grad = None
        out = m.forward_packed(points, counts, tcounts, capacity=cap)
        _loss(out).backward()
        return out

    load("A")
    s = torch.cuda.Stream(dev())
    s.wait_stream(torch.cuda.current_stream(dev()))
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream(dev()).wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    assert len(grads) == 76
    keys = OUT_KEYS + ("edge_counts", "edge_width", "actual_vertex_counts")
    got = {}
    for name in ("B", "C", "A", "B"):
        load(name)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                       # a host read of the counts would raise here
        try:
            g.replay()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert out["point_status"].tolist() == [0]
        got[name] = ({k: out[k].clone() for k in keys}, {n: v.clone() for n, v in grads.items()})
    for name in ("A", "B", "C"):                                      # eager, host counts, the same capacity
        load(name)
        m.zero_grad(set_to_none=True)
        for p in m.parameters():
            p.grad = None
        ref = m.forward_packed(points, [c.shape[0] for c in batches[name]], tcounts, capacity=cap)
        _loss(ref).backward()
        for k in keys:
            assert torch.equal(got[name][0][k], ref[k]), (name, k)
        for n, p in m.named_parameters():
            if p.grad is not None:
                assert torch.equal(got[name][1][n], p.grad), (name, n)
    assert not torch.equal(got["A"][0]["vertices"], got["B"][0]["vertices"])
    m.set_edge_layout("ragged")


def test_forward_with_device_counts_reads_nothing_back():
    """eager too: device point counts, device target counts and the padded edge layout issue no device -> host read"""
    m = _model().set_edge_layout("padded")
    pts = _capacity_batch([300, 1, 700], 1536)
    tc = torch.tensor([6, 2, 4], device=dev())
    pc = torch.tensor([300, 1, 700], device=dev())
    m.forward_packed(pts, pc, tc, capacity=1536)                      # warm-up: lazily created state of the other stages
    pc2 = torch.tensor([10, 1200, 257], dtype=torch.int32, device=dev())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = m.forward_packed(pts, pc2, tc, capacity=1536)
        _loss(out).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert out["point_status"].tolist() == [0]


# ---------------------------------------------------------------------------------------------------------------------
# 7. existing behaviour, and host-side errors
# ---------------------------------------------------------------------------------------------------------------------
def test_without_capacity_nothing_changed(ops):
    from wf3d import config
    from wf3d.functional import EncoderFnPacked, FusionFn
    m, x, pcounts, c = TP._small()
    with torch.no_grad():
        out = m.forward_packed(x, pcounts, c)
        old = ops.PackedLayout(pcounts).to(dev())                     # built the old way: no capacity, one pad chunk
        assert old.capacity is None and old.nchunk_bwd == old.nchunk + 1 and old.M_pad == 512 and old.M_abi == old.M == 471
        assert old.chunks[-1].tolist() == [-1, 0, 471, 512]
        enc = m.encoder
        pooled, pf, up = EncoderFnPacked.apply(x, old, enc._n_hidden, config.precision(), *enc._mlp_params())
        assert pf.shape[0] == 471
        assert torch.equal(FusionFn.apply(pooled, *enc._fusion_params()), out["global_features"])
        assert torch.equal(m.vertex_predictor.predict(out["global_features"], up)["vertices"], out["vertices"])
    assert "point_status" not in out
    # a CUDA count tensor without capacity: read once, then served from the cache while it is unmodified
    pc = torch.tensor(pcounts, device=dev())
    first = m.forward_packed(x, pc, c)
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = m.forward_packed(x, pc, c)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first["vertices"], again["vertices"]) and torch.equal(first["vertices"], out["vertices"])
    with pytest.raises(RuntimeError, match="host values"):
        m.encoder.encode_packed(x, pc)                                # the encoder alone never reads a device tensor


def test_capacity_errors_are_raised_on_the_host():
    m = _model()
    pts = _capacity_batch([300, 1, 700], 1536)
    tc = torch.tensor([6, 2, 4], device=dev())
    pc = torch.tensor([300, 1, 700], device=dev())
    with pytest.raises(ValueError, match="multiple of 256"):
        m.forward_packed(pts[:1500], pc, tc, capacity=1500)
    with pytest.raises(ValueError, match="must have 1792 rows"):
        m.forward_packed(pts, pc, tc, capacity=1792)
    with pytest.raises(ValueError, match="int64 or int32"):
        m.forward_packed(pts, pc.float(), tc, capacity=1536)
    with pytest.raises(ValueError, match="int64 or int32"):
        m.forward_packed(pts, pc.view(1, 3), tc, capacity=1536)
    with pytest.raises(ValueError, match="above the capacity"):
        m.forward_packed(pts, [300, 1, 1300], tc, capacity=1536)
    with pytest.raises(RuntimeError, match="requires grad"):
        m.forward_packed(pts.clone().requires_grad_(), pc, tc, capacity=1536)
    with pytest.raises(ValueError, match="contiguous"):
        m.forward_packed(torch.randn(8, 1536, device=dev()).t(), pc, tc, capacity=1536)
