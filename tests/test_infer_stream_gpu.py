"""The forward-only encoder (wf3d.infer) on the GPU: its two kernels alone, the block walk against the fp64 oracle on
every route, dense and packed, against the training forward bit for bit where the two must agree, through the whole
model against the goldens, and its memory footprint.

Bounds.  Pools: maxima, cnt and nvalid exact; a mean within n * 2^-23 * mean|x| of the fp64 value, n the rows summed
(twice the standard fp32 summation bound (n - 1) * 2^-24 * sum|x| / n; the numpy model itself is far inside it).
Encoder and model outputs: 1e-4 by H.rel_err and H.elem_err, the bound the project holds its forward to (TOL in
tests/test_encoder_cotangents_gpu.py, TOL_OUT in tests/test_model_gpu.py); bf16: TOL_BF16_FWD of
tests/test_precision_bf16_gpu.py.  Each test prints what it measured (pytest -s)."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import enc_cases as E  # noqa: E402
import helpers as H  # noqa: E402
import infer_model as IM  # noqa: E402

TOL = 1e-4
TOL_BF16_FWD = 1.75e-2
MODEL = [512, 1024, 2048, 1024]


def dev():
    return torch.device("cuda:0")


@contextlib.contextmanager
def mode(precision, split_min_rows=1):
    """Precision and SPLIT_MIN_ROWS for the body, as tests/test_encoder_cotangents_gpu.py::mode."""
    from wf3d import config
    old = (config.precision(), config.SPLIT_MIN_ROWS)
    config.set_precision(precision)
    config.SPLIT_MIN_ROWS = split_min_rows
    try:
        yield
    finally:
        config.set_precision(old[0])
        config.SPLIT_MIN_ROWS = old[1]


@contextlib.contextmanager
def inference(setting, rows=None):
    from wf3d import config
    old = (config.inference(), config.INFER_ROWS)
    config.set_inference(setting)
    if rows is not None:
        config.INFER_ROWS = rows
    try:
        yield
    finally:
        config.set_inference(old[0])
        config.INFER_ROWS = old[1]


# ----------------------------------------------------------------------------------------------------------------------
# 1. the pool kernel alone against the numpy model
# ----------------------------------------------------------------------------------------------------------------------
OFFSETS = [0, 37, 37, 100, 356]             # cloud 1 has no rows, cloud 3 crosses 256 rows
PAD = 20                                    # rows behind offsets[B]
_POOL_REF = {}


def pool_case(C):
    """(pf, valid, fp64 model result, per-cloud mean|x| of the rows each mean sums) — computed once per width."""
    if C not in _POOL_REF:
        rng = np.random.default_rng(C)
        R = OFFSETS[-1] + PAD
        pf = rng.standard_normal((R, C)).astype(np.float32)
        pf[:, 3] = -1.0 - np.abs(pf[:, 3])                  # negative everywhere: a maximum initialised to 0 would be wrong
        pf[:, 7] = 0.75                                     # constant
        valid = np.ones(R, dtype=np.float32)
        valid[[2, 3, 11, 30, 36]] = 0.0                     # scattered zeros in cloud 0
        valid[OFFSETS[2]:OFFSETS[3]] = 0.0                  # cloud 2: no valid row
        pf[OFFSETS[-1]:] = 1e6                              # pad rows: valid, huge — and no cloud's
        ref = IM.stream(OFFSETS, pf.astype(np.float64), valid, [0, R])
        B = len(OFFSETS) - 1
        mabs_u, mabs_m = np.zeros((B, C)), np.zeros((B, C))
        for b in range(B):
            v, m = np.abs(pf[OFFSETS[b]:OFFSETS[b + 1]].astype(np.float64)), valid[OFFSETS[b]:OFFSETS[b + 1]] != 0
            if len(v):
                mabs_u[b] = v.mean(0)
            if m.any():
                mabs_m[b] = v[m].mean(0)
        _POOL_REF[C] = (pf, valid, ref, mabs_u, mabs_m)
    return _POOL_REF[C]


def run_pool(pf_d, valid_d, offsets_d, C, rows):
    """Blocks of `rows` rows folded from r0 = 0 (the kernel takes any block height, also one that is no multiple of 8)."""
    from wf3d import ops
    pool = ops.PoolStream(offsets_d, C)
    for r0 in range(0, pf_d.shape[0], rows):
        pool.fold(pf_d[r0:r0 + rows], valid_d[r0:r0 + rows], r0)
    return pool.finish()


@pytest.mark.parametrize("rows", [8, 24, 100, 1000])
@pytest.mark.parametrize("C", [40, 64, 512])
def test_pool_stream_vs_numpy_model(C, rows):
    pf, valid, ref, mabs_u, mabs_m = pool_case(C)
    pf_d, valid_d = torch.from_numpy(pf).to(dev()), torch.from_numpy(valid).to(dev())
    offsets_d = torch.tensor(OFFSETS, dtype=torch.int32, device=dev())
    po = run_pool(pf_d, valid_d, offsets_d, C, rows)
    assert po.arg_m is None and po.arg_u is None
    masked, unmasked = po.masked.cpu().numpy().astype(np.float64), po.unmasked.cpu().numpy().astype(np.float64)
    assert np.array_equal(masked[:, :C], ref["masked"][:, :C]), "masked max"
    assert np.array_equal(unmasked[:, C:], ref["unmasked"][:, C:]), "unmasked max"
    assert np.array_equal(po.cnt.cpu().numpy(), ref["cnt"]) and np.array_equal(po.nvalid.cpu().numpy(), ref["nvalid"])
    n_u = np.diff(np.array(OFFSETS)).astype(np.float64)[:, None]
    n_m = ref["nvalid"][:, None]
    err_u, bound_u = np.abs(unmasked[:, :C] - ref["unmasked"][:, :C]), n_u * 2.0 ** -23 * mabs_u
    err_m, bound_m = np.abs(masked[:, C:] - ref["masked"][:, C:]), n_m * 2.0 ** -23 * mabs_m
    print(f"C={C} rows={rows}: worst mean error / bound: unmasked {np.max(err_u / np.maximum(bound_u, 1e-300)):.3f}, "
          f"masked {np.max(err_m / np.maximum(bound_m, 1e-300)):.3f}")
    assert np.all(err_u <= bound_u), "unmasked mean"
    assert np.all(err_m <= bound_m), "masked mean"
    # the cloud of no rows, and the cloud without a valid row
    assert not masked[1].any() and not unmasked[1].any() and not masked[2].any()
    # the same calls again: the same bits
    po2 = run_pool(pf_d, valid_d, offsets_d, C, rows)
    for a, b in ((po.masked, po2.masked), (po.unmasked, po2.unmasked), (po.cnt, po2.cnt), (po.nvalid, po2.nvalid)):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------------------------------------
# 2. the first layer without z
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R, K, D", [(33, 8, 512), (33, 5, 136), (33, 8, 1024), (33, 5, 520)],
                         ids=["fast", "general", "fast-ns2", "general-ns2"])
def test_first_layer_infer_is_first_layer_fwd_bit_for_bit(R, K, D):
    """The two instantiations of the one first-layer body against each other, in all four NS x FAST forms (NS = 2: D > 512)."""
    from wf3d import ops
    g = torch.Generator().manual_seed(R + K + D)
    x, W = torch.randn(R, K, generator=g).to(dev()), (0.3 * torch.randn(D, K, generator=g)).to(dev())
    b, gamma, beta = (t.to(dev()) for t in (0.1 * torch.randn(D, generator=g), 1 + 0.1 * torch.randn(D, generator=g),
                                            0.1 * torch.randn(D, generator=g)))
    _, _, _, h = ops.first_layer_fwd(x, W, b, gamma, beta, ops.ACT_RELU)
    h2 = ops.first_layer_infer(x, W, b, gamma, beta, ops.ACT_RELU)
    assert bool((h.view(torch.int32) != 0).any())
    assert torch.equal(h.view(torch.int32), h2.view(torch.int32))
    buf = torch.full((R, D), float("nan"), device=dev())
    assert ops.first_layer_infer(x, W, b, gamma, beta, ops.ACT_RELU, out=buf) is buf
    assert torch.equal(h.view(torch.int32), buf.view(torch.int32))


# ----------------------------------------------------------------------------------------------------------------------
# 3. encoder, dense, against the fp64 oracle
# ----------------------------------------------------------------------------------------------------------------------
DENSE = {
    "model":     dict(hidden=MODEL, out=512, B=2, N=48, precision="bf16x3"),
    "odd-rows":  dict(hidden=[64], out=40, B=3, N=11, precision="bf16x3"),           # M = 33: no multiple of 8
    "mixed":     dict(hidden=[64, 36], out=20, B=2, N=48, precision="bf16x3"),       # split, then fp32 routes
    "no-hidden": dict(hidden=[], out=32, B=2, N=48, precision="bf16x3"),
    "fp32":      dict(hidden=[128], out=256, B=2, N=48, precision="fp32"),
    "one-cloud": dict(hidden=[64], out=64, B=1, N=600, precision="bf16x3"),          # blocks inside one cloud, 16-byte pool form
    "bf16":      dict(hidden=[128], out=256, B=2, N=48, precision="bf16"),
}
_ENCODERS, _DENSE_REF = {}, {}


def encoder(hidden, out):
    """One PointNetEncoder per width set for the whole file, as tests/test_encoder_cotangents_gpu.py::encoder builds them."""
    from models.PointNetEncoder import PointNetEncoder
    key = (tuple(hidden), out)
    if key not in _ENCODERS:
        torch.manual_seed(20)
        enc = PointNetEncoder(8, hidden, out).to(dev())
        E.perturb_1d(enc)
        _ENCODERS[key] = enc
    return _ENCODERS[key]


def dense_case(cid):
    """(encoder, x, fp64 reference outputs) — the reference is computed once per case."""
    cfg = DENSE[cid]
    enc = encoder(cfg["hidden"], cfg["out"])
    if cid not in _DENSE_REF:
        x = E.dense_input(100, cfg["B"], cfg["N"])
        with torch.no_grad():
            ref = dict(zip(E.OUTS, E.ref_dense(E.params64(enc), x.double())))
        _DENSE_REF[cid] = (x, ref)
    return (enc,) + _DENSE_REF[cid]


def check_outputs(tag, outs, ref, tol):
    errs = E.out_errors(outs, ref)
    print(f"{tag}: " + ", ".join(f"{k} {a:.1e} / {b:.1e}" for k, (a, b) in errs.items()))
    for k, (a, b) in errs.items():
        assert a < tol and b < tol, (tag, k, a, b)


@pytest.mark.parametrize("rows", [8, 40, 608])
@pytest.mark.parametrize("cid", sorted(DENSE))
def test_encoder_stream_dense_vs_oracle(cid, rows):
    cfg = DENSE[cid]
    enc, x, ref = dense_case(cid)
    with mode(cfg["precision"]):
        g, pf, up = enc.encode_stream(x.to(dev()), want_pf=True, rows=rows)
        g2, none, up2 = enc.encode_stream(x.to(dev()), rows=rows)
    assert not g.requires_grad and not pf.requires_grad and not up.requires_grad
    assert none is None and torch.equal(g, g2) and torch.equal(up, up2)
    assert tuple(pf.shape) == (cfg["B"], cfg["N"], cfg["out"])
    check_outputs(f"{cid} rows={rows}", {"g": g, "pf": pf, "up": up}, ref, TOL_BF16_FWD if cfg["precision"] == "bf16" else TOL)


# ----------------------------------------------------------------------------------------------------------------------
# 4. encoder, packed
# ----------------------------------------------------------------------------------------------------------------------
# counts, capacity, counts on the device
PACKED = {
    "packed95": ([33, 7, 55], None, False),
    "packed-far": ([420, 30, 100], None, False),
    "cap-host": ([40, 1, 55], 256, False),
    "cap-dev": ([40, 0, 56], 256, True),
}
PACKED_WIDTHS = ([128], 256)
_PACKED_REF = {}


def packed_case(layout):
    counts, cap, on_dev = PACKED[layout]
    enc = encoder(*PACKED_WIDTHS)
    if layout not in _PACKED_REF:
        x = E.packed_input(100, counts)
        with torch.no_grad():
            ref = dict(zip(E.OUTS, E.ref_packed(E.params64(enc), x.double(), counts)))
        _PACKED_REF[layout] = (x, ref)
    return (enc,) + _PACKED_REF[layout]


@pytest.mark.parametrize("rows", [8, 64])
@pytest.mark.parametrize("layout", sorted(PACKED))
def test_encoder_stream_packed_vs_oracle(layout, rows):
    counts, cap, on_dev = PACKED[layout]
    enc, x, ref = packed_case(layout)
    M = sum(counts)
    pts = x
    if cap is not None:
        pts = torch.zeros(cap, x.shape[1])
        pts[:M] = x
    pts = pts.to(dev())
    with mode("bf16x3"):
        if on_dev:
            enc.encode_packed_stream(pts, [c or 1 for c in counts], capacity=cap, rows=rows)   # lazily created state of the fusion MLP
            arg = torch.tensor(counts, device=dev())
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")                 # a host read of the counts would raise here
            try:
                g, pf, up = enc.encode_packed_stream(pts, arg, capacity=cap, want_pf=True, rows=rows)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        else:
            g, pf, up = enc.encode_packed_stream(pts, counts, capacity=cap, want_pf=True, rows=rows)
    assert tuple(pf.shape) == (pts.shape[0], PACKED_WIDTHS[1])
    if cap is not None and not on_dev:
        assert not bool(pf[-(-M // 8) * 8:].any())                  # the rows behind the walk are zeros
    check_outputs(f"{layout} rows={rows}", {"g": g, "pf": pf[:M], "up": up}, ref, TOL)


# ----------------------------------------------------------------------------------------------------------------------
# 5. one block is the training forward
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_one_block_equals_the_training_forward(precision):
    """Model widths, B = 2, N = 48, rows >= M: the same kernels on the same rows, so point_features and both max pools are
    the training forward's under no_grad bit for bit (the means are sums in another order)."""
    from wf3d import infer
    from wf3d.functional import EncoderFn
    enc = encoder(MODEL, 512)
    x = E.dense_input(100, 2, 48).to(dev())
    C, params = 512, enc._mlp_params()
    with mode(precision), torch.no_grad():
        pooled0, pf0, up0 = EncoderFn.apply(x, 4, precision, *params)
        g0 = enc.encode(x)[0]
        for rows in (96, 1024):
            po, pf = infer.encoder_stream(x.reshape(96, 8), infer.DenseRows(2, 48, dev()), 4, precision, params, rows, True)
            assert torch.equal(pf0.reshape(96, C), pf), rows
            assert torch.equal(pooled0[:, :C], po.masked[:, :C]), rows          # masked max
            assert torch.equal(up0[:, C:], po.unmasked[:, C:]), rows            # unmasked max
            assert H.rel_err(po.masked.cpu().numpy(), pooled0.cpu().numpy()) < 1e-6
            assert H.rel_err(po.unmasked.cpu().numpy(), up0.cpu().numpy()) < 1e-6
        g1, pf1, up1 = enc.encode_stream(x, want_pf=True, rows=96)
    assert torch.equal(pf0, pf1) and torch.equal(up0[:, C:], up1[:, C:])
    assert H.rel_err(g1.cpu().numpy(), g0.cpu().numpy()) < 1e-5


# ----------------------------------------------------------------------------------------------------------------------
# 6. the whole model against the goldens
# ----------------------------------------------------------------------------------------------------------------------
KEYS = ["vertices", "existence_probabilities", "edge_probs", "edge_indices", "global_features", "actual_vertex_counts"]


def build_full(tag):
    """As tests/test_model_gpu.py::build_full."""
    from models.PointCloudToWireframe import PointCloudToWireframe
    gold = H.load_golden(tag)
    x, arrs, counts, V, seed, train = H.full_case_inputs(tag, gold)
    model = PointCloudToWireframe(8, V).to(dev())
    model.vertex_predictor.ensure_point_pool_proj(1024, dev())
    with torch.no_grad():
        for k, v in model.state_dict().items():
            v.copy_(torch.from_numpy(arrs[k]))
    model.set_dropout(0.0)
    model.train(train)
    return gold, model, x, counts


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("tag", ["cfg1", "ragged", "evalmode"])
def test_whole_model_stream_vs_golden(tag, precision):
    gold, model, x, counts = build_full(tag)
    xd = torch.from_numpy(x).to(dev())
    cd = counts.to(dev()) if counts is not None else None
    with mode(precision), inference("stream", rows=256), torch.no_grad():
        from wf3d import config
        assert config.inference() == "stream" and config.INFER_ROWS == 256
        out = model(xd, cd)
    from wf3d import config
    assert config.inference() == "train"
    assert list(out.keys()) == KEYS
    for k in ("vertices", "existence_probabilities", "edge_probs", "global_features"):
        assert out[k].dtype == torch.float32 and not out[k].requires_grad
    assert out["actual_vertex_counts"].dtype == torch.int64
    assert np.array_equal(out["actual_vertex_counts"].cpu().numpy(), gold["out.actual_vertex_counts"])
    lens = [len(e) for e in out["edge_indices"]]
    assert lens == gold["out.edge_index_lens"].tolist()
    flat = np.array([ij for e in out["edge_indices"] for ij in e], dtype=np.int64).reshape(-1, 2)
    assert np.array_equal(flat, gold["out.edge_indices_flat"])
    for k in ("vertices", "existence_probabilities", "edge_probs", "global_features"):
        got = out[k].cpu().numpy()
        a, b = H.rel_err(got, gold["out." + k]), H.elem_err(got, gold["out." + k], H.OUT_FLOOR[k])
        print(f"{tag} {precision} {k}: {a:.1e} / {b:.1e}")
        assert a < TOL and b < TOL, (k, a, b)
    ep = out["edge_probs"].cpu().numpy()
    for s, n in enumerate(lens):
        assert np.all(ep[s, n:] == 0.0)


# ----------------------------------------------------------------------------------------------------------------------
# 7. nothing changes with grad on
# ----------------------------------------------------------------------------------------------------------------------
def test_stream_setting_changes_nothing_with_grad_enabled():
    gold, model, x, counts = build_full("cfg1")
    xd, cd = torch.from_numpy(x).to(dev()), counts.to(dev())
    cot = None
    grads = {}
    for setting in ("train", "stream"):
        model.zero_grad(set_to_none=True)
        with inference(setting, rows=256):
            out = model(xd, cd)
            assert out["vertices"].requires_grad
            if cot is None:
                cot = {k: torch.randn(out[k].shape, generator=torch.Generator().manual_seed(5)).to(dev())
                       for k in ("vertices", "existence_probabilities", "edge_probs")}
            sum((out[k] * cot[k]).sum() for k in cot).backward()
        grads[setting] = {n: (None if p.grad is None else p.grad.clone()) for n, p in model.named_parameters()}
    assert any(g is not None and bool(g.any()) for g in grads["train"].values())
    for n, a in grads["train"].items():
        b = grads["stream"][n]
        assert (a is None and b is None) or torch.equal(a, b), n


# ----------------------------------------------------------------------------------------------------------------------
# 8. footprint
# ----------------------------------------------------------------------------------------------------------------------
def peak_of(fn):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def test_stream_footprint_is_at_most_a_quarter_of_the_training_forward():
    """Default widths, B = 2, N = 16384 (M = 32768), rows = 2048, bf16x3.  The training forward holds at least 18.4 KB of z
    per row (>= 600 MB) plus its weights; the stream path about 23 KB per BLOCK row plus 21 - 42 MB of split weights and
    the GEMMs' split-K workspace."""
    from models.PointNetEncoder import PointNetEncoder
    torch.manual_seed(0)
    enc = PointNetEncoder().to(dev())
    x = torch.randn(2, 16384, 8, generator=torch.Generator().manual_seed(1)).to(dev())
    with mode("bf16x3", split_min_rows=1024), torch.no_grad():
        stream = peak_of(lambda: enc.encode_stream(x, rows=2048))
        train = peak_of(lambda: enc.encode(x))
    print(f"peak allocated over the call: stream {stream / 2 ** 20:.1f} MiB, training forward {train / 2 ** 20:.1f} MiB, "
          f"ratio {stream / train:.3f}")
    assert train >= 600e6
    assert stream <= train / 4
