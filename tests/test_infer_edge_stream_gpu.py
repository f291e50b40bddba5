"""The forward-only edge head (wf3d.infer.edge_stream) on the GPU: its pair kernel against the training forward's bit for
bit, block_live against the numpy model, the block walk against the fp64 oracle on both routes and both layouts, against
EdgeFn bit for bit where the two must agree, through the whole model against the goldens, and its memory footprint.

Bounds.  The pair kernel and the one-block walk: torch.equal.  Stream vs oracle and the whole model: 1e-4 by H.elem_err /
H.rel_err, the bound the project holds its forward to (TOL_OUT in tests/test_model_gpu.py); bf16: TOL_BF16_FWD of
tests/test_precision_bf16_gpu.py.  Each test prints what it measured (pytest -s)."""
import contextlib
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402
import infer_edge_model as EM  # noqa: E402
from helpers import oracle  # noqa: E402

TOL_OUT = 1e-4
TOL_BF16_FWD = 1.75e-2
GUARD = 64                                   # canary floats behind every block buffer


def dev():
    return torch.device("cuda:0")


@contextlib.contextmanager
def mode(precision, split_min_rows=None):
    """Precision and (optionally) SPLIT_MIN_ROWS for the body, as tests/test_encoder_cotangents_gpu.py::mode."""
    from wf3d import config
    old = (config.precision(), config.SPLIT_MIN_ROWS)
    config.set_precision(precision)
    if split_min_rows is not None:
        config.SPLIT_MIN_ROWS = split_min_rows
    try:
        yield
    finally:
        config.set_precision(old[0])
        config.SPLIT_MIN_ROWS = old[1]


@contextlib.contextmanager
def settings(encoder=None, edge=None, rows=None, edge_rows=None):
    from wf3d import config
    old = (config.inference(), config.edge_inference(), config.INFER_ROWS, config.INFER_EDGE_ROWS)
    if encoder is not None:
        config.set_inference(encoder)
    if edge is not None:
        config.set_edge_inference(edge)
    if rows is not None:
        config.INFER_ROWS = rows
    if edge_rows is not None:
        config.INFER_EDGE_ROWS = edge_rows
    try:
        yield
    finally:
        config.set_inference(old[0])
        config.set_edge_inference(old[1])
        config.INFER_ROWS, config.INFER_EDGE_ROWS = old[2], old[3]


def guarded(n, width, fill=float("nan")):
    """(view [n, width] or [n], the whole flat buffer): n * width floats followed by GUARD canary floats."""
    flat = torch.full((n * width + GUARD,), fill, dtype=torch.float32, device=dev())
    body = flat[:n * width]
    return (body.view(n, width) if width > 1 else body), flat


def guard_intact(flat, n, width):
    return bool(torch.isnan(flat[n * width:]).all())


# ----------------------------------------------------------------------------------------------------------------------
# 1. the pair kernel: the rows of the training forward's kernel, bit for bit
# ----------------------------------------------------------------------------------------------------------------------
def pair_layout(name):
    from wf3d import ops
    if name == "ragged":
        meta = ops.EdgeMeta([5, 2, 9, 3], dev())
        assert meta.Re == 50
        return meta, 50
    meta = ops.EdgeMeta.device(torch.tensor([5, 0, 1, 9], dtype=torch.int64, device=dev()), 4, 9)
    assert meta.Re == 144
    return meta, 46                                         # 10 + 0 + 0 + 36 live rows, then the tail


_PAIR_REF = {}


def pair_case(layout, Hd, vd):
    """(meta, live, inputs, the training forward's outputs) — the reference is computed once per case."""
    from wf3d import ops
    key = (layout, Hd, vd)
    if key not in _PAIR_REF:
        meta, live = pair_layout(layout)
        g = torch.Generator().manual_seed(Hd + vd)
        Pa, Pb = torch.randn(meta.Rv, Hd, generator=g).to(dev()), torch.randn(meta.Rv, Hd, generator=g).to(dev())
        cv = torch.randn(meta.Rv, vd, generator=g).to(dev())
        W0 = torch.randn(Hd, 2 * Hd + 2 * vd + 1, generator=g).to(dev())
        gamma, beta = (1 + 0.1 * torch.randn(Hd, generator=g)).to(dev()), (0.1 * torch.randn(Hd, generator=g)).to(dev())
        _, _, _, _, h = ops.edge_pair_fwd(Pa, Pb, cv, W0, meta, ln=(gamma, beta, ops.ACT_GELU, 0.0, 0))
        pre, mu, rs, _ = ops.edge_pair_fwd(Pa, Pb, cv, W0, meta)
        _PAIR_REF[key] = (meta, live, (Pa, Pb, cv, W0, gamma, beta), (h, pre, mu, rs))
    return _PAIR_REF[key]


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("rows", [8, 16, 24, 4096])
@pytest.mark.parametrize("Hd, vd", [(64, 3), (144, 2), (512, 3), (520, 3), (1032, 3)])      # NS = 1, 1, 2, 4, 8
@pytest.mark.parametrize("layout", ["ragged", "padded"])
def test_pair_infer_is_pair_fwd_bit_for_bit(layout, Hd, vd, rows):
    from wf3d import infer, ops
    meta, live, (Pa, Pb, cv, W0, gamma, beta), (h0, pre0, mu0, rs0) = pair_case(layout, Hd, vd)
    assert bool((bits(h0[:live]) != 0).any()) and bool((pre0[:live] != 0).any())
    for e0, n in infer.block_plan(meta.Re, rows):
        h, h_flat = guarded(n, Hd)
        assert ops.edge_pair_infer(Pa, Pb, cv, W0, meta, e0, n, h, ln=(gamma, beta, ops.ACT_GELU)) is h
        assert torch.equal(bits(h), bits(h0[e0:e0 + n])), (e0, n, "h")
        assert guard_intact(h_flat, n, Hd), (e0, n, "h canary")
        (pre, pre_flat), (mu, mu_flat), (rs, rs_flat) = guarded(n, Hd), guarded(n, 1), guarded(n, 1)
        ops.edge_pair_infer(Pa, Pb, cv, W0, meta, e0, n, (pre, mu, rs))
        for name, got, want in (("pre", pre, pre0), ("mu", mu, mu0), ("rs", rs, rs0)):
            assert torch.equal(bits(got), bits(want[e0:e0 + n])), (e0, n, name)
        assert guard_intact(pre_flat, n, Hd) and guard_intact(mu_flat, n, 1) and guard_intact(rs_flat, n, 1), (e0, n)
        # the tail of a padded layout: exact zeros in every output
        t0 = max(live - e0, 0)
        if t0 < n:
            assert not bool(bits(h[t0:]).any()) and not bool(bits(pre[t0:]).any())
            assert not bool(bits(mu[t0:]).any()) and not bool(bits(rs[t0:]).any())


def test_pair_infer_rows_do_not_depend_on_the_map_behind_the_block():
    """esample at and past e0 + n rewritten to -1 (what a tail looks like): the block's rows keep their bits."""
    from wf3d import infer, ops
    meta, live, (Pa, Pb, cv, W0, gamma, beta), (h0, pre0, mu0, rs0) = pair_case("ragged", 64, 3)
    for e0, n in infer.block_plan(meta.Re, 16)[:-1]:
        cut = copy.copy(meta)
        cut.esample = meta.esample.clone()
        cut.esample[e0 + n:] = -1
        h, _ = guarded(n, 64)
        ops.edge_pair_infer(Pa, Pb, cv, W0, cut, e0, n, h, ln=(gamma, beta, ops.ACT_GELU))
        assert torch.equal(bits(h), bits(h0[e0:e0 + n])), e0


def test_pair_infer_under_a_block_live_count():
    """V = 24, B = 4: 1,104 padded rows, 324 live.  One block of 1,024 rows under blive[0] = 324: rows [0, 512), the
    count's 256-row extent, are the training kernel's rows (zeros from 324 on), rows [512, 1024) are not written; the
    second block (80 rows, blive[1] = 0) is not written at all."""
    from wf3d import ops
    Hd, vd = 64, 3
    meta = ops.EdgeMeta.device(torch.tensor([24, 3, 0, 10], dtype=torch.int64, device=dev()), 4, 24, tail="skip")
    assert meta.Re == 1104
    g = torch.Generator().manual_seed(3)
    Pa, Pb = torch.randn(meta.Rv, Hd, generator=g).to(dev()), torch.randn(meta.Rv, Hd, generator=g).to(dev())
    cv, W0 = torch.randn(meta.Rv, vd, generator=g).to(dev()), torch.randn(Hd, 2 * Hd + 2 * vd + 1, generator=g).to(dev())
    gamma, beta = torch.ones(Hd, device=dev()), torch.zeros(Hd, device=dev())
    _, _, _, _, h0 = ops.edge_pair_fwd(Pa, Pb, cv, W0, meta, ln=(gamma, beta, ops.ACT_GELU, 0.0, 0))
    blive = ops.block_live(meta.live, 1024, meta.Re, 2)
    assert blive.tolist() == [324, 0]
    for k, (e0, n, extent) in enumerate([(0, 1024, 512), (1024, 80, 0)]):
        h, flat = guarded(n, Hd)
        with ops.live_rows(blive[k:k + 1]):
            ops.edge_pair_infer(Pa, Pb, cv, W0, meta, e0, n, h, ln=(gamma, beta, ops.ACT_GELU))
        assert torch.equal(bits(h[:extent]), bits(h0[e0:e0 + extent]))
        assert bool(torch.isnan(h[extent:]).all()) and guard_intact(flat, n, Hd)
    assert not bool(bits(h0[324:512]).any())


def test_pair_infer_refuses_what_it_cannot_take():
    from wf3d import ops
    meta, live, (Pa, Pb, cv, W0, gamma, beta), _ = pair_case("ragged", 64, 3)
    h = torch.empty(8, 64, device=dev())
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.edge_pair_infer(Pa, Pb, cv, W0, meta, 4, 8, h, ln=(gamma, beta, ops.ACT_GELU))
    with pytest.raises(RuntimeError, match="not inside"):
        ops.edge_pair_infer(Pa, Pb, cv, W0, meta, 48, 8, h, ln=(gamma, beta, ops.ACT_GELU))
    with pytest.raises(RuntimeError, match=r"contiguous float32 \[8, 64\]"):
        ops.edge_pair_infer(Pa, Pb, cv, W0, meta, 0, 8, torch.empty(16, 64, device=dev()), ln=(gamma, beta, ops.ACT_GELU))


# ----------------------------------------------------------------------------------------------------------------------
# 2. block_live against the numpy model
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows, Re", [(256, 1000), (8, 50), (24, 144), (4096, 144)])
def test_block_live_vs_numpy_model(rows, Re):
    from wf3d import ops
    nblocks = -(-Re // rows)
    for total in (0, 1, rows, rows + 1, Re, Re - 1, Re + 7, -2):
        t = torch.tensor([total], dtype=torch.int32, device=dev())
        got = ops.block_live(t, rows, Re, nblocks)
        assert got.dtype == torch.int32 and tuple(got.shape) == (nblocks,)
        assert np.array_equal(got.cpu().numpy(), EM.block_live(total, rows, Re, nblocks)), (total, got.tolist())


# ----------------------------------------------------------------------------------------------------------------------
# 3. the block walk against the fp64 oracle
# ----------------------------------------------------------------------------------------------------------------------
# (hidden, heads, counts, SPLIT_MIN_ROWS or None = the shipped value)
CASES = {
    "h64-fp32-route": (64, 2, [7, 4], None),               # 27 rows: the fp32 route in every precision
    "h256-split": (256, 4, [50, 3], None),                 # 1,228 rows (2,450 padded): the split route as shipped
    "h512-split": (512, 8, [12, 2, 7], 1),                 # 88 rows, the model's widths, split by SPLIT_MIN_ROWS = 1
}
HEIGHTS = [8, 24, 4096]
_HEAD, _ORACLE = {}, {}


def edge_head(hidden, heads):
    """One EdgePredictor per width for the whole file, built as tests/test_model_gpu.py::_edge_head_case builds it."""
    from models.EdgePredictor import EdgePredictor
    if (hidden, heads) not in _HEAD:
        torch.manual_seed(60 + hidden)
        ep = EdgePredictor(3, hidden, heads).to(dev())
        with torch.no_grad():
            for n, p_ in ep.named_parameters():
                if p_.dim() == 1:
                    p_.add_(0.05 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(len(n))).to(dev()))
        _HEAD[hidden, heads] = ep.eval()
    return _HEAD[hidden, heads]


def oracle_case(cid):
    """(module, vertices [B, max(counts), 3], per-sample fp64 probabilities) — the oracle runs once per case."""
    hidden, heads, counts, _ = CASES[cid]
    ep = edge_head(hidden, heads)
    if cid not in _ORACLE:
        v = torch.randn(len(counts), max(counts), 3, generator=torch.Generator().manual_seed(7))
        P = {"edge_predictor." + n: p_.detach().cpu().double() for n, p_ in ep.named_parameters()}
        with torch.no_grad():
            ref = [oracle.edge_forward(P, v[s:s + 1, :c].double(), num_heads=heads)[0][0].numpy() for s, c in enumerate(counts)]
        _ORACLE[cid] = (v, ref)
    return (ep,) + _ORACLE[cid]


def check_vs_oracle(tag, probs, ref, tol):
    worst = 0.0
    p = probs.cpu().numpy()
    for s, r in enumerate(ref):
        worst = max(worst, H.elem_err(p[s, :len(r)], r, 1e-6))
        assert np.all(p[s, len(r):] == 0.0), (tag, s, "padding")
    print(f"{tag}: worst element error {worst:.2e} (bound {tol:.1e})")
    assert worst < tol, (tag, worst)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("cid", sorted(CASES))
def test_edge_stream_vs_oracle(cid, precision):
    hidden, heads, counts, smr = CASES[cid]
    ep, v, ref = oracle_case(cid)
    vd_, cd = v.to(dev()), torch.tensor(counts, device=dev())
    tol = TOL_BF16_FWD if precision == "bf16" else TOL_OUT
    B, V = v.shape[0], v.shape[1]
    width = max(len(r) for r in ref)
    with mode(precision, smr):
        for rows in HEIGHTS:
            ragged = ep.forward_stream(vd_, counts, rows=rows)
            assert tuple(ragged.shape) == (B, width) and ragged.dtype == torch.float32 and not ragged.requires_grad
            check_vs_oracle(f"{cid} {precision} rows={rows} ragged", ragged, ref, tol)
            for tail in ("compute", "skip"):
                padded = ep.forward_stream(vd_, cd, rows=rows, tail=tail)
                assert tuple(padded.shape) == (B, V * (V - 1) // 2) and not padded.requires_grad
                assert tuple(padded[:, :width].shape) == tuple(ragged.shape)
                assert not bool(padded[:, width:].any())
                check_vs_oracle(f"{cid} {precision} rows={rows} padded/{tail}", padded, ref, tol)


# ----------------------------------------------------------------------------------------------------------------------
# 4. equality with the training forward
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid, precision", [("h64-fp32-route", "bf16x3"), ("h256-split", "bf16x3"), ("h256-split", "fp32"),
                                            ("h512-split", "bf16x3"), ("h512-split", "bf16")])
def test_one_block_equals_edgefn_and_skip_equals_compute(cid, precision):
    """rows >= Re: the same kernels on the same rows, so edge_probs are EdgeFn's under no_grad bit for bit, ragged and
    padded.  tail="skip" equals tail="compute" bit for bit at every height; a repeated call repeats its bits."""
    from wf3d import config
    from wf3d.functional import _edge_routes
    hidden, heads, counts, smr = CASES[cid]
    ep, v, _ = oracle_case(cid)
    vd_, cd = v.to(dev()), torch.tensor(counts, device=dev())
    B, V = v.shape[0], v.shape[1]
    Re_pad = B * V * (V - 1) // 2
    with mode(precision, smr), settings(edge="train"), torch.no_grad():
        want_split = cid != "h64-fp32-route" and precision != "fp32"
        assert (_edge_routes(Re_pad, hidden, precision, False)[0].fwd == "split") == want_split
        train_r = ep.forward_ragged(vd_, counts)
        train_p = {t: ep.forward_padded(vd_, cd, tail=t) for t in ("compute", "skip")}
        assert config.edge_inference() == "train"
        for rows in (-(-Re_pad // 8) * 8, 1 << 20):
            assert torch.equal(ep.forward_stream(vd_, counts, rows=rows), train_r), ("ragged", rows)
            for t in ("compute", "skip"):
                assert torch.equal(ep.forward_stream(vd_, cd, rows=rows, tail=t), train_p[t]), ("padded", t, rows)
        for rows in HEIGHTS + [256]:
            a = ep.forward_stream(vd_, cd, rows=rows, tail="compute")
            b = ep.forward_stream(vd_, cd, rows=rows, tail="skip")
            assert torch.equal(a, b), rows
            assert torch.equal(b, ep.forward_stream(vd_, cd, rows=rows, tail="skip")), rows
            r1 = ep.forward_stream(vd_, counts, rows=rows)
            assert torch.equal(r1, ep.forward_stream(vd_, counts, rows=rows)), rows


def test_padded_stream_reads_nothing_on_the_host(monkeypatch):
    """2,450 padded rows, 1,228 live, blocks of 256: the walk runs under per-block counts (block_live is called once) and
    nothing synchronises with the host."""
    from wf3d import infer
    ep, v, ref = oracle_case("h256-split")
    vd_, cd = v.to(dev()), torch.tensor(CASES["h256-split"][2], device=dev())
    lives = []
    real = infer.ops.block_live
    monkeypatch.setattr(infer.ops, "block_live", lambda *a: (lives.append(a[1:]), real(*a))[1])
    with mode("bf16x3"):
        first = ep.forward_stream(vd_, cd, rows=256, tail="skip")             # loads every kernel, grows the workspaces
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                              # a host read would raise here
        try:
            again = ep.forward_stream(vd_, cd, rows=256, tail="skip")
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert lives == [(256, 2450, 10)] * 2
    assert torch.equal(first, again)
    check_vs_oracle("no-sync padded/skip rows=256", again, ref, TOL_OUT)


def test_the_setting_routes_the_module_and_only_without_grad_and_dropout(monkeypatch):
    """forward / forward_ragged / forward_padded go to edge_stream when the edge setting is "stream", grad mode is off
    and no dropout probability is active; otherwise they run EdgeFn as before."""
    import models.EdgePredictor as EP
    from wf3d import infer
    ep, v, _ = oracle_case("h64-fp32-route")
    counts = CASES["h64-fp32-route"][2]
    vd_, cd = v.to(dev()), torch.tensor(counts, device=dev())
    calls = []
    real = infer.edge_stream

    def spy(*a, **k):
        calls.append(a[1])
        return real(*a, **k)
    monkeypatch.setattr(EP.infer, "edge_stream", spy)
    with mode("bf16x3"):
        with settings(edge="train"), torch.no_grad():
            base_r, base_p, (base_f, idx) = ep.forward_ragged(vd_, counts), ep.forward_padded(vd_, cd), ep(vd_[:, :4])
        assert calls == []
        with settings(edge="stream", edge_rows=256):
            with torch.no_grad():
                assert torch.equal(ep.forward_ragged(vd_, counts), base_r)
                probs, ecounts, width = ep.forward_padded(vd_, cd, return_layout=True, tail="skip")
                assert torch.equal(probs, base_p) and ecounts.tolist() == counts and int(width) == 21
                f, idx2 = ep(vd_[:, :4])
                assert torch.equal(f, base_f) and idx2 == idx
                assert len(calls) == 3
                with pytest.raises(IndexError):
                    ep.forward_ragged(vd_, [7, 1])
            # grad mode on: EdgeFn, with a graph
            out = ep.forward_ragged(vd_, counts)
            assert out.requires_grad and torch.equal(out, base_r) and len(calls) == 3
            # dropout active: EdgeFn, with its masks
            ep.train()
            try:
                with torch.no_grad():
                    dropped = ep.forward_ragged(vd_, counts)
                assert len(calls) == 3 and not torch.equal(dropped, base_r)
                with pytest.raises(ValueError, match="no dropout"):
                    ep.forward_stream(vd_, counts)
            finally:
                ep.eval()


# ----------------------------------------------------------------------------------------------------------------------
# 5. the whole model against the goldens
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
def test_whole_model_both_stages_streamed_vs_golden(tag, precision, monkeypatch):
    import models.EdgePredictor as EP
    from wf3d import infer
    gold, model, x, counts = build_full(tag)
    xd = torch.from_numpy(x).to(dev())
    cd = counts.to(dev()) if counts is not None else None
    calls = []
    real = infer.edge_stream
    monkeypatch.setattr(EP.infer, "edge_stream", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with mode(precision), settings(encoder="stream", edge="stream", rows=256, edge_rows=64), torch.no_grad():
        out = model(xd, cd)
    assert calls == [1]                                             # the edge head took the forward-only path
    assert list(out.keys()) == KEYS
    for k in ("vertices", "existence_probabilities", "edge_probs", "global_features"):
        assert out[k].dtype == torch.float32 and not out[k].requires_grad
    assert np.array_equal(out["actual_vertex_counts"].cpu().numpy(), gold["out.actual_vertex_counts"])
    lens = [len(e) for e in out["edge_indices"]]
    assert lens == gold["out.edge_index_lens"].tolist()
    flat = np.array([ij for e in out["edge_indices"] for ij in e], dtype=np.int64).reshape(-1, 2)
    assert np.array_equal(flat, gold["out.edge_indices_flat"])
    for k in ("vertices", "existence_probabilities", "edge_probs", "global_features"):
        got = out[k].cpu().numpy()
        a, b = H.rel_err(got, gold["out." + k]), H.elem_err(got, gold["out." + k], H.OUT_FLOOR[k])
        print(f"{tag} {precision} {k}: {a:.1e} / {b:.1e}")
        assert a < TOL_OUT and b < TOL_OUT, (k, a, b)
    ep = out["edge_probs"].cpu().numpy()
    for s, n in enumerate(lens):
        assert np.all(ep[s, n:] == 0.0)


def test_both_settings_change_nothing_with_grad_enabled():
    gold, model, x, counts = build_full("cfg1")
    xd, cd = torch.from_numpy(x).to(dev()), counts.to(dev())
    cot = None
    grads, outs = {}, {}
    for setting in ("train", "stream"):
        model.zero_grad(set_to_none=True)
        with settings(encoder=setting, edge=setting, rows=256, edge_rows=64):
            out = model(xd, cd)
            assert out["edge_probs"].requires_grad
            if cot is None:
                cot = {k: torch.randn(out[k].shape, generator=torch.Generator().manual_seed(5)).to(dev())
                       for k in ("vertices", "existence_probabilities", "edge_probs")}
            sum((out[k] * cot[k]).sum() for k in cot).backward()
        outs[setting] = out["edge_probs"].detach().clone()
        grads[setting] = {n: (None if p.grad is None else p.grad.clone()) for n, p in model.named_parameters()}
    assert torch.equal(outs["train"], outs["stream"])
    assert any(g is not None and bool(g.any()) for g in grads["train"].values())
    for n, a in grads["train"].items():
        b = grads["stream"][n]
        assert (a is None and b is None) or torch.equal(a, b), n


# ----------------------------------------------------------------------------------------------------------------------
# 6. footprint
# ----------------------------------------------------------------------------------------------------------------------
def peak_of(fn):
    """As tests/test_infer_stream_gpu.py::peak_of."""
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def test_stream_footprint_is_at_most_a_quarter_of_the_training_forward():
    """Default widths, eval mode, bf16x3, counts [128] * 4 = 32,512 edge rows, rows = 2048.  The training forward holds at
    least h1, z2, h2 and z3 of every edge row: 32512 x 4608 B = 149.8 MB.  The stream holds 9.4 MB of block buffers, the
    per-vertex tensors (512 rows), the split weights, the logits and the GEMMs' workspace."""
    from models.EdgePredictor import EdgePredictor
    torch.manual_seed(0)
    ep = EdgePredictor().to(dev()).eval()
    counts = [128] * 4
    v = torch.randn(4, 128, 3, generator=torch.Generator().manual_seed(1)).to(dev())
    with mode("bf16x3"), settings(edge="train"), torch.no_grad():
        stream = peak_of(lambda: ep.forward_stream(v, counts, rows=2048))
        train = peak_of(lambda: ep.forward_ragged(v, counts))
        same = torch.equal(ep.forward_stream(v, counts, rows=1 << 16), ep.forward_ragged(v, counts))
    print(f"peak allocated over the call: stream {stream / 2 ** 20:.1f} MiB, training forward {train / 2 ** 20:.1f} MiB, "
          f"ratio {stream / train:.3f}")
    assert same
    assert train >= 32512 * 4608
    assert stream <= train / 4
