"""The key-tiled MFMA attention at head widths 64 < hd <= 128 (csrc/attn_mfma.hip, padded widths 96 and 128, any vertex
count; methods of tests/test_attn_tiled_gpu.py).

1. ctx, dqkv and lse against torch's MultiheadAttention math in fp64 at counts on each side of the 32-row blocks, the
   64-row tile of P = 96, the 128-row tile of P = 128 (and row group of both) and the third tile, at widths 68 (P = 96,
   mostly padding), 96, 100 (P = 128) and 128; bound = the rule of tests/test_degenerate_values_gpu.py::held (4 x fp32
   torch's own error, or the floor);
2. width 68: nothing is read or written past a head's columns (the neighbouring head NaN, memory after the last row
   NaN, sentinels around and inside the outputs);
3. dropout: reproducible, lse untouched, fp64 under the replayed host mask, device seed words, the VALU kernels' masks;
4. against the VALU kernels where both run;
5. bit-reproducible, and a captured forward + backward replays bit-equal to eager;
6. the padded layout (EdgePredictor(3, 256, 2), max_vertices = 160): tail rows clean on poisoned memory;
7. the whole edge head at hidden 512 / 4 heads and 200 vertices, train mode, against the oracle under the replayed
   masks: the parent refused this shape in backward().
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402
from oracle import dropout as D  # noqa: E402

WIDTHS = [(136, 2), (288, 3), (200, 2), (256, 2)]          # head widths 68, 96, 100, 128
BATCHES = [[2, 31, 32, 33], [63, 64, 65], [127, 128, 129], [255, 256, 257, 300]]
ATTN_FLOORS = (2e-5, 1e-4, 1e-5)                            # ctx, dqkv (scaled), lse (absolute)


def dev():
    return torch.device("cuda:0")


@pytest.fixture
def device_rng():
    from wf3d import config
    old = config.dropout_rng()
    config.set_dropout_rng("device")
    try:
        yield
    finally:
        config.set_dropout_rng(old)


def tiled(v):
    return H.lib_option("attn_tiled", v, default=1)


def run(ops, qkv, dctx, counts, E, heads, p=0.0, seed=0):
    meta = ops.EdgeMeta.get(counts, dev())
    ctx, lse = ops.attn_fwd(qkv, meta, E, heads, p, seed)
    return ctx, lse, ops.attn_bwd(qkv, dctx, ctx, lse, meta, E, heads, p, seed)


def inputs(counts, E, seed):
    g = torch.Generator().manual_seed(seed)
    R = sum(counts)
    return torch.randn(R, 3 * E, generator=g), torch.randn(R, E, generator=g)


def mha32(q, counts, E, heads, p, seed):
    """helpers.mha64's math in the dtype of q (its host mask is float64: cast here, the values are 0 and 1 / (1 - p))."""
    voff, _ = D.offsets(counts)
    hd = E // heads
    outs, lses = [], []
    for s, c in enumerate(counts):
        blk = q[voff[s]:voff[s] + c]
        sp = lambda t: t.reshape(c, heads, hd).transpose(0, 1)     # noqa: E731
        sc = (sp(blk[:, :E]) / hd ** 0.5) @ sp(blk[:, E:2 * E]).transpose(-1, -2)
        w = torch.softmax(sc, -1)
        if p > 0:
            w = w * torch.from_numpy(D.attention_weights(voff[s], c, heads, seed, p)).to(q.dtype)
        outs.append((w @ sp(blk[:, 2 * E:])).transpose(0, 1).reshape(c, E))
        lses.append(torch.logsumexp(sc, -1).transpose(0, 1))
    return torch.cat(outs), torch.cat(lses)


def ref(qkv, dctx, counts, E, heads, dtype, p=0.0, seed=0):
    """(ctx, lse, dqkv) on the CPU: helpers.mha64 in fp64 (the reference), the same math in fp32 (the yardstick)."""
    q = qkv.detach().cpu().to(dtype).requires_grad_()
    ctx, lse = (H.mha64 if dtype == torch.float64 else mha32)(q, counts, E, heads, p, seed)
    (ctx * dctx.detach().cpu().to(dtype)).sum().backward()
    return ctx.detach(), lse.detach(), q.grad


def errs(got, r64):
    return (H.rel_err(got[0].double().cpu().numpy(), r64[0].numpy()), H.rel_err(got[2].double().cpu().numpy(), r64[2].numpy()),
            float((got[1].double().cpu() - r64[1]).abs().max()))


def held(tag, got, qkv, dctx, counts, E, heads, p=0.0, seed=0):
    """kernel error <= max(4 x the error of the same math in fp32 torch against the same fp64 reference, floor)."""
    r64 = ref(qkv, dctx, counts, E, heads, torch.float64, p, seed)
    r32 = ref(qkv, dctx, counts, E, heads, torch.float32, p, seed)
    e, y = errs(got, r64), errs(r32, r64)
    bounds = [max(4.0 * yy, f) for yy, f in zip(y, ATTN_FLOORS)]
    print(f"{tag}: " + ", ".join(f"{n} kernel {a:.2e} fp32 torch {b:.2e} bound {c:.2e}"
                                 for n, a, b, c in zip(("ctx", "dqkv", "lse"), e, y, bounds)))
    for n, a, c in zip(("ctx", "dqkv", "lse"), e, bounds):
        assert a <= c, (tag, n, a, c)


# ---------------------------------------------------------------------------
# 1. against fp64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("counts", BATCHES)
@pytest.mark.parametrize("E,heads", WIDTHS)
def test_wide_attention_vs_fp64(E, heads, counts):
    from wf3d import ops
    qkv, dctx = inputs(counts, E, 1)
    assert ops.attn_kernel(E, heads, max(counts)) == 2
    got = run(ops, qkv.to(dev()), dctx.to(dev()), counts, E, heads)
    held(f"wide attention hd={E // heads} counts={counts}", got, qkv, dctx, counts, E, heads)


# ---------------------------------------------------------------------------
# 2. neighbours are not touched
# ---------------------------------------------------------------------------
SENT = 12345.0


def _guarded(rows, cols, fill, pad=4096):
    """A [rows, cols] view in the middle of a larger buffer filled with `fill` -> (buffer, view)."""
    buf = torch.full((2 * pad + rows * cols,), fill, dtype=torch.float32, device=dev())
    return buf, buf[pad:pad + rows * cols].view(rows, cols)


def _raw_run(ops, q_host, d_host, counts, E, heads):
    """wf3d_attn_fwd / wf3d_attn_bwd through the C entry on buffers of this test: inputs sit in NaN-filled memory, outputs
    in sentinel-filled memory.  Returns (ctx, lse, dqkv) views and their whole buffers."""
    from wf3d import _lib
    L = _lib.load()
    meta = ops.EdgeMeta.get(counts, dev())
    R = sum(counts)
    nan = float("nan")
    (_, qkv), (_, dctx) = _guarded(R, 3 * E, nan), _guarded(R, E, nan)
    qkv.copy_(q_host)
    dctx.copy_(d_host)
    (bc, ctx), (bl, lse), (bd, dqkv) = _guarded(R, E, SENT), _guarded(R, heads, SENT), _guarded(R, 3 * E, SENT)
    stream = torch.cuda.current_stream().cuda_stream
    rc = L.wf3d_attn_fwd(qkv.data_ptr(), meta.voff.data_ptr(), meta.B, meta.vmax, E, heads, 0.0, 0, ctx.data_ptr(),
                         lse.data_ptr(), stream)
    assert rc == 0, L.wf3d_last_error()
    rc = L.wf3d_attn_bwd(qkv.data_ptr(), dctx.data_ptr(), ctx.data_ptr(), lse.data_ptr(), meta.voff.data_ptr(), meta.B,
                         meta.vmax, E, heads, 0.0, 0, dqkv.data_ptr(), stream)
    assert rc == 0, L.wf3d_last_error()
    torch.cuda.synchronize()
    return (ctx, lse, dqkv), (bc, bl, bd)


def test_width_68_reads_and_writes_nothing_past_a_heads_columns():
    from wf3d import ops
    E, heads, hd, counts = 136, 2, 68, [33, 130]
    assert ops.attn_kernel(E, heads, max(counts)) == 2
    q, d = inputs(counts, E, 8)
    clean, bufs = _raw_run(ops, q, d, counts, E, heads)
    pad = 4096
    for t, b in zip(clean, bufs):
        assert bool(torch.isfinite(t).all())
        assert not bool((t == SENT).any())                         # every element of the live rows was written
        assert bool((b[:pad] == SENT).all()) and bool((b[pad + t.numel():] == SENT).all())    # and nothing outside them
    qn, dn = q.clone(), d.clone()
    for part in range(3):
        qn[:, part * E + hd:(part + 1) * E] = float("nan")        # head 1 of q, k and v
    dn[:, hd:] = float("nan")
    bad, _ = _raw_run(ops, qn, dn, counts, E, heads)
    assert torch.equal(bad[0][:, :hd], clean[0][:, :hd])
    assert torch.equal(bad[1][:, 0], clean[1][:, 0])
    for part in range(3):
        assert torch.equal(bad[2][:, part * E:part * E + hd], clean[2][:, part * E:part * E + hd]), part
    assert bool(torch.isnan(bad[0][:, hd:]).all())                 # head 1 did run on its own NaNs


# ---------------------------------------------------------------------------
# 3. dropout
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("E,heads", [(256, 2), (136, 2)])
@pytest.mark.parametrize("p,seed", [(0.1, 0xDEADBEEF), (0.5, 0x2545F491)])
def test_wide_attention_dropout_vs_fp64_with_host_mask(E, heads, p, seed):
    from wf3d import ops
    counts = [300, 7, 257]
    qkv, dctx = inputs(counts, E, 2)
    qd, dd = qkv.to(dev()), dctx.to(dev())
    assert ops.attn_kernel(E, heads, max(counts)) == 2
    got = run(ops, qd, dd, counts, E, heads, p, seed)
    again = run(ops, qd, dd, counts, E, heads, p, seed)
    lse0 = run(ops, qd, dd, counts, E, heads)[1]
    for a, b in zip(got, again):
        assert torch.equal(a, b)                                  # counter-based masks: reproducible
    assert torch.equal(got[1], lse0)                              # dropout acts after the softmax normaliser
    held(f"wide attention dropout hd={E // heads} p={p}", got, qkv, dctx, counts, E, heads, p, seed)


@pytest.mark.parametrize("E,heads", [(256, 2), (136, 2)])
def test_wide_attention_device_seed_words_equal_the_host_seed(E, heads):
    from wf3d import ops
    from wf3d.random import seed_words
    counts = [300, 7, 257]
    qkv, dctx = (t.to(dev()) for t in inputs(counts, E, 3))
    words = torch.tensor([11, 0x2545F491, 0xDEADBEEF - (1 << 32), 7, 9], dtype=torch.int32, device=dev())
    assert ops.attn_kernel(E, heads, max(counts)) == 2
    by_value = run(ops, qkv, dctx, counts, E, heads, 0.1, 0xDEADBEEF)
    with seed_words(words):
        by_word = run(ops, qkv, dctx, counts, E, heads, 0.1, 2)
    for a, b in zip(by_value, by_word):
        assert torch.equal(a, b)


def test_wide_tiled_and_valu_kernels_draw_the_same_masks():
    """p = 0.5, V = identity in head 0: ctx[i, :c] of that head is the dropped weight row itself, so the exactly-zero
    entries are the dropped keys; they must be the ones the VALU kernels drop and the ones the host mask names."""
    from wf3d import ops
    E, heads, counts, p, seed = 256, 2, [64, 40], 0.5, 0x2545F491
    qkv, dctx = (t.to(dev()) for t in inputs(counts, E, 4))
    voff, _ = D.offsets(counts)
    for s, c in enumerate(counts):
        qkv[voff[s]:voff[s] + c, 2 * E:2 * E + 128] = torch.eye(128, device=dev())[:c]
    assert ops.attn_kernel(E, heads, max(counts)) == 2
    t = run(ops, qkv, dctx, counts, E, heads, p, seed)[0]
    with tiled(0):
        assert ops.attn_kernel(E, heads, max(counts)) == 0
        v = run(ops, qkv, dctx, counts, E, heads, p, seed)[0]
    assert torch.equal(t[:, :64] == 0, v[:, :64] == 0)
    for s, c in enumerate(counts):
        keep = D.attention_weights(voff[s], c, heads, seed, p)[0] != 0          # [c, c] of head 0
        assert np.array_equal((t[voff[s]:voff[s] + c, :c] != 0).cpu().numpy(), keep), s
        assert np.array_equal((v[voff[s]:voff[s] + c, :c] != 0).cpu().numpy(), keep), s


# ---------------------------------------------------------------------------
# 4. against the VALU kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("E,heads", [(256, 2), (192, 2)])
def test_wide_tiled_agrees_with_the_valu_kernels(E, heads, p):
    from wf3d import ops
    counts = [5, 64, 130, 2]
    qkv, dctx = inputs(counts, E, 5)
    qd, dd = qkv.to(dev()), dctx.to(dev())
    with tiled(0):
        assert ops.attn_kernel(E, heads, max(counts)) == 0
        valu = run(ops, qd, dd, counts, E, heads, p, 99)
    assert ops.attn_kernel(E, heads, max(counts)) == 2
    til = run(ops, qd, dd, counts, E, heads, p, 99)
    for name, got in (("VALU", valu), ("tiled", til)):
        held(f"wide vs VALU hd={E // heads} p={p} {name}", got, qkv, dctx, counts, E, heads, p, 99)
    assert H.rel_err(til[0].cpu().numpy(), valu[0].cpu().numpy()) < 2 * ATTN_FLOORS[0]
    assert H.rel_err(til[2].cpu().numpy(), valu[2].cpu().numpy()) < 2 * ATTN_FLOORS[1]
    assert float((til[1] - valu[1]).abs().max()) < 2 * ATTN_FLOORS[2]


# ---------------------------------------------------------------------------
# 5. determinism and capture
# ---------------------------------------------------------------------------
def test_wide_eager_calls_are_bit_equal_and_a_capture_replays_them():
    from wf3d import ops
    E, heads, counts = 256, 2, [300, 513]
    qkv, dctx = (t.to(dev()) for t in inputs(counts, E, 6))
    assert ops.attn_kernel(E, heads, 513) == 2
    a = run(ops, qkv, dctx, counts, E, heads, 0.1, 5)
    b = run(ops, qkv, dctx, counts, E, heads, 0.1, 5)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    s = torch.cuda.Stream(dev())
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(ops, qkv, dctx, counts, E, heads, 0.1, 5)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = run(ops, qkv, dctx, counts, E, heads, 0.1, 5)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(a, c):
            assert torch.equal(x, y)
    q2, d2 = inputs(counts, E, 7)                                  # new contents in the captured buffers
    qkv.copy_(q2)
    dctx.copy_(d2)
    graph.replay()
    torch.cuda.synchronize()
    e = run(ops, qkv, dctx, counts, E, heads, 0.1, 5)
    for x, y in zip(e, c):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------
# 6. the padded layout
# ---------------------------------------------------------------------------
def test_wide_padded_tail_rows_clean_on_poisoned_memory_at_160_vertices(device_rng):
    """tests/test_attn_tiled_gpu.py part 6 at head width 128 and max_vertices = 160.  This step allocates about 0.3 GiB
    (five [63,600 x 256] edge tensors and their sx8 forms are the largest); 512 MiB of junk covers every block of it."""
    from models.EdgePredictor import EdgePredictor
    from test_padded_edge_gpu import SITE_PS, _run, _set_site_ps
    from wf3d import ops
    from wf3d.random import default_generator
    B, V = 5, 160
    assert ops.attn_kernel(256, 2, V) == 2
    torch.manual_seed(9)
    ep = _set_site_ps(EdgePredictor(3, 256, 2), SITE_PS).to(dev()).train()
    g = torch.Generator().manual_seed(2)
    v = torch.randn(B, V, 3, generator=g).to(dev())
    cot = torch.randn(B, V * (V - 1) // 2, generator=g).to(dev())
    counts = torch.tensor([150, 129, 6, 1, 0], device=dev())
    gen = default_generator(dev())
    st = gen.get_state()

    def run_(fill):
        junk = torch.full((128 << 20,), fill, dtype=torch.float32, device=dev())      # 512 MiB handed back to the cache
        del junk
        gen.set_state(st)
        return _run(ep, v, lambda x: ep.forward_padded(x, counts), cot)

    torch.cuda.synchronize()
    bad = run_(float("nan"))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    good = run_(0.0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(bad[0]).all()) and torch.equal(bad[0], good[0])
    assert bool(torch.isfinite(bad[1]).all()) and torch.equal(bad[1], good[1])
    assert len(good[2]) > 0
    for n in good[2]:
        assert bool(torch.isfinite(bad[2][n]).all()), n
        assert torch.equal(bad[2][n], good[2][n]), n


# ---------------------------------------------------------------------------
# 7. the whole edge head in a shape the VALU kernels refuse
# ---------------------------------------------------------------------------
def test_edge_head_hidden_512_4_heads_train_mode_vs_oracle():
    """EdgePredictor(3, 512, 4).forward_ragged at [200, 131] vertices (head width 128: the VALU kernels refuse the
    backward from 146 vertices), train mode with a different dropout p at each site, against oracle/reference_cpu.py
    under the replayed masks.  fp32 at the bound of tests/test_dropout_gpu.py's fp32 case (outputs and gradients 1e-4);
    bf16x3 gated on the outputs only (< 1e-4): its gradient error is the GEMMs' operand rounding, printed here."""
    from test_dropout_gpu import _report, edge_head_case
    from wf3d import ops
    counts = [200, 131]
    assert ops.attn_kernel(512, 4, max(counts)) == 2
    _report("hidden 512 / 4 heads, fp32, wide tiled attention", edge_head_case(counts, "fp32", None, hidden=512, heads=4), 1e-4)
    errs_b = edge_head_case(counts, "bf16x3", None, hidden=512, heads=4)
    worst = sorted(((e, n) for n, e in errs_b.items()), reverse=True)
    print("hidden 512 / 4 heads, bf16x3, wide tiled attention: worst element-wise errors",
          [(f"{e:.2e}", n) for e, n in worst[:4]])
    assert errs_b["<probs>"] < 1e-4, errs_b["<probs>"]
