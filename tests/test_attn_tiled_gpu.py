"""The key-tiled MFMA attention (csrc/attn_mfma.hip, head_dim 64, any vertex count; wf3d_set_option "attn_tiled").

1. ctx and dqkv against torch's MultiheadAttention math in fp64 at counts on each side of every boundary (the 32-row
   blocks, the 128-row tiles, the 256-vertex limit of the resident kernels), bounds of tests/test_model_gpu.py;
2. lse against the fp64 log-sum-exp (the backward recomputes the weights from it);
3. dropout: reproducible, host seed and device seed words, fp64 under the replayed host mask (method and bounds of
   tests/test_dropout_gpu.py part b), the same masks as the VALU kernels draw;
4. against the resident MFMA kernel where both apply; the default dispatch at vmax <= 256 did not move;
5. bit-reproducible, and a captured forward + backward replays bit-equal to eager, with device seeds too;
6. the padded layout at max_vertices = 320 against the oracle, tail rows clean on poisoned memory;
7. the whole edge head at V = 320 in train mode against the oracle under the replayed masks.
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402
from oracle import dropout as D  # noqa: E402

E, HEADS = 512, 8
BATCHES = [[2, 31, 32, 33], [255, 256, 257, 300], [511, 512, 513], [1000, 2]]


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


def tiled(v=2):
    return H.lib_option("attn_tiled", v, default=1)


def mha64(qkv64, counts, p=0.0, seed=0):
    """(ctx, lse) of torch's MultiheadAttention math in fp64, with the host dropout mask on the softmax weights
    (helpers.mha64 at this file's E and HEADS)."""
    return H.mha64(qkv64, counts, E, HEADS, p, seed)


def run(ops, qkv, dctx, counts, p=0.0, seed=0):
    meta = ops.EdgeMeta.get(counts, dev())
    ctx, lse = ops.attn_fwd(qkv, meta, E, HEADS, p, seed)
    return ctx, lse, ops.attn_bwd(qkv, dctx, ctx, lse, meta, E, HEADS, p, seed)


def inputs(counts, seed):
    g = torch.Generator().manual_seed(seed)
    R = sum(counts)
    return torch.randn(R, 3 * E, generator=g).to(dev()), torch.randn(R, E, generator=g).to(dev())


def fp64_errors(got, qkv, dctx, counts, p=0.0, seed=0):
    q64 = qkv.double().cpu().requires_grad_()
    ref, lse = mha64(q64, counts, p, seed)
    (ref * dctx.double().cpu()).sum().backward()
    return (H.rel_err(got[0].cpu().numpy(), ref.detach().numpy()), H.rel_err(got[2].cpu().numpy(), q64.grad.numpy()),
            float((got[1].double().cpu() - lse.detach()).abs().max()))


# ---------------------------------------------------------------------------
# 1, 2. against fp64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("option", [2, 1])
@pytest.mark.parametrize("counts", BATCHES)
def test_tiled_attention_vs_fp64(counts, option):
    """Option 2 puts every batch on the tiled kernels; under the default (1) those with a sample beyond 256 vertices."""
    from wf3d import ops
    if option == 1 and max(counts) <= 256:
        counts = counts + [257]
    qkv, dctx = inputs(counts, 1)
    with tiled(option):
        assert ops.attn_kernel(E, HEADS, max(counts)) == 2
        got = run(ops, qkv, dctx, counts)
    e_ctx, e_d, e_lse = fp64_errors(got, qkv, dctx, counts)
    print(f"tiled attention counts={counts} option={option}: ctx {e_ctx:.2e} (< 2e-5), dqkv {e_d:.2e} (< 1e-4), "
          f"lse {e_lse:.2e} (< 1e-5 abs)")
    assert e_ctx < 2e-5
    assert e_d < 1e-4
    assert e_lse < 1e-5


# ---------------------------------------------------------------------------
# 3. dropout
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [[300, 7, 257], [5, 64, 130, 256, 2], [513, 33]])
@pytest.mark.parametrize("p,seed", [(0.1, 0xDEADBEEF), (0.5, 0x2545F491)])
def test_tiled_attention_dropout_vs_fp64_with_host_mask(counts, p, seed):
    from wf3d import ops
    qkv, dctx = inputs(counts, 2)
    with tiled():
        assert ops.attn_kernel(E, HEADS, max(counts)) == 2
        got = run(ops, qkv, dctx, counts, p, seed)
        again = run(ops, qkv, dctx, counts, p, seed)
        lse0 = run(ops, qkv, dctx, counts)[1]
    for a, b in zip(got, again):
        assert torch.equal(a, b)                                  # counter-based masks: reproducible
    assert torch.equal(got[1], lse0)                              # dropout acts after the softmax normaliser
    e_ctx, e_d, _ = fp64_errors(got, qkv, dctx, counts, p, seed)
    print(f"tiled attention dropout counts={counts} p={p}: ctx {e_ctx:.2e} (< 2e-5), dqkv {e_d:.2e} (< 1e-4)")
    assert e_ctx < 2e-5
    assert e_d < 1e-4


def test_tiled_attention_device_seed_words_equal_the_host_seed():
    from wf3d import ops
    from wf3d.random import seed_words
    counts = [300, 513]
    qkv, dctx = inputs(counts, 3)
    words = torch.tensor([11, 0x2545F491, 0xDEADBEEF - (1 << 32), 7, 9], dtype=torch.int32, device=dev())
    with tiled():
        by_value = run(ops, qkv, dctx, counts, 0.1, 0xDEADBEEF)
        with seed_words(words):
            by_word = run(ops, qkv, dctx, counts, 0.1, 2)
    for a, b in zip(by_value, by_word):
        assert torch.equal(a, b)


def test_tiled_and_valu_kernels_draw_the_same_masks():
    """p = 0.5, V = identity in head 0: ctx[i, :64] of that head is the dropped weight row itself, so the exactly-zero
    entries are the dropped keys; they must be the ones the VALU kernels drop and the ones the host mask names."""
    from wf3d import ops
    counts, p, seed = [64, 40], 0.5, 0x2545F491
    qkv, dctx = inputs(counts, 4)
    voff, _ = D.offsets(counts)
    for s, c in enumerate(counts):
        qkv[voff[s]:voff[s] + c, 2 * E:2 * E + 64] = torch.eye(64, device=dev())[:c]
    with tiled(2):
        assert ops.attn_kernel(E, HEADS, max(counts)) == 2
        t = run(ops, qkv, dctx, counts, p, seed)[0]
    big = [300, 64]                                                 # option 0 at vmax > 256: the chunked VALU kernels
    qb, db = inputs(big, 4)
    qb[:300, 2 * E:2 * E + 64] = 0
    qb[:64, 2 * E:2 * E + 64] = torch.eye(64, device=dev())         # keys 0..63 of sample 0 carry the identity
    with tiled(0):
        assert ops.attn_kernel(E, HEADS, 300) == 0
        v = run(ops, qb, db, big, p, seed)
    with tiled(2):
        tb = run(ops, qb, db, big, p, seed)
    assert torch.equal(v[0][:300, :64] == 0, tb[0][:300, :64] == 0)
    e_ctx = H.rel_err(tb[0].cpu().numpy(), v[0].double().cpu().numpy())
    assert e_ctx < 2e-5, e_ctx                                      # cannot hold if the masks differ
    for s, c in enumerate(counts):
        keep = D.attention_weights(voff[s], c, HEADS, seed, p)[0] != 0          # [c, c] of head 0
        assert np.array_equal((t[voff[s]:voff[s] + c, :c] != 0).cpu().numpy(), keep), s


# ---------------------------------------------------------------------------
# 4. against the resident kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_tiled_agrees_with_resident_and_default_dispatch_did_not_move(p):
    from wf3d import ops
    counts = [5, 64, 130, 256, 2, 129]
    qkv, dctx = inputs(counts, 5)
    with tiled(0):
        assert ops.attn_kernel(E, HEADS, 256) == 1
        off = run(ops, qkv, dctx, counts, p, 99)
    assert ops.attn_kernel(E, HEADS, 256) == 1
    res = run(ops, qkv, dctx, counts, p, 99)
    for a, b in zip(off, res):
        assert torch.equal(a, b)                                  # the same kernel: option 1 == option 0 here
    with tiled(2):
        assert ops.attn_kernel(E, HEADS, 256) == 2
        til = run(ops, qkv, dctx, counts, p, 99)
    for got in (res, til):
        e_ctx, e_d, e_lse = fp64_errors(got, qkv, dctx, counts, p, 99)
        assert e_ctx < 2e-5 and e_d < 1e-4 and e_lse < 1e-5, (e_ctx, e_d, e_lse)
    assert H.rel_err(til[0].cpu().numpy(), res[0].cpu().numpy()) < 2 * 2e-5
    assert H.rel_err(til[2].cpu().numpy(), res[2].cpu().numpy()) < 2 * 1e-4


# ---------------------------------------------------------------------------
# 5. determinism and capture
# ---------------------------------------------------------------------------
def test_tiled_eager_calls_are_bit_equal_and_a_capture_replays_them():
    from wf3d import ops
    counts = [300, 513]
    qkv, dctx = inputs(counts, 6)
    assert ops.attn_kernel(E, HEADS, 513) == 2
    a = run(ops, qkv, dctx, counts, 0.1, 5)
    b = run(ops, qkv, dctx, counts, 0.1, 5)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    s = torch.cuda.Stream(dev())
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(ops, qkv, dctx, counts, 0.1, 5)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = run(ops, qkv, dctx, counts, 0.1, 5)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(a, c):
            assert torch.equal(x, y)
    q2, d2 = inputs(counts, 7)                                     # new contents in the captured buffers
    qkv.copy_(q2)
    dctx.copy_(d2)
    graph.replay()
    torch.cuda.synchronize()
    e = run(ops, qkv, dctx, counts, 0.1, 5)
    for x, y in zip(e, c):
        assert torch.equal(x, y)


def test_edge_head_replays_draw_fresh_masks_and_match_eager_beyond_256_vertices(device_rng):
    """tests/test_graph_step_gpu.py part 2 at counts [300, 513]: the tiled attention inside a captured step."""
    from models.EdgePredictor import EdgePredictor
    from wf3d import ops
    from wf3d.random import default_generator
    torch.manual_seed(11)
    ep = EdgePredictor(3, 512, 8)
    ep.vertex_proj[5].p, ep.attention.dropout, ep.edge_mlp[3].p, ep.edge_mlp[7].p = (0.1,) * 4
    ep = ep.to(dev()).train()
    twin = copy.deepcopy(ep)
    counts = [300, 513]
    assert ops.attn_kernel(512, 8, max(counts)) == 2
    g = torch.Generator().manual_seed(4)
    v = torch.randn(2, 513, 3, generator=g).to(dev())
    cot = torch.randn(2, 513 * 512 // 2, generator=g).to(dev())
    gen = default_generator(dev())

    def step(m):
        for p in m.parameters():
            p.grad = None
        (m.forward_ragged(v, counts) * cot).sum().backward()

    s = torch.cuda.Stream(dev())
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step(ep)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(ep)
    words_buf = ep.last_dropout_seeds
    seen = []
    for _ in range(3):
        before = gen.get_state()
        graph.replay()
        torch.cuda.synchronize()
        w = [int(x) & 0xFFFFFFFF for x in words_buf.cpu().tolist()]
        assert w[1:] == D.site_seeds(w[0]) and w not in seen
        seen.append(w)
        got = {n: p.grad.clone() for n, p in ep.named_parameters() if p.grad is not None}
        assert len(got) == 24
        gen.set_state(before)
        step(twin)
        torch.cuda.synchronize()
        assert [int(x) & 0xFFFFFFFF for x in twin.last_dropout_seeds.cpu().tolist()] == w
        for n, p in twin.named_parameters():
            assert (p.grad is None) == (n not in got), n
            assert p.grad is None or torch.equal(p.grad, got[n]), n


# ---------------------------------------------------------------------------
# 6. the padded layout
# ---------------------------------------------------------------------------
def test_padded_layout_at_320_vertices_vs_oracle(device_rng):
    """forward_padded, max_vertices = 320, ragged device counts with a 1- and a 0-vertex sample: method and bound of
    tests/test_padded_edge_gpu.py part 3 (bf16x3, the production kernel selection: 2e-4)."""
    from test_padded_edge_gpu import _oracle_case, _report
    from wf3d import ops
    assert ops.attn_kernel(512, 8, 320) == 2
    _report("padded, bf16x3, V=320, tiled attention", _oracle_case([300, 129, 260, 6, 1, 0], 320, "bf16x3"), 2e-4)


def test_padded_tail_rows_clean_on_poisoned_memory_at_320_vertices(device_rng):
    """tests/test_padded_edge_gpu.py part 4 at max_vertices = 320."""
    from models.EdgePredictor import EdgePredictor
    from test_padded_edge_gpu import SITE_PS, _run, _set_site_ps
    from wf3d.random import default_generator
    B, V = 4, 320
    torch.manual_seed(9)
    ep = _set_site_ps(EdgePredictor(3, 512, 8), SITE_PS).to(dev()).train()
    g = torch.Generator().manual_seed(2)
    v = torch.randn(B, V, 3, generator=g).to(dev())
    cot = torch.randn(B, V * (V - 1) // 2, generator=g).to(dev())
    counts = torch.tensor([300, 7, 1, 257], device=dev())
    gen = default_generator(dev())
    st = gen.get_state()

    def run_(fill):
        junk = torch.full((256 << 20,), fill, dtype=torch.float32, device=dev())      # 1 GiB handed back to the cache
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
    for n in good[2]:
        assert bool(torch.isfinite(bad[2][n]).all()), n
        assert torch.equal(bad[2][n], good[2][n]), n


# ---------------------------------------------------------------------------
# 7. the whole edge head at V = 320
# ---------------------------------------------------------------------------
def test_edge_head_v320_train_mode_vs_oracle():
    """EdgePredictor.forward_ragged at 320 vertices, bf16x3 at the production kernel selection, train mode with a
    different dropout p at each site, against oracle/reference_cpu.py under the replayed masks; bound of
    tests/test_model_gpu.py::test_edge_head_v256_vs_oracle in bf16x3 mode (outputs 1e-4, gradients 2e-4)."""
    from test_dropout_gpu import _report, edge_head_case
    from wf3d import ops
    assert ops.attn_kernel(512, 8, 320) == 2
    _report("V=320 edge head, bf16x3, tiled attention", edge_head_case([320, 131], "bf16x3", None), 2e-4)
