"""The padded edge head: a row layout built on the device from count tensors (ops.EdgeMeta.device, wf3d_edge_layout),
so that one captured forward / training step serves batches with any vertex counts.

1. the layout kernel's tables equal the host EdgeMeta's in the live region, -1 in the tails, and the clamped counts and
   the edge width are right, for random, 0, 1, negative, > V, all-V counts and B = 1;
2. at counts = V, forward_padded equals forward_ragged bit for bit (outputs and every gradient), in all three precision
   modes, in eval and in train under the same device seed words;
3. at ragged counts, forward_padded against the fp64 oracle (method and bounds of tests/test_graph_step_gpu.py part 1,
   masks from oracle.dropout.edge_head_masks): out[:, :max_e], exact zeros after it, zero gradients of the vertex rows
   past each count; MFMA attention (V <= 256) and the VALU attention (V > 256);
4. tail hygiene: after the caching allocator hands back NaN-filled memory, a padded forward + backward at ragged
   counts has finite gradients equal to a run on clean memory;
5. the loss with a device edge width: padded predictions with full-width labels equal the sliced predictions with
   reference-width labels, for both assignment modes;
6. capture: a padded eval forward captures and its replays on new clouds equal eager calls; one captured train.py step
   (device seeds, device loss, ClipAdam(capturable=True), TrainMeter) replayed over batches with different counts
   equals eager padded steps bit for bit; an eager padded step's gradients agree with a ragged step's.
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402
from helpers import oracle  # noqa: E402
from oracle import dropout as D  # noqa: E402

SITE_PS = (0.05, 0.1, 0.2, 0.3)


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


class _precision:
    def __init__(self, p):
        self.p = p

    def __enter__(self):
        from wf3d import config
        self.old = config.precision()
        config.set_precision(self.p)

    def __exit__(self, *exc):
        from wf3d import config
        config.set_precision(self.old)


def _set_site_ps(ep, ps):
    ep.vertex_proj[5].p, ep.attention.dropout, ep.edge_mlp[3].p, ep.edge_mlp[7].p = ps
    return ep


def _clamp(c, V):
    return min(c, V) if c >= 0 else max(V + c, 0)


# ---------------------------------------------------------------------------
# 1. the layout kernel
# ---------------------------------------------------------------------------
LAYOUT_CASES = [([5, 0, 1, 7, -2, 12, 9], 9), ([4], 4), ([0], 6), ([1, 1], 3), ([3, 3, 3], 3), ([-20, 40, 2], 10),
                ([0, 0, 5], 5), ([256, 200, 17], 256)]


@pytest.mark.parametrize("case", range(len(LAYOUT_CASES) + 3))
def test_layout_kernel_matches_host_meta(case):
    from wf3d import ops
    if case < len(LAYOUT_CASES):
        counts, V = LAYOUT_CASES[case]
    else:
        rng = np.random.default_rng(case)
        V = int(rng.integers(2, 70))
        counts = rng.integers(-V - 3, V + 5, size=int(rng.integers(1, 40))).tolist()
    B = len(counts)
    m = ops.EdgeMeta.device(torch.tensor(counts, dtype=torch.int64, device=dev()), B, V)
    torch.cuda.synchronize()
    cl = [_clamp(c, V) for c in counts]
    h = ops.EdgeMeta(cl, dev())
    E = V * (V - 1) // 2
    assert (m.B, m.Rv, m.Re, m.vmax, m.max_e) == (B, B * V, B * E, V, E)
    assert m.counts.tolist() == cl
    assert int(m.width) == max(c * (c - 1) // 2 for c in cl)
    assert torch.equal(m.voff, h.voff) and torch.equal(m.eoff, h.eoff)
    assert torch.equal(m.vsample[:h.Rv], h.vsample) and torch.equal(m.esample[:h.Re], h.esample)
    assert bool((m.vsample[h.Rv:] == -1).all()) and bool((m.esample[h.Re:] == -1).all())


# ---------------------------------------------------------------------------
# 2. bit-identical to the ragged path at counts = V
# ---------------------------------------------------------------------------
def _run(ep, v, fn, cot):
    for p in ep.parameters():
        p.grad = None
    vg = v.clone().requires_grad_()
    out = fn(vg)
    (out * cot).sum().backward()
    return out.detach(), vg.grad, {n: p.grad for n, p in ep.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_full_counts_bit_identical_to_ragged(precision, mode, device_rng):
    from models.EdgePredictor import EdgePredictor
    from wf3d.random import default_generator
    B, V = 3, 40
    torch.manual_seed(3)
    ep = _set_site_ps(EdgePredictor(3, 512, 8), SITE_PS).to(dev())
    ep.train() if mode == "train" else ep.eval()
    g = torch.Generator().manual_seed(8)
    v = torch.randn(B, V, 3, generator=g).to(dev())
    cot = torch.randn(B, V * (V - 1) // 2, generator=g).to(dev())
    gen = default_generator(dev())
    counts = torch.full((B,), V, dtype=torch.int64, device=dev())
    with _precision(precision):
        st = gen.get_state()
        a = _run(ep, v, lambda x: ep.forward_ragged(x, [V] * B), cot)
        wa = ep.last_dropout_seeds.clone() if mode == "train" else None
        gen.set_state(st)
        b = _run(ep, v, lambda x: ep.forward_padded(x, counts), cot)
        if mode == "train":
            assert torch.equal(ep.last_dropout_seeds, wa)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert len(a[2]) == 24 and set(a[2]) == set(b[2])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


# ---------------------------------------------------------------------------
# 3. ragged counts against the fp64 oracle
# ---------------------------------------------------------------------------
def _oracle_case(counts, V, precision, hidden=512, heads=8, ps=SITE_PS):
    """counts: the live samples (>= 2 vertices) first, then samples with fewer than 2 (all-zero rows)."""
    from models.EdgePredictor import EdgePredictor
    live = [c for c in counts if c >= 2]
    assert counts[:len(live)] == live
    with _precision(precision):
        torch.manual_seed(5)
        ep = _set_site_ps(EdgePredictor(3, hidden, heads), ps).to(dev()).train()
        with torch.no_grad():
            for n, p_ in ep.named_parameters():
                if p_.dim() == 1:
                    p_.add_(0.05 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(len(n))).to(dev()))
        g = torch.Generator().manual_seed(7)
        v = torch.randn(len(counts), V, 3, generator=g)
        vg = v.clone().to(dev()).requires_grad_()
        probs = ep.forward_padded(vg, torch.tensor(counts, device=dev()))
        words = [int(w) & 0xFFFFFFFF for w in ep.last_dropout_seeds.cpu().tolist()]
        assert tuple(probs.shape) == (len(counts), V * (V - 1) // 2)
        cot = torch.randn(probs.shape, generator=g)
        (probs * cot.to(dev())).sum().backward()
        torch.cuda.synchronize()
    masks = D.edge_head_masks(words[0], counts, ps, hidden, heads, s1=len(live))
    P = {"edge_predictor." + n: p_.detach().cpu().double().requires_grad_() for n, p_ in ep.named_parameters()}
    vr = v.double().requires_grad_()
    pc = probs.detach().cpu()
    errs, tot, e_out = {}, 0.0, 0.0
    for s, c in enumerate(counts):
        if c < 2:
            assert not pc[s].any(), s
            continue
        pr, _ = oracle.edge_forward(P, vr[s:s + 1, :c], num_heads=heads, drop=masks[s])
        E = pr.shape[1]
        assert E == c * (c - 1) // 2
        e_out = max(e_out, H.elem_err(pc[s, :E].numpy(), pr[0].detach().numpy(), 1e-6))
        assert not pc[s, E:].any(), s                          # exactly 0.0 past the sample's pairs
        tot = tot + (pr[0] * cot[s, :E].double()).sum()
    tot.backward()
    gv = vg.grad.cpu()
    for s, c in enumerate(counts):
        assert not gv[s, max(c, 0):].any(), s                  # vertex rows past the count: exactly zero
    errs["<probs>"] = e_out
    errs["<vertices>"] = H.elem_err(gv.numpy(), vr.grad.numpy())
    for n, p_ in ep.named_parameters():
        ref = P["edge_predictor." + n].grad
        if ref is None:
            assert p_.grad is None, n
            continue
        assert bool(torch.isfinite(p_.grad).all()), n
        errs[n] = H.elem_err(p_.grad.cpu().numpy(), ref.numpy())
    return errs


def _report(tag, errs, tol):
    worst = sorted(((e, n) for n, e in errs.items()), reverse=True)
    print(f"{tag}: worst element-wise errors (bound {tol:.0e})", [(f"{e:.2e}", n) for e, n in worst[:4]])
    assert errs["<probs>"] < 1e-4, errs["<probs>"]
    bad = [(n, e) for n, e in errs.items() if not e < tol]
    assert not bad, bad


def test_ragged_counts_mfma_attention_vs_oracle(device_rng):
    _report("padded, fp32, V=14", _oracle_case([9, 2, 5, 12, 1, 0], 14, "fp32"), 1e-4)


def test_ragged_counts_valu_attention_vs_oracle(device_rng):
    _report("padded, bf16x3, V=262", _oracle_case([260, 6, 1], 262, "bf16x3"), 2e-4)


# ---------------------------------------------------------------------------
# 4. tail hygiene on poisoned memory
# ---------------------------------------------------------------------------
def test_tail_rows_clean_on_poisoned_memory(device_rng):
    from models.EdgePredictor import EdgePredictor
    from wf3d.random import default_generator
    B, V = 4, 48
    torch.manual_seed(9)
    ep = _set_site_ps(EdgePredictor(3, 512, 8), SITE_PS).to(dev()).train()
    g = torch.Generator().manual_seed(2)
    v = torch.randn(B, V, 3, generator=g).to(dev())
    cot = torch.randn(B, V * (V - 1) // 2, generator=g).to(dev())
    counts = torch.tensor([30, 7, 1, 19], device=dev())
    gen = default_generator(dev())
    st = gen.get_state()

    def run(fill):
        junk = torch.full((256 << 20,), fill, dtype=torch.float32, device=dev())      # 1 GiB handed back to the cache
        del junk
        gen.set_state(st)
        return _run(ep, v, lambda x: ep.forward_padded(x, counts), cot)

    torch.cuda.synchronize()
    bad = run(float("nan"))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    good = run(0.0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(bad[0]).all()) and torch.equal(bad[0], good[0])
    assert bool(torch.isfinite(bad[1]).all()) and torch.equal(bad[1], good[1])
    for n in good[2]:
        assert bool(torch.isfinite(bad[2][n]).all()), n
        assert torch.equal(bad[2][n], good[2][n]), n


# ---------------------------------------------------------------------------
# 5. the loss with a device edge width
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("assignment", ["device", "scipy"])
def test_loss_with_device_edge_width(assignment):
    from losses.WireframeLoss import WireframeLoss
    B, V = 3, 12
    counts = [10, 7, 9]
    Ef, Ew = V * (V - 1) // 2, max(c * (c - 1) // 2 for c in counts)
    g = torch.Generator().manual_seed(6)
    live = torch.zeros(B, Ef, dtype=torch.bool)
    for s, c in enumerate(counts):
        live[s, :c * (c - 1) // 2] = True
    probs = torch.rand(B, Ef, generator=g).clamp(0.02, 0.98) * live
    labels = (torch.rand(B, Ef, generator=g) > 0.7).float() * live
    pv = torch.randn(B, V, 3, generator=g).to(dev())
    pe = torch.rand(B, V, generator=g).clamp(0.02, 0.98).to(dev())
    tc = torch.tensor(counts, device=dev())
    tg = {"vertices": torch.randn(B, V, 3, generator=g).to(dev()),
          "vertex_existence": (torch.arange(V)[None] < tc.cpu()[:, None]).float().to(dev()), "vertex_counts": tc}
    crit = WireframeLoss(vertex_weight=3.0, edge_weight=1.0, existence_weight=1.5, assignment=assignment)
    pa = probs.clone().to(dev()).requires_grad_()
    ra = crit({"vertices": pv, "existence_probabilities": pe, "edge_probs": pa,
               "edge_width": torch.tensor(Ew, device=dev())}, dict(tg, edge_labels=labels.to(dev())))
    ra["total_loss"].backward()
    pb = probs[:, :Ew].clone().to(dev()).requires_grad_()
    rb = crit({"vertices": pv, "existence_probabilities": pe, "edge_probs": pb},
              dict(tg, edge_labels=labels[:, :Ew].contiguous().to(dev())))
    rb["total_loss"].backward()
    for k in ("total_loss", "vertex_loss", "existence_loss", "edge_loss"):
        a, b = float(ra[k].detach()), float(rb[k].detach())
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (k, a, b)
    assert float(rb["edge_loss"]) > 0
    ga, gb = pa.grad.cpu(), pb.grad.cpu()
    assert H.elem_err(ga[:, :Ew].numpy(), gb.numpy()) < 1e-5
    assert not ga[:, Ew:].any()


# ---------------------------------------------------------------------------
# 6. capture
# ---------------------------------------------------------------------------
def _capture(fn):
    s = torch.cuda.Stream(dev())
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


def test_padded_eval_forward_captures_and_replays():
    from models.PointCloudToWireframe import PointCloudToWireframe
    B, N, V = 3, 2048, 38
    torch.manual_seed(4)
    model = PointCloudToWireframe(8, V).to(dev()).eval().set_edge_layout("padded")
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, N, 8, generator=g).to(dev())
    with torch.no_grad():
        graph, out = _capture(lambda: model(x))
        for k in range(3):
            x.copy_(torch.randn(B, N, 8, generator=g).to(dev()) * (1.0 + 0.5 * k))
            graph.replay()
            want = model(x)
            torch.cuda.synchronize()
            assert set(out) == set(want) >= {"edge_probs", "edge_indices", "edge_counts", "edge_width"}
            for key in ("vertices", "existence_probabilities", "edge_probs", "global_features", "actual_vertex_counts",
                        "edge_counts", "edge_width"):
                assert torch.equal(out[key], want[key]), (k, key)
            assert tuple(out["edge_probs"].shape) == (B, V * (V - 1) // 2)
            cl = want["edge_counts"].tolist()
            assert cl == [min(c, V) for c in want["actual_vertex_counts"].tolist()]
            assert want["edge_indices"] == [[[i, j] for i in range(c) for j in range(i + 1, c)] for c in cl]


def _batches(n, B, N, V, seed):
    """Clouds with train.py-style targets at full label width; counts drawn from the demo set's 4..38 spread."""
    from wf3d.targets import train_targets
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        cnt = rng.integers(4, V + 1, size=B).tolist()
        vs = [rng.standard_normal((c, 3)).astype(np.float32) for c in cnt]
        es = [np.stack([np.arange(c - 1), np.arange(1, c)], 1) for c in cnt]
        t = train_targets(vs, es, V, device=dev(), full_width=True)
        t["x"] = torch.from_numpy(rng.standard_normal((B, N, 8)).astype(np.float32)).to(dev())
        out.append(t)
    assert len({tuple(b["vertex_counts"].tolist()) for b in out}) == n
    return out


def test_one_captured_training_step_serves_every_batch(device_rng):
    from losses.WireframeLoss import WireframeLoss
    from models.PointCloudToWireframe import PointCloudToWireframe
    from wf3d.meter import TrainMeter
    from wf3d.optim import ClipAdam
    from wf3d.random import default_generator
    B, N, V = 3, 2560, 38
    torch.manual_seed(0)
    gen = default_generator(dev())
    model = PointCloudToWireframe(8, V).to(dev()).set_dropout(0.1).train().set_edge_layout("padded")
    twin = copy.deepcopy(model)
    batches = _batches(6, B, N, V, seed=1)
    static = {k: t.clone() for k, t in batches[0].items()}
    crit = WireframeLoss(vertex_weight=3.0, edge_weight=1.0, existence_weight=1.5, assignment="device")

    def setup(m):
        opt = ClipAdam(m.parameters(), lr=1e-3, weight_decay=1e-6, max_norm=1.0, norm_params=m.parameters, capturable=True)
        return opt, TrainMeter(dev())

    def step(m, opt, meter, bt):
        opt.zero_grad()
        out = m(bt["x"], bt["vertex_counts"])
        res = crit(out, {k: bt[k] for k in ("vertices", "vertex_existence", "edge_labels", "vertex_counts")})
        res["total_loss"].backward()
        opt.step()
        meter.update(res, out["vertices"], bt["vertices"], bt["vertex_counts"])

    opt, meter = setup(model)
    opt2, meter2 = setup(twin)
    start = gen.get_state()
    torch.manual_seed(2)                              # the lazy point_pool_proj is created in the first forward
    graph, _ = _capture(lambda: step(model, opt, meter, static))
    gen.set_state(start)
    torch.manual_seed(2)
    for _ in range(2):
        step(twin, opt2, meter2, batches[0])
    named2 = dict(twin.named_parameters())
    for k, bt in enumerate(batches[1:]):
        for key, t in bt.items():
            static[key].copy_(t)
        before = gen.get_state()
        graph.replay()
        torch.cuda.synchronize()
        after = gen.get_state()
        gen.set_state(before)                         # the eager twin draws the same seed words
        step(twin, opt2, meter2, bt)
        torch.cuda.synchronize()
        assert torch.equal(gen.get_state(), after)
        torch.cuda.synchronize()
        for n, p in model.named_parameters():
            assert torch.equal(p, named2[n]), (k, n)
            assert (p.grad is None) == (named2[n].grad is None) and (p.grad is None or torch.equal(p.grad, named2[n].grad)), (k, n)
    assert torch.equal(meter.state, meter2.state)
    hist = meter.read()["loss_history"]
    assert len(hist) == 2 + len(batches) - 1 and np.all(np.isfinite(hist))


def test_padded_step_gradients_agree_with_ragged(device_rng):
    from losses.WireframeLoss import WireframeLoss
    from models.PointCloudToWireframe import PointCloudToWireframe
    from wf3d.random import default_generator
    B, N, V = 3, 2560, 38
    torch.manual_seed(0)
    ragged = PointCloudToWireframe(8, V).to(dev()).set_dropout(0.1).train()
    padded = copy.deepcopy(ragged).set_edge_layout("padded")
    bt = _batches(1, B, N, V, seed=5)[0]
    Ew = max(c * (c - 1) // 2 for c in bt["vertex_counts"].tolist())          # train.py's label width
    crit = WireframeLoss(vertex_weight=3.0, edge_weight=1.0, existence_weight=1.5, assignment="device")
    gen = default_generator(dev())
    st = gen.get_state()
    res = {}
    for name, m, labels in (("ragged", ragged, bt["edge_labels"][:, :Ew].contiguous()), ("padded", padded, bt["edge_labels"])):
        gen.set_state(st)
        torch.manual_seed(2)
        out = m(bt["x"], bt["vertex_counts"])
        r = crit(out, {"vertices": bt["vertices"], "vertex_existence": bt["vertex_existence"], "edge_labels": labels,
                       "vertex_counts": bt["vertex_counts"]})
        r["total_loss"].backward()
        res[name] = (out, {k: float(v.detach()) for k, v in r.items()})
    torch.cuda.synchronize()
    (oa, la), (ob, lb) = res["ragged"], res["padded"]
    assert int(ob["edge_width"]) == Ew == oa["edge_probs"].shape[1]
    assert H.elem_err(ob["edge_probs"][:, :Ew].detach().cpu().numpy(), oa["edge_probs"].detach().cpu().numpy(), 1e-6) < 1e-4
    for k in la:
        assert abs(la[k] - lb[k]) <= 1e-4 * max(1.0, abs(la[k])), (k, la[k], lb[k])
    named = dict(padded.named_parameters())
    errs = {}
    for n, p in ragged.named_parameters():
        q = named[n]
        assert (p.grad is None) == (q.grad is None), n
        if p.grad is not None:
            errs[n] = H.elem_err(q.grad.cpu().numpy(), p.grad.cpu().numpy())
    worst = sorted(((e, n) for n, e in errs.items()), reverse=True)
    print("padded vs ragged step, worst element-wise gradient errors", [(f"{e:.2e}", n) for e, n in worst[:4]])
    assert worst[0][0] < 2e-4, worst[:4]
