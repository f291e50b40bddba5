"""A captured training step: device-side dropout seeds (wf3d.random, dropout_rng "device") and the capturable ClipAdam.

1. device seeds, eager: every train-mode forward draws new words, words[1:] are the site seeds of words[0], and the edge
   head under those words matches the fp64 oracle fed oracle.dropout.edge_head_masks(words[0]) (method and bounds of
   tests/test_dropout_gpu.py part c), with MFMA attention (V <= 256) and the VALU attention over key chunks (V > 256);
2. a captured forward + backward draws fresh masks on every replay, and each replay's gradients equal an eager step
   of a copy run from the same generator state, bit for bit;
3. ClipAdam(capturable=True): a captured step replayed equals eager capturable steps bit for bit and torch's
   clip_grad_norm_ + Adam(capturable=True) within the tests/test_optim_gpu.py bound; a tensor lr changed between
   replays takes effect; state_dict round-trips with torch's Adam; a non-capturable ClipAdam refuses to be captured;
4. the whole train.py step (model + device WireframeLoss + capturable ClipAdam + TrainMeter, dropout 0.1) replayed
   20 times equals 20 eager steps from the same start bit for bit, and the loss goes down.
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402
from helpers import oracle  # noqa: E402
from oracle import dropout as D  # noqa: E402

SITE_PS = (0.05, 0.1, 0.2, 0.3)                  # vertex_proj.5, attention, edge_mlp.3, edge_mlp.7: all different


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


def _set_site_ps(ep, ps):
    ep.vertex_proj[5].p, ep.attention.dropout, ep.edge_mlp[3].p, ep.edge_mlp[7].p = ps
    return ep


def _words(t):
    return [int(w) & 0xFFFFFFFF for w in t.cpu().tolist()]


# ---------------------------------------------------------------------------
# 1. device seeds, eager, against the oracle
# ---------------------------------------------------------------------------
def _edge_head_case(counts, precision, hidden=512, heads=8, ps=SITE_PS):
    from wf3d import config
    from models.EdgePredictor import EdgePredictor
    old = config.precision()
    config.set_precision(precision)
    try:
        torch.manual_seed(5)
        ep = _set_site_ps(EdgePredictor(3, hidden, heads), ps).to(dev()).train()
        with torch.no_grad():
            for n, p_ in ep.named_parameters():
                if p_.dim() == 1:
                    p_.add_(0.05 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(len(n))).to(dev()))
        g = torch.Generator().manual_seed(7)
        v = torch.randn(len(counts), max(counts), 3, generator=g)
        with torch.no_grad():
            ep.forward_ragged(v.to(dev()), counts)
        first = _words(ep.last_dropout_seeds)
        vg = v.clone().to(dev()).requires_grad_()
        probs = ep.forward_ragged(vg, counts)
        words = _words(ep.last_dropout_seeds)
        assert words != first                                   # a new draw per train-mode forward
        assert words[1:] == D.site_seeds(words[0])
        cot = torch.randn(probs.shape, generator=g)
        (probs * cot.to(dev())).sum().backward()
        torch.cuda.synchronize()
        masks = D.edge_head_masks(words[0], counts, ps, hidden, heads)
        P = {"edge_predictor." + n: p_.detach().cpu().double().requires_grad_() for n, p_ in ep.named_parameters()}
        vr = v.double().requires_grad_()
        errs, tot, e_out = {}, 0.0, 0.0
        for s, c in enumerate(counts):
            pr, _ = oracle.edge_forward(P, vr[s:s + 1, :c], num_heads=heads, drop=masks[s])
            e_out = max(e_out, H.elem_err(probs[s, :pr.shape[1]].detach().cpu().numpy(), pr[0].detach().numpy(), 1e-6))
            tot = tot + (pr[0] * cot[s, :pr.shape[1]].double()).sum()
        tot.backward()
        errs["<probs>"] = e_out
        errs["<vertices>"] = H.elem_err(vg.grad.cpu().numpy(), vr.grad.numpy())
        for n, p_ in ep.named_parameters():
            ref = P["edge_predictor." + n].grad
            if ref is None:
                assert p_.grad is None, n
                continue
            errs[n] = H.elem_err(p_.grad.cpu().numpy(), ref.numpy())
        return errs
    finally:
        config.set_precision(old)


def _report(tag, errs, tol):
    worst = sorted(((e, n) for n, e in errs.items()), reverse=True)
    print(f"{tag}: worst element-wise errors (bound {tol:.0e})", [(f"{e:.2e}", n) for e, n in worst[:4]])
    assert errs["<probs>"] < 1e-4, errs["<probs>"]
    bad = [(n, e) for n, e in errs.items() if not e < tol]
    assert not bad, bad


def test_device_seeds_mfma_attention_vs_oracle(device_rng):
    """fp32, V <= 256 (head_dim 64: MFMA attention): bound of the fp32 cases of test_dropout_gpu part c."""
    _report("device seeds, fp32, V=12", _edge_head_case([9, 2, 5, 12], "fp32"), 1e-4)


def test_device_seeds_chunked_valu_attention_vs_oracle(device_rng):
    """V > 256: the VALU attention over key chunks, at the production kernel selection (bf16x3; 33,700 edge rows):
    bound of the production-selection case of test_dropout_gpu part c."""
    _report("device seeds, bf16x3, V=260", _edge_head_case([260, 6], "bf16x3"), 2e-4)


def test_eval_and_p0_draw_nothing_in_device_mode(device_rng):
    from models.EdgePredictor import EdgePredictor
    from wf3d.random import default_generator
    torch.manual_seed(5)
    ep = EdgePredictor(3, 512, 8).to(dev())
    v = torch.randn(2, 7, 3, generator=torch.Generator().manual_seed(3)).to(dev())
    gen = default_generator(dev())
    st = gen.get_state()
    _set_site_ps(ep, (0.0,) * 4).train()
    with torch.no_grad():
        a = ep.forward_ragged(v, [7, 4])
    _set_site_ps(ep, SITE_PS).eval()
    with torch.no_grad():
        b = ep.forward_ragged(v, [7, 4])
    assert torch.equal(gen.get_state(), st) and ep.last_dropout_seeds is None
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# 2. replays of a captured forward + backward draw fresh masks
# ---------------------------------------------------------------------------
def test_replays_draw_fresh_masks_and_match_eager(device_rng):
    from models.EdgePredictor import EdgePredictor
    from wf3d.random import default_generator
    torch.manual_seed(11)
    ep = _set_site_ps(EdgePredictor(3, 512, 8), (0.1,) * 4).to(dev()).train()
    twin = copy.deepcopy(ep)
    counts = [12, 7, 9]
    g = torch.Generator().manual_seed(4)
    v = torch.randn(3, 12, 3, generator=g).to(dev())
    cot = torch.randn(3, 66, generator=g).to(dev())
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
        w = _words(words_buf)
        assert w[1:] == D.site_seeds(w[0])
        assert w not in seen
        seen.append(w)
        got = {n: p.grad.clone() for n, p in ep.named_parameters() if p.grad is not None}     # spatial_proj: unused
        assert len(got) == 24
        after = gen.get_state()
        assert int(after[1]) == int(before[1]) + 1
        # the eager twin from the same generator state: the same words, the same gradients bit for bit
        gen.set_state(before)
        step(twin)
        torch.cuda.synchronize()
        assert _words(twin.last_dropout_seeds) == w
        assert torch.equal(gen.get_state(), after)
        for n, p in twin.named_parameters():
            assert (p.grad is None) == (n not in got), n
            assert p.grad is None or torch.equal(p.grad, got[n]), n


# ---------------------------------------------------------------------------
# 3. ClipAdam(capturable=True)
# ---------------------------------------------------------------------------
SHAPES = [(512, 8), (512,), (1024, 512), (7,), (3, 5, 11), (70001,)] + [(37 + i,) for i in range(90)]   # 96 tensors: 2 tables


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g).to(dev())) for s in SHAPES]


def _grads(seed, scale):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(*s, generator=g) * scale).to(dev()) for s in SHAPES]


def test_clip_adam_capturable_replays_equal_eager_and_torch():
    from wf3d.optim import ClipAdam
    g0 = _grads(3, 0.05)                          # below and, scaled, above the clip threshold
    pg, pe, pt = _params(1), _params(1), _params(1)
    lr_g = torch.tensor(1e-3, device=dev())
    lr_e = torch.tensor(1e-3, device=dev())
    og = ClipAdam(pg, lr=lr_g, weight_decay=1e-6, max_norm=1.0, capturable=True)
    oe = ClipAdam(pe, lr=lr_e, weight_decay=1e-6, max_norm=1.0, capturable=True)
    ot = torch.optim.Adam(pt, lr=1e-3, weight_decay=1e-6, capturable=True)

    def load(ps, k):
        for p, g in zip(ps, g0):
            if p.grad is None:
                p.grad = torch.empty_like(p)
            p.grad.copy_(g * (1.0 if k % 2 else 30.0))

    # warm-up step on a side stream (creates the state), then the capture
    s = torch.cuda.Stream(dev())
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        load(pg, 0)
        og.step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert og.state[pg[0]]["step"].is_cuda and og.state[pg[0]]["step"].dtype == torch.float32
    k_cap = torch.zeros((), dtype=torch.float32, device=dev())      # replays alternate the gradient scale via this
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for p, g in zip(pg, g0):
            p.grad.copy_(g * (1.0 + 29.0 * k_cap))
        og.step()
    for k in range(6):
        if k > 0:
            if k == 3:
                lr_g.fill_(2.5e-4)
            k_cap.fill_(0.0 if k % 2 else 1.0)
            graph.replay()
        if k == 3:
            lr_e.fill_(2.5e-4)
            for gr in ot.param_groups:
                gr["lr"] = 2.5e-4
        load(pe, k); oe.step()
        load(pt, k)
        torch.nn.utils.clip_grad_norm_(pt, max_norm=1.0)
        ot.step()
    torch.cuda.synchronize()
    for a, b, c in zip(pg, pe, pt):
        assert torch.equal(a, b)
        for key in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(og.state[a][key], oe.state[b][key]), key
        assert float(og.state[a]["step"]) == 6.0
        assert H.elem_err(a.detach().cpu().numpy(), c.detach().cpu().numpy()) < 2e-6
        assert H.elem_err(og.state[a]["exp_avg_sq"].cpu().numpy(), ot.state[c]["exp_avg_sq"].cpu().numpy()) < 2e-6
    # the lr change took effect: a run that kept lr = 1e-3 ends elsewhere
    pk = _params(1)
    ok = ClipAdam(pk, lr=1e-3, weight_decay=1e-6, max_norm=1.0, capturable=True)
    for k in range(6):
        load(pk, k); ok.step()
    assert not torch.equal(pk[2], pg[2])
    # state_dict round trips with torch's Adam(capturable=True), both ways
    t2 = torch.optim.Adam(pe, lr=2.5e-4, weight_decay=1e-6, capturable=True)
    t2.load_state_dict(oe.state_dict())
    assert t2.state[pe[0]]["step"].is_cuda and float(t2.state[pe[0]]["step"]) == 6.0
    c2 = ClipAdam(pt, lr=2.5e-4, weight_decay=1e-6, max_norm=1.0, capturable=True)
    c2.load_state_dict(ot.state_dict())
    assert c2.param_groups[0]["capturable"] is True
    load(pe, 1); oe.step()
    load(pt, 1); c2.step()
    torch.cuda.synchronize()
    for b, c in zip(pe, pt):
        assert float(c2.state[c]["step"]) == 7.0 and c2.state[c]["step"].is_cuda
        assert H.elem_err(c.detach().cpu().numpy(), b.detach().cpu().numpy()) < 2e-6


def test_capturing_a_non_capturable_clip_adam_raises():
    from wf3d.optim import ClipAdam
    ps = _params(2)[:3]
    opt = ClipAdam(ps, lr=1e-3, max_norm=1.0)
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()
    torch.cuda.synchronize()
    x = torch.zeros(4, device=dev())
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="capturable=True"):
        with torch.cuda.graph(graph):
            x.add_(1.0)
            opt.step()
    assert int(opt.state[ps[0]]["step"]) == 1


# ---------------------------------------------------------------------------
# 4. the whole train.py step
# ---------------------------------------------------------------------------
def test_whole_training_step_replays_equal_eager(device_rng):
    from losses.WireframeLoss import WireframeLoss
    from models.PointCloudToWireframe import PointCloudToWireframe
    from wf3d.meter import TrainMeter
    from wf3d.optim import ClipAdam
    from wf3d.random import default_generator
    B, N, V = 3, 2560, 38                             # main.py / train.py: 3 clouds of 2,560 points, max_vertices 38
    torch.manual_seed(0)
    gen = default_generator(dev())
    model = PointCloudToWireframe(8, V).to(dev()).set_dropout(0.1).train()
    twin = copy.deepcopy(model)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, N, 8, generator=g).to(dev())
    counts = torch.tensor([38, 21, 30]).to(dev())
    E = V * (V - 1) // 2
    tg = {"vertices": torch.randn(B, V, 3, generator=g).to(dev()),
          "vertex_existence": (torch.arange(V)[None] < counts.cpu()[:, None]).float().to(dev()),
          "edge_labels": (torch.rand(B, E, generator=g) > 0.8).float().to(dev()), "vertex_counts": counts}
    crit = WireframeLoss(assignment="device")

    def setup(m):
        opt = ClipAdam(m.parameters(), lr=1e-3, weight_decay=1e-6, max_norm=1.0, norm_params=m.parameters, capturable=True)
        return opt, TrainMeter(dev())

    def step(m, opt, meter):
        opt.zero_grad()
        out = m(x, counts)
        res = crit(out, tg)
        res["total_loss"].backward()
        opt.step()
        meter.update(res, out["vertices"], tg["vertices"], counts)

    opt, meter = setup(model)
    opt2, meter2 = setup(twin)
    start = gen.get_state()
    torch.manual_seed(2)                              # the lazy point_pool_proj is created in the first forward
    s = torch.cuda.Stream(dev())
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step(model, opt, meter)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(model, opt, meter)
    for _ in range(20):
        graph.replay()
    torch.cuda.synchronize()
    gen_after = gen.get_state()

    gen.set_state(start)
    torch.manual_seed(2)
    for _ in range(22):
        step(twin, opt2, meter2)
    torch.cuda.synchronize()
    assert torch.equal(gen.get_state(), gen_after)
    assert int(gen_after[1]) - int(start[1]) == 22
    named2 = dict(twin.named_parameters())
    for n, p in model.named_parameters():
        assert torch.equal(p, named2[n]), n
    for p, q in zip(opt.param_groups[0]["params"], opt2.param_groups[0]["params"]):
        assert bool(opt.state[p]) == bool(opt2.state[q])             # spatial_proj never gets a gradient: no state
        if not opt.state[p]:
            continue
        assert float(opt.state[p]["step"]) == 22.0
        for key in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[p][key], opt2.state[q][key]), key
    assert torch.equal(meter.state, meter2.state)
    rec = meter.read()
    assert rec["steps"] == 22
    hist = rec["loss_history"]
    print("loss history:", [f"{h:.4f}" for h in hist])
    assert np.all(np.isfinite(hist))
    assert np.mean(hist[-5:]) < np.mean(hist[:5])
