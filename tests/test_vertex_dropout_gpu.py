"""Train-mode dropout at the vertex head's sites vertex_mlp{k}.3, the whole model with all twelve sites active, and a
captured training step that draws fresh encoder / vertex-head masks on every replay.

  - VertexPredictor in train mode with a different p per site, B = 3 (with and without point_features) and B = 33:
    outputs and every gradient against tests/dropout_sites_model.py under the masks of the recorded seed, at the bounds of
    tests/test_model_gpu.py::test_vertex_head_other_sizes_vs_oracle (TOL_OUT, TOL_GRAD).  While a site is active the head
    runs on the generic GEMM kernels; with p = 0 everywhere B = 3 stays on the skinny kernels, bit-equal to a module whose
    p was never touched.
  - PointCloudToWireframe, B = 2, N = 640, V = 8, twelve sites: the oracle assembled from the fp64 encoder and vertex
    head of dropout_sites_model and oracle.edge_forward(drop=), each under the masks of its module's seed and the kernels'
    own decisions, at the bounds of tests/test_dropout_gpu.py's model case (TOL forward, TOL_X3 gradients).
  - plumbing: eval() draws nothing and is today's bits; p = 1 raises naming the site; a model with edge-head dropout
    alone consumes torch's CPU generator and the device generator exactly as before.
  - capture (device seeds, capturable ClipAdam, padded edge layout): replays draw different encoder and vertex masks, and
    equal an eager twin from the same generator state bit for bit."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dropout_sites_model as M  # noqa: E402
import helpers as H  # noqa: E402
from helpers import oracle  # noqa: E402
from oracle import dropout as D  # noqa: E402
from test_frozen_grad_gpu import TOL, TOL_X3  # noqa: E402
from test_model_gpu import TOL_GRAD, TOL_OUT  # noqa: E402

VERT_PS = (0.05, 0.1, 0.2, 0.3)
ENC_PS = (0.05, 0.1, 0.2, 0.3)
EDGE_PS = (0.05, 0.1, 0.2, 0.3)


def dev():
    return torch.device("cuda:0")


def host_seed_after(s):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(s)
        return int(torch.empty((), dtype=torch.int64).random_().item())


def set_vertex_ps(vp, ps):
    for st, p in zip((vp.vertex_mlp1, vp.vertex_mlp2, vp.vertex_mlp3, vp.vertex_mlp4), ps):
        st[3].p = p
    return vp


def perturb_1d(m):
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(n))).to(p.device))


# ----------------------------------------------------------------------------------------------------------------------
# the vertex head
# ----------------------------------------------------------------------------------------------------------------------
_VP = {}


def vertex_head():
    """One VertexPredictor(512, 8) for the file (its values never change: only .grad and the sites' p do)."""
    from models.VertexPredictor import VertexPredictor
    if "vp" not in _VP:
        torch.manual_seed(41)
        vp = VertexPredictor(512, 8, 4).to(dev())
        vp.ensure_point_pool_proj(2 * 48, dev())
        perturb_1d(vp)
        _VP["vp"] = vp
    vp = _VP["vp"]
    vp.zero_grad(set_to_none=True)
    return vp.train()


def vertex_inputs(B, npts=7):
    g0 = torch.Generator().manual_seed(3)
    return (torch.randn(B, 512, generator=g0), torch.randn(B, npts, 48, generator=g0),
            torch.randn(B, 8, 3, generator=g0), torch.randn(B, 8, generator=g0))


@pytest.mark.parametrize("B,with_pf", [(3, True), (3, False), (33, True)])
def test_vertex_head_train_mode_vs_fp64_model_with_replayed_masks(B, with_pf):
    vp = set_vertex_ps(vertex_head(), VERT_PS)
    g, pf, cv, ce = vertex_inputs(B)
    gg = g.clone().to(dev()).requires_grad_()
    pg = pf.clone().to(dev()).requires_grad_() if with_pf else None
    torch.manual_seed(50 + B)
    out = vp(gg, pg)
    seed = vp.last_dropout_seed
    assert seed == host_seed_after(50 + B)
    assert out["existence_probabilities"].grad_fn.skinny is False       # an active site: the generic GEMM route, any B
    ((out["vertices"] * cv.to(dev())).sum() + (out["existence_probabilities"] * ce.to(dev())).sum()).backward()

    P = {"vertex_predictor." + n: p.detach().cpu().double().requires_grad_() for n, p in vp.named_parameters()}
    gr = g.double().requires_grad_()
    pr = pf.double().requires_grad_() if with_pf else None
    masks = M.vertex_masks(seed, VERT_PS, B)
    assert sorted(masks) == sorted(M.VERTEX_SITES)
    ref = M.vertex_forward(P, gr, pr, 8, 4, drop=masks)
    ((ref["vertices"] * cv.double()).sum() + (ref["existence_probabilities"] * ce.double()).sum()).backward()
    errs = {"<vertices>": H.rel_err(out["vertices"].detach().cpu().numpy(), ref["vertices"].detach().numpy()),
            "<exist>": H.rel_err(out["existence_probabilities"].detach().cpu().numpy(), ref["existence_probabilities"].detach().numpy())}
    assert errs["<vertices>"] < TOL_OUT and errs["<exist>"] < TOL_OUT, errs
    assert np.array_equal(out["actual_vertex_counts"].cpu().numpy(), ref["actual_vertex_counts"].numpy())
    gerrs = {"<g>": H.rel_err(gg.grad.cpu().numpy(), gr.grad.numpy())}
    if with_pf:
        gerrs["<pf>"] = H.rel_err(pg.grad.cpu().numpy(), pr.grad.numpy())
    for n, p in vp.named_parameters():
        r = P["vertex_predictor." + n].grad
        if not with_pf and n.startswith("point_pool_proj"):
            assert r is None and p.grad is None, n
            continue
        assert r is not None and p.grad is not None, n
        gerrs[n] = H.rel_err(p.grad.cpu().numpy(), r.numpy())
    worst = sorted(((e, n) for n, e in gerrs.items()), reverse=True)[:3]
    print(f"vertex head B={B} pf={with_pf}: forward {errs}; worst gradients {[(f'{e:.1e}', n) for e, n in worst]}")
    bad = [(n, e) for n, e in gerrs.items() if not e < TOL_GRAD]
    assert not bad, bad
    # and the masks matter, each at its own site: without one the model is far from the kernels' output
    with torch.no_grad():
        for site in masks:
            less = {s: v for s, v in masks.items() if s != site}
            off = H.rel_err(out["vertices"].detach().cpu().numpy(), M.vertex_forward(P, gr, pr, 8, 4, drop=less)["vertices"].numpy())
            assert off > 10 * TOL_OUT, (site, off)


def test_vertex_head_p0_keeps_the_skinny_route_and_todays_bits():
    vp = set_vertex_ps(vertex_head(), (0.0,) * 4)
    g, pf, cv, ce = vertex_inputs(3)

    def run(m):
        m.zero_grad(set_to_none=True)
        gg, pg = g.clone().to(dev()).requires_grad_(), pf.clone().to(dev()).requires_grad_()
        state = torch.get_rng_state()
        out = m(gg, pg)
        assert torch.equal(torch.get_rng_state(), state)                 # nothing drawn
        ((out["vertices"] * cv.to(dev())).sum() + (out["existence_probabilities"] * ce.to(dev())).sum()).backward()
        return out, [gg.grad, pg.grad] + [p.grad for p in m.parameters()]

    out, grads = run(vp)
    assert out["existence_probabilities"].grad_fn.skinny is True
    fresh = copy.deepcopy(vp)                                            # same values, no p ever set on it
    for st in (fresh.vertex_mlp1, fresh.vertex_mlp2, fresh.vertex_mlp3, fresh.vertex_mlp4):
        st[3] = torch.nn.Dropout(0.0)
    out2, grads2 = run(fresh)
    # eval mode with p > 0: the same
    out3, grads3 = run(set_vertex_ps(vp, VERT_PS).eval())
    assert out3["existence_probabilities"].grad_fn.skinny is True
    for o, gs in ((out2, grads2), (out3, grads3)):
        for k in ("vertices", "existence_probabilities", "actual_vertex_counts"):
            assert torch.equal(o[k], out[k]), k
        for a, b in zip(gs, grads):
            assert torch.equal(a, b)
    # train mode with the sites on changes the output
    out4 = vp.train()(g.to(dev()), pf.to(dev()))
    assert not torch.equal(out4["vertices"], out["vertices"])


@pytest.mark.parametrize("k", [1, 4])
def test_vertex_head_p_one_is_refused_naming_the_site(k):
    ps = [0.1] * 4
    ps[k - 1] = 1.0
    vp = set_vertex_ps(vertex_head(), ps)
    g, pf, _, _ = vertex_inputs(3)
    with pytest.raises(ValueError, match=rf"vertex_mlp{k}\.3"):
        vp(g.to(dev()), pf.to(dev()))
    vp.eval()(g.to(dev()), pf.to(dev()))
    set_vertex_ps(vp, (0.0,) * 4)


# ----------------------------------------------------------------------------------------------------------------------
# the whole model, twelve sites
# ----------------------------------------------------------------------------------------------------------------------
def set_model_ps(model, enc_ps, vert_ps, edge_ps):
    for i, p in enumerate(enc_ps):
        model.encoder.mlp[4 * i + 3].p = p
    set_vertex_ps(model.vertex_predictor, vert_ps)
    ep = model.edge_predictor
    ep.vertex_proj[5].p, ep.attention.dropout, ep.edge_mlp[3].p, ep.edge_mlp[7].p = edge_ps
    return model


_MODEL = {}


def small_model(V=8):
    """One PointCloudToWireframe(8, V) for the file, its lazy layer created."""
    from models.PointCloudToWireframe import PointCloudToWireframe
    if V not in _MODEL:
        torch.manual_seed(20)
        m = PointCloudToWireframe(8, V).to(dev())
        perturb_1d(m)
        m.vertex_predictor.ensure_point_pool_proj(1024, dev())
        _MODEL[V] = m
    m = _MODEL[V]
    m.zero_grad(set_to_none=True)
    return m.set_edge_layout("ragged").train()


def three_host_seeds(s):
    """What the encoder, the vertex head and the edge head draw, in that order, after torch.manual_seed(s)."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(s)
        return [int(torch.empty((), dtype=torch.int64).random_().item()) for _ in range(3)]


def test_whole_model_twelve_sites_vs_assembled_fp64_oracle():
    B, N, V, counts = 2, 640, 8, [8, 5]
    model = set_model_ps(small_model(V), ENC_PS, VERT_PS, EDGE_PS)
    enc, vp, ep = model.encoder, model.vertex_predictor, model.edge_predictor
    cnt = torch.tensor(counts)
    for seed in range(100, 116):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, N, 8, generator=g)
        x[0, N - N // 4:] = 0.0
        model.zero_grad(set_to_none=True)
        torch.manual_seed(seed)
        out = model(x.to(dev()), cnt.to(dev()))
        frozen, n_border = H.capture_decisions(out, model, kernel_masks=True)
        if n_border == 0:
            break
    else:
        pytest.fail("no borderline-free input in 16 draws")
    seeds = three_host_seeds(seed)
    assert [enc.last_dropout_seed, vp.last_dropout_seed] == seeds[:2]
    cot = {k: torch.randn(out[k].shape, generator=g) for k in ("vertices", "existence_probabilities", "edge_probs")}
    sum((out[k] * cot[k].to(dev())).sum() for k in cot).backward()
    got = {n: p.grad.detach().cpu().numpy() for n, p in model.named_parameters() if p.grad is not None}

    P = oracle.params_from_module(model, dtype=torch.float64)
    x64 = x.double()
    gl, pf, _ = M.ref_dense(P, x64, M.encoder_masks(seeds[0], ENC_PS, B * N, [512, 1024, 2048, 1024]), frozen)
    vo = M.vertex_forward(P, gl, pf, V, 4, drop=M.vertex_masks(seeds[1], VERT_PS, B), frozen=frozen)
    emasks = D.edge_head_masks(seeds[2], counts, EDGE_PS, 512, ep._heads)
    probs = torch.zeros(B, max(c * (c - 1) // 2 for c in counts), dtype=torch.float64)
    rows = []
    for s, c in enumerate(counts):
        pr, idx = oracle.edge_forward(P, vo["vertices"][s:s + 1, :c, :], ep._heads, drop=emasks[s])
        rows.append(torch.nn.functional.pad(pr[0], (0, probs.shape[1] - pr.shape[1])))
        assert out["edge_indices"][s] == idx
    ref = {"vertices": vo["vertices"], "existence_probabilities": vo["existence_probabilities"],
           "edge_probs": torch.stack(rows), "global_features": gl}
    sum((ref[k] * cot[k].double()).sum() for k in cot).backward()
    fwd = H.out_errs(out, ref)
    errs = {}
    for n in P:
        if P[n].grad is None:
            assert n not in got, n
            continue
        errs[n] = H.elem_err(got[n], P[n].grad.numpy())
    worst = sorted(((e, n) for n, e in errs.items()), reverse=True)
    print(f"twelve sites (input seed {seed}): forward {fwd}; worst gradient elements", [(f"{e:.2e}", n) for e, n in worst[:5]])
    for k, (a, b) in fwd.items():
        assert a < TOL and b < TOL, (k, a, b)
    assert len(errs) == len(list(model.parameters())) - 4               # spatial_proj is never used
    bad = [(n, e) for n, e in errs.items() if not e <= TOL_X3]
    assert not bad, bad


# ----------------------------------------------------------------------------------------------------------------------
# plumbing, model level
# ----------------------------------------------------------------------------------------------------------------------
def _count_draws(monkeypatch):
    from wf3d.random import DropoutGenerator
    n = [0]
    orig = DropoutGenerator.draw

    def draw(self, out=None):
        n[0] += 1
        return orig(self, out)
    monkeypatch.setattr(DropoutGenerator, "draw", draw)
    return n


def _fwd(model, x, cnt, tseed):
    torch.manual_seed(tseed)
    with torch.no_grad():
        out = model(x, cnt)
    return out, torch.get_rng_state()


def test_edge_dropout_alone_draws_as_before_and_eval_draws_nothing(monkeypatch):
    from wf3d import config
    model = small_model().set_edge_layout("padded")      # eval mode runs on the predicted counts: any count is served
    x = torch.randn(2, 640, 8, generator=torch.Generator().manual_seed(1)).to(dev())
    cnt = torch.tensor([8, 5]).to(dev())
    draws = _count_draws(monkeypatch)
    # host mode: with the new sites at 0 the only value taken from torch's generator is the edge head's
    set_model_ps(model, (0.0,) * 4, (0.0,) * 4, (0.1,) * 4)
    out_a, state_a = _fwd(model, x, cnt, 7)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7)
        torch.empty((), dtype=torch.int64).random_()
        assert torch.equal(torch.get_rng_state(), state_a)               # exactly one draw
    assert draws[0] == 0
    # the sites of the other two modules switched on: two more values, drawn first (encoder, vertex head, edge head)
    set_model_ps(model, (0.1,) * 4, (0.1,) * 4, (0.1,) * 4)
    out_b, state_b = _fwd(model, x, cnt, 7)
    assert not torch.equal(state_b, state_a) and not torch.equal(out_b["vertices"], out_a["vertices"])
    assert [model.encoder.last_dropout_seed, model.vertex_predictor.last_dropout_seed] == three_host_seeds(7)[:2]
    # eval(): nothing drawn, and the bits of a model whose sites are all 0
    state = torch.get_rng_state()
    out_e = model.eval()(x, cnt)
    assert torch.equal(torch.get_rng_state(), state) and draws[0] == 0
    set_model_ps(model, (0.0,) * 4, (0.0,) * 4, (0.0,) * 4)
    out_0 = model(x, cnt)
    model.train()
    out_t = _fwd(model, x, cnt, 7)[0]
    model.eval()
    for k in ("vertices", "existence_probabilities", "edge_probs", "global_features"):
        assert torch.equal(out_e[k], out_0[k]), k
    model.train()
    for k in ("vertices", "existence_probabilities", "edge_probs", "global_features"):
        if k != "edge_probs":      # (the edge rows follow the target counts in train mode, the predicted ones in eval)
            assert torch.equal(out_t[k], out_0[k]), k                    # train mode at p = 0 everywhere: the same launches
    # device mode: one draw per module with an active site
    old = config.dropout_rng()
    config.set_dropout_rng("device")
    try:
        set_model_ps(model, (0.0,) * 4, (0.0,) * 4, (0.1,) * 4)
        _fwd(model, x, cnt, 7)
        assert draws[0] == 1
        set_model_ps(model, (0.0, 0.0, 0.2, 0.0), (0.0,) * 4, (0.1,) * 4)
        _fwd(model, x, cnt, 7)
        assert draws[0] == 3
        set_model_ps(model, (0.1,) * 4, (0.1,) * 4, (0.1,) * 4)
        _fwd(model, x, cnt, 7)
        assert draws[0] == 6
        model.eval()(x, cnt)
        assert draws[0] == 6
    finally:
        config.set_dropout_rng(old)
        set_model_ps(model, (0.0,) * 4, (0.0,) * 4, (0.1,) * 4).train()


def test_model_stream_setting_is_left_while_an_encoder_site_is_active():
    from wf3d import config
    model = set_model_ps(small_model(), (0.0, 0.3, 0.0, 0.0), (0.0,) * 4, (0.0,) * 4)
    x = torch.randn(2, 640, 8, generator=torch.Generator().manual_seed(1)).to(dev())
    cnt = torch.tensor([8, 5]).to(dev())
    old = config.inference()
    try:
        want, _ = _fwd(model, x, cnt, 9)
        config.set_inference("stream")
        got, _ = _fwd(model, x, cnt, 9)
        set_model_ps(model, (0.0,) * 4, (0.0,) * 4, (0.0,) * 4)
        plain, _ = _fwd(model, x, cnt, 9)                                # no site: the stream path serves it
    finally:
        config.set_inference(old)
    for k in ("vertices", "existence_probabilities", "edge_probs", "global_features"):
        assert torch.equal(got[k], want[k]), k
    assert not torch.equal(got["global_features"], plain["global_features"])


# ----------------------------------------------------------------------------------------------------------------------
# capture
# ----------------------------------------------------------------------------------------------------------------------
def _words(t):
    return [int(w) & 0xFFFFFFFF for w in t.cpu().tolist()]


def test_captured_step_draws_fresh_encoder_and_vertex_masks_and_equals_eager():
    from losses.WireframeLoss import WireframeLoss
    from models.PointCloudToWireframe import PointCloudToWireframe
    from wf3d import config
    from wf3d.optim import ClipAdam
    from wf3d.random import default_generator
    B, N, V = 3, 2560, 38                             # the sizes of tests/test_graph_step_gpu.py's whole-step test
    old = config.dropout_rng()
    config.set_dropout_rng("device")
    try:
        torch.manual_seed(0)
        gen = default_generator(dev())
        model = PointCloudToWireframe(8, V).to(dev()).set_dropout(0.1).set_encoder_dropout(0.1).set_vertex_dropout(0.1)
        model.set_edge_layout("padded").train()
        model.vertex_predictor.ensure_point_pool_proj(1024, dev())
        twin = copy.deepcopy(model)
        g = torch.Generator().manual_seed(1)
        x = torch.randn(B, N, 8, generator=g).to(dev())
        counts = torch.tensor([38, 21, 30]).to(dev())
        E_ = V * (V - 1) // 2
        tg = {"vertices": torch.randn(B, V, 3, generator=g).to(dev()),
              "vertex_existence": (torch.arange(V)[None] < counts.cpu()[:, None]).float().to(dev()),
              "edge_labels": (torch.rand(B, E_, generator=g) > 0.8).float().to(dev()), "vertex_counts": counts}
        crit = WireframeLoss(assignment="device")

        def setup(m):
            return ClipAdam(m.parameters(), lr=1e-3, weight_decay=1e-6, max_norm=1.0, norm_params=m.parameters, capturable=True)

        def step(m, opt):
            opt.zero_grad()
            out = m(x, counts)
            crit(out, tg)["total_loss"].backward()
            opt.step()

        opt, opt2 = setup(model), setup(twin)
        start = gen.get_state()
        s = torch.cuda.Stream(dev())
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                step(model, opt)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step(model, opt)
        bufs = (model.encoder.last_dropout_seeds, model.vertex_predictor.last_dropout_seeds, model.edge_predictor.last_dropout_seeds)
        seen = []
        for _ in range(3):
            before = gen.get_state()
            graph.replay()
            torch.cuda.synchronize()
            ws = [_words(b) for b in bufs]
            for w in ws:
                assert w[1:] == D.site_seeds(w[0])
                assert w not in seen                                     # every module, every replay: fresh words
                seen.append(w)
            assert int(gen.get_state()[1]) == int(before[1]) + 3         # one draw per module
        torch.cuda.synchronize()
        gen_after = gen.get_state()
        # the eager twin from the same generator state: the model ran five steps (two warm-up steps and three replays;
        # the capture itself records launches and runs none)
        gen.set_state(start)
        for _ in range(5):
            step(twin, opt2)
        torch.cuda.synchronize()
        assert torch.equal(gen.get_state(), gen_after)
        assert [_words(m.last_dropout_seeds) for m in (twin.encoder, twin.vertex_predictor, twin.edge_predictor)] == ws
        named2 = dict(twin.named_parameters())
        for n, p in model.named_parameters():
            assert torch.equal(p, named2[n]), n
    finally:
        config.set_dropout_rng(old)
