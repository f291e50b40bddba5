"""WireframeLoss(edge_targets="matched", edge_pos_weight=4, edge_focal_gamma=2) as a module, against a float64 composition
of its own parts: `last_assignment` -> wf3d.targets.matched_edge_labels (the numpy specification) -> the loss and its
gradients from float64 torch autograd.  B = 3, V = 8 and B = 2, V = 70 (the general assignment kernel), under both
`assignment=` values; through PointCloudToWireframe in the ragged and the padded (tail="skip") edge layouts; and captured
once in a graph and replayed on a batch with other counts and another assignment, equal to the eager result bit for bit.

Bounds are those of tests/test_loss_terms_forms_gpu.py: each loss within 5e-6 x max(1, |ref|), each gradient tensor
within 2e-5 of its largest element."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WEIGHTS = {"vertex_weight": 3.0, "existence_weight": 1.0, "edge_weight": 1.5}
BALANCE = {"edge_pos_weight": 4, "edge_focal_gamma": 2}


def dev():
    return torch.device("cuda:0")


def make_targets(B, V, seed, counts=None):
    """train.py-style targets at full label width from random wireframes: a ring of edges plus a few chords per sample."""
    from wf3d.targets import train_targets
    rng = np.random.default_rng(seed)
    counts = rng.integers(3, V + 1, size=B).tolist() if counts is None else counts
    vs = [rng.standard_normal((c, 3)).astype(np.float32) for c in counts]
    es = []
    for c in counts:
        ring = np.stack([np.arange(c), (np.arange(c) + 1) % c], 1) if c > 1 else np.zeros((0, 2), np.int64)
        es.append(np.concatenate([ring, rng.integers(0, max(c, 1), size=(c // 2, 2))]))
    return train_targets(vs, es, V, device=dev(), full_width=True)


def make_predictions(tgt, seed, width=None):
    """Each target vertex to 0.05 in a shuffled slot, random vertices in the other slots; random probabilities."""
    B, V = tgt["vertex_existence"].shape
    g = torch.Generator().manual_seed(seed)
    pv = torch.randn(B, V, 3, generator=g)
    for b, c in enumerate(tgt["vertex_counts"].tolist()):
        slots = torch.randperm(V, generator=g)[:c]
        pv[b, slots] = tgt["vertices"][b, :c].cpu() + 0.05 * torch.randn(c, 3, generator=g)
    E = V * (V - 1) // 2 if width is None else width
    return {"vertices": pv.to(dev()).requires_grad_(),
            "existence_probabilities": torch.rand(B, V, generator=g).clamp(0.02, 0.98).to(dev()).requires_grad_(),
            "edge_probs": torch.rand(B, E, generator=g).clamp(0.02, 0.98).to(dev()).requires_grad_()}


def composition64(pred, tgt, assignment, labels, common, w=4.0, gamma=2.0):
    """(losses [4], grads of vertices / existence / edge_probs) in float64 of the loss under `assignment` (slot p matched
    to assignment[b, p] iff below the count) with the edge term over the first `common` columns of `labels`."""
    pv, pe, pp = (pred[k].detach().cpu().double().requires_grad_() for k in ("vertices", "existence_probabilities", "edge_probs"))
    tv, te = tgt["vertices"].cpu().double(), tgt["vertex_existence"].cpu().double()
    a = torch.as_tensor(assignment).long()
    cnt = tgt["vertex_counts"].cpu().clamp(0, min(pv.shape[1], tv.shape[1]))
    matched = (a >= 0) & (a < cnt[:, None])
    bs, ps = matched.nonzero(as_tuple=True)
    lv = torch.nn.functional.smooth_l1_loss(pv[bs, ps], tv[bs, a[bs, ps]], reduction="sum", beta=1.0) / (3 * len(bs))
    le = torch.nn.BCELoss()(pe, te)
    p, t = pp[:, :common], torch.as_tensor(labels).double()[:, :common]
    live = ~((p == t) & ((t == 0) | (t == 1)))               # a padded head's zero columns: exactly 0, and 0 / 0 in autograd
    p, t = p[live], t[live]
    lp, lq = torch.log(p).clamp(min=-100.0), torch.log1p(-p).clamp(min=-100.0)
    ld = -(w * t * (1.0 - p) ** gamma * lp + (1.0 - t) * p ** gamma * lq).sum() / (pp.shape[0] * max(common, 1))
    total = WEIGHTS["vertex_weight"] * lv + WEIGHTS["existence_weight"] * le + WEIGHTS["edge_weight"] * ld
    total.backward()
    return torch.stack([lv, le, ld, total]).detach(), (pv.grad, pe.grad, pp.grad)


def assert_close(res, grads, ref_losses, ref_grads, what):
    got = [float(res[k].detach()) for k in ("vertex_loss", "existence_loss", "edge_loss", "total_loss")]
    for name, a, b in zip(("vertex", "existence", "edge", "total"), got, ref_losses.tolist()):
        err, lim = abs(a - b), 5e-6 * max(1.0, abs(b))
        print(f"{what}: {name} loss {a:.9g} ref {b:.9g} err {err:.2e} limit {lim:.2e}")
        assert err < lim, (what, name)
    for name, a, b in zip(("dverts", "dexist", "dedge"), grads, ref_grads):
        if a is None:
            continue
        err, lim = float((a.detach().cpu().double() - b).abs().max()), 2e-5 * float(b.abs().max())
        print(f"{what}: {name} max err {err:.2e} limit {lim:.2e}")
        assert err <= lim, (what, name)


@pytest.mark.parametrize("assignment", ["device", "scipy"])
@pytest.mark.parametrize("B, V", [(3, 8), (2, 70)])
def test_matched_focal_loss_equals_the_float64_composition(B, V, assignment):
    from losses.WireframeLoss import WireframeLoss
    from wf3d.targets import matched_edge_labels
    tgt = make_targets(B, V, seed=V)
    pred = make_predictions(tgt, seed=V + 1)
    crit = WireframeLoss(assignment=assignment, edge_targets="matched", **WEIGHTS, **BALANCE)
    res = crit(pred, tgt)
    res["total_loss"].backward()
    E = V * (V - 1) // 2
    a, labels = crit.last_assignment.cpu().numpy(), crit.last_edge_labels
    assert labels.is_cuda and labels.dtype == torch.float32 and tuple(labels.shape) == (B, E)
    spec = matched_edge_labels(tgt["edge_labels"].cpu().numpy(), a, tgt["vertex_counts"].cpu().numpy(), E)
    assert np.array_equal(labels.cpu().numpy(), spec)
    positional = tgt["edge_labels"].cpu().numpy()
    assert spec.sum() > 0 and not np.array_equal(spec, positional)        # a shuffled matching: the labels moved
    ref_l, ref_g = composition64(pred, tgt, a, spec, E)
    assert_close(res, [pred[k].grad for k in ("vertices", "existence_probabilities", "edge_probs")], ref_l, ref_g,
                 f"B{B} V{V} {assignment}")


def test_both_assignment_modes_agree_and_defaults_keep_no_labels():
    from losses.WireframeLoss import WireframeLoss
    tgt = make_targets(3, 8, seed=3)
    pred = make_predictions(tgt, seed=4)
    out = {}
    for mode in ("device", "scipy"):
        crit = WireframeLoss(assignment=mode, edge_targets="matched", **BALANCE)
        out[mode] = (float(crit(pred, tgt)["edge_loss"]), crit.last_edge_labels.cpu())
        plain = WireframeLoss(assignment=mode)
        plain(pred, tgt)
        assert plain.last_edge_labels is None
    assert torch.equal(out["device"][1], out["scipy"][1])
    assert abs(out["device"][0] - out["scipy"][0]) <= 1e-6 * max(1.0, abs(out["scipy"][0]))


@pytest.mark.parametrize("layout", ["ragged", "padded"])
def test_forward_and_backward_through_the_model(layout):
    from losses.WireframeLoss import WireframeLoss
    from models.PointCloudToWireframe import PointCloudToWireframe
    from wf3d.targets import matched_edge_labels
    B, N, V = 3, 64, 8
    torch.manual_seed(2)
    model = PointCloudToWireframe(8, V).to(dev()).train()
    if layout == "padded":
        model.set_edge_layout("padded", tail="skip")
    tgt = make_targets(B, V, seed=12, counts=[8, 3, 5])
    x = torch.randn(B, N, 8, generator=torch.Generator().manual_seed(3)).to(dev())
    out = model(x, tgt["vertex_counts"])
    out["edge_probs"].retain_grad()
    crit = WireframeLoss(edge_targets="matched", **WEIGHTS, **BALANCE)
    res = crit(out, tgt)
    res["total_loss"].backward()
    for n, p in model.named_parameters():
        assert p.grad is None or bool(torch.isfinite(p.grad).all()), n
    assert sum(float(p.grad.abs().sum()) for p in model.parameters() if p.grad is not None) > 0
    Ep = out["edge_probs"].shape[1]
    common = int(out["edge_width"]) if layout == "padded" else Ep
    assert (Ep, common) == ((V * (V - 1) // 2, 28) if layout == "padded" else (28, 28))
    a = crit.last_assignment.cpu().numpy()
    pair = out["edge_counts"].cpu().numpy() if layout == "padded" else None
    spec = matched_edge_labels(tgt["edge_labels"].cpu().numpy(), a, tgt["vertex_counts"].cpu().numpy(), Ep, pair)
    assert np.array_equal(crit.last_edge_labels.cpu().numpy(), spec) and spec.sum() > 0
    ref_l, ref_g = composition64(out, tgt, a, spec, common)
    assert_close(res, [None, None, out["edge_probs"].grad], ref_l, ref_g, layout)
    assert bool(torch.isfinite(out["edge_probs"].grad).all())


def test_captured_matched_loss_replays_bit_for_bit():
    """Forward and backward captured once over static buffers, a padded head's device counts and width among them; the
    replay on a second batch with other counts, another assignment and another width equals the eager result."""
    from losses.WireframeLoss import WireframeLoss
    B, V = 3, 8
    E = V * (V - 1) // 2

    def batch(seed, counts, width):
        tgt = make_targets(B, V, seed=seed, counts=counts)
        pred = make_predictions(tgt, seed=seed + 1)
        pred["edge_counts"] = torch.tensor(counts, dtype=torch.int64, device=dev())
        pred["edge_width"] = torch.tensor(width, dtype=torch.int64, device=dev())
        return pred, tgt
    pred, tgt = batch(30, [8, 4, 6], E)
    crit = WireframeLoss(edge_targets="matched", **WEIGHTS, **BALANCE)
    leaves = [pred[k] for k in ("vertices", "existence_probabilities", "edge_probs")]

    def step(c=crit):
        res = c(pred, tgt)
        return res["total_loss"], torch.autograd.grad(res["total_loss"], leaves), c.last_edge_labels, c.last_assignment
    s = torch.cuda.Stream(dev())
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        total, grads, labels, assignment = step()
    first = (labels.clone(), assignment.clone())
    new_pred, new_tgt = batch(40, [3, 8, 5], 21)
    with torch.no_grad():
        for d, n in ((pred, new_pred), (tgt, new_tgt)):
            for key, t in n.items():
                d[key].copy_(t)
    graph.replay()
    torch.cuda.synchronize()
    e_total, e_grads, e_labels, e_assignment = step(WireframeLoss(edge_targets="matched", **WEIGHTS, **BALANCE))
    torch.cuda.synchronize()
    assert torch.equal(total, e_total) and torch.equal(labels, e_labels) and torch.equal(assignment, e_assignment)
    for a, b in zip(grads, e_grads):
        assert torch.equal(a, b)
    assert not torch.equal(first[0], labels) and not torch.equal(first[1], assignment)
    assert float(grads[2][:, 21:].abs().sum()) == 0.0 and float(grads[2][:, :21].abs().sum()) > 0
