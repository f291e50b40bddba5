"""The loss-term kernels of csrc/loss.hip (loss_terms_kernel over host match lists, over a device assignment, and the latter's device-edge-width form)
fed by the test itself: the assignment is a RANDOM permutation per sample, not an optimal one, so the kernels are held
to what they are told and not to what the solver would have said.  Reference: float64 torch on the CPU with autograd —
SmoothL1 (beta = 1) over the pairs {(p, col4row[p]) : col4row[p] < count}, averaged over 3 x the batch's matches, and
the two nn.BCELoss means.  Shapes the other tests do not reach: target width != V in both directions, V > 256 (more than
one trip of the kernels' 256-wide loops), B > 64, no edge columns at all, the strided [B, V, 4][:, :, :3] view.

Bounds are those of tests/test_loss.py::test_device_loss_matches_the_cpu_oracle_at_other_shapes: each loss within
5e-6 x max(1, |ref|), each gradient tensor within 2e-5 of its largest element; gradients of unmatched predictions and
of edge columns past the common width are exactly 0."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WEIGHTS = (3.0, 1.0, 1.5)            # vertex, existence, edge: the kernels' order
# (B, V, Vt, Ep, Et, strided vertices)
SHAPES = [(1, 1, 1, 0, 0, False), (3, 5, 9, 10, 10, False), (3, 9, 5, 36, 20, False), (2, 320, 320, 600, 51040, False),
          (70, 4, 4, 6, 6, False), (4, 12, 12, 66, 66, True)]
IDS = ["B1_V1_noedges", "Vt_wider", "Vt_narrower", "V320", "B70", "strided_view"]


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(shape, all_zero=False):
    """Inputs of one shape (CPU, float32), a random permutation per sample and the match lists built from it."""
    B, V, Vt, Ep, Et, _ = shape
    g = torch.Generator().manual_seed(B * 100003 + V * 101 + Vt + int(all_zero))
    top = min(V, Vt)
    counts = torch.randint(0, top + 1, (B,), generator=g)
    counts[0] = top
    if B > 2:
        counts[1] = 0
    if all_zero:
        counts.zero_()
    c = {"pv": torch.randn(B, V, 3, generator=g) * 1.5,              # |d| on both sides of SmoothL1's beta
         "pe": torch.sigmoid(2.0 * torch.randn(B, V, generator=g)),
         "pp": torch.sigmoid(2.0 * torch.randn(B, Ep, generator=g)),
         "tv": torch.randn(B, Vt, 3, generator=g),
         "te": (torch.arange(V)[None, :] < counts[:, None]).float(),
         "tl": (torch.rand(B, Et, generator=g) > 0.7).float(),
         "counts": counts,
         "c4r": torch.stack([torch.randperm(V, generator=g) for _ in range(B)]).to(torch.int32)}
    matched = c["c4r"] < counts[:, None]                              # [B, V]
    bs, ps = matched.nonzero(as_tuple=True)
    c["matched"], c["m_b"], c["m_pred"], c["m_tgt"] = matched, bs, ps, c["c4r"][bs, ps].long()
    c["m_off"] = torch.cat([torch.zeros(1, dtype=torch.long), matched.sum(1).cumsum(0)])
    return c


@functools.lru_cache(maxsize=None)
def reference(shape, width, all_zero=False):
    """(losses [4], dverts, dexist, dedge) in float64 from autograd; `width` is the prediction's edge width."""
    c = case(shape, all_zero)
    B, V, Vt, Ep, Et, _ = shape
    pv, pe, pp = (c[k].double().requires_grad_() for k in ("pv", "pe", "pp"))
    n = len(c["m_b"])
    if n:
        lv = torch.nn.functional.smooth_l1_loss(pv[c["m_b"], c["m_pred"]], c["tv"].double()[c["m_b"], c["m_tgt"]],
                                                reduction="sum", beta=1.0) / (3 * n)
    else:
        lv = pv.sum() * 0.0
    le = torch.nn.BCELoss()(pe, c["te"].double())
    w = min(width, Ep, Et)
    ld = torch.nn.BCELoss()(pp[:, :w], c["tl"].double()[:, :w]) if w > 0 else pp.sum() * 0.0
    total = WEIGHTS[0] * lv + WEIGHTS[1] * le + WEIGHTS[2] * ld
    total.backward()
    return torch.stack([lv, le, ld, total]).detach(), pv.grad, pe.grad, pp.grad, w


def run(entry, shape, width=None, all_zero=False):
    from wf3d import ops
    c = case(shape, all_zero)
    B, V, Vt, Ep, Et, strided = shape
    d = {k: c[k].to(dev()) for k in ("pe", "pp", "tv", "te", "tl", "counts", "c4r")}
    if strided:                          # what the model passes: the first three columns of its [B, V, 4] output
        out4 = torch.full((B, V, 4), float("nan"))
        out4[:, :, :3] = c["pv"]
        pv = out4.to(dev())[:, :, :3]
        assert not pv.is_contiguous()
    else:
        pv = c["pv"].to(dev())
    if entry == "loss_terms":
        i32 = lambda t: t.to(torch.int32).to(dev())     # noqa: E731
        return ops.loss_terms(pv, d["pe"], d["pp"], d["tv"], d["te"], d["tl"], i32(c["m_pred"]), i32(c["m_tgt"]),
                              i32(c["m_off"]), len(c["m_b"]), WEIGHTS)
    ew = None if width is None else torch.tensor(width, dtype=torch.int64, device=dev())
    return ops.loss_terms_assigned(pv, d["pe"], d["pp"], d["tv"], d["te"], d["tl"], d["c4r"], d["counts"], WEIGHTS,
                                   edge_width=ew)


def check(got, shape, width, all_zero=False):
    c = case(shape, all_zero)
    Ep = shape[3]
    ref_l, ref_dv, ref_de, ref_dd, w = reference(shape, Ep if width is None else width, all_zero)
    losses, dv, de, dd = (t.cpu().double() for t in got)
    for k, name in enumerate(("vertex", "existence", "edge", "total")):
        err, lim = abs(float(losses[k]) - float(ref_l[k])), 5e-6 * max(1.0, abs(float(ref_l[k])))
        print(f"{name} loss {float(losses[k]):.9g} ref {float(ref_l[k]):.9g} err {err:.2e} limit {lim:.2e}")
        assert err < lim, name
    for name, a, b in (("dverts", dv, ref_dv), ("dexist", de, ref_de), ("dedge", dd, ref_dd)):
        assert a.shape == b.shape, name
        if b.numel() == 0:
            continue
        err, lim = float((a - b).abs().max()), 2e-5 * max(float(b.abs().max()), 1e-12)
        print(f"{name} max err {err:.2e} limit {lim:.2e}")
        assert err <= lim, name
    assert float(dv[~c["matched"]].abs().sum()) == 0.0                  # unmatched predictions: exactly 0
    assert float(dd[:, w:].abs().sum()) == 0.0                          # past the common width: exactly 0
    if len(c["m_b"]) == 0:
        assert float(losses[0]) == 0.0 and float(dv.abs().sum()) == 0.0


def widths(shape):
    Ep = shape[3]
    return sorted({0, Ep // 2, Ep + 3})


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_terms_from_host_match_lists(shape):
    check(run("loss_terms", shape), shape, None)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_terms_from_a_device_assignment(shape):
    check(run("loss_terms_assigned", shape), shape, None)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_terms_with_a_device_edge_width(shape):
    for width in widths(shape):
        check(run("loss_terms_assigned_ew", shape, width), shape, width)


@pytest.mark.parametrize("entry", ["loss_terms", "loss_terms_assigned", "loss_terms_assigned_ew"])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]], ids=[IDS[1], IDS[4]])
def test_batches_without_any_match(shape, entry):
    """Every count 0: the vertex loss is 0 and no coordinate gets a gradient."""
    width = shape[3] if entry.endswith("_ew") else None
    got = run(entry, shape, width, all_zero=True)
    assert len(case(shape, True)["m_b"]) == 0
    check(got, shape, width, all_zero=True)
