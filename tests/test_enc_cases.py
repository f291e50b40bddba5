"""The yardstick of tests/test_encoder_cotangents_gpu.py held to itself on the CPU (tests/enc_cases.py): the packed
reference against the dense one, and the decision-frozen reference against the unfrozen one under its own decisions."""
import pytest
import torch

import enc_cases as E
from helpers import oracle


def _params(hidden, out, din=8, seed=3):
    shapes = {k: v for k, v in oracle.state_dict_shapes(din, 4, hidden, out).items() if k.startswith("encoder.")}
    g = torch.Generator().manual_seed(seed)
    P = {}
    for k, s in shapes.items():
        t = torch.randn(s, generator=g, dtype=torch.float64)
        if len(s) == 2:
            t = t / s[1] ** 0.5
        elif k.endswith(".weight"):
            t = 1.0 + 0.05 * t                      # a LayerNorm gamma
        else:
            t = 0.05 * t
        P[k] = t
    return P


def _leaf(P):
    return {k: v.clone().requires_grad_() for k, v in P.items()}


def _loss(outs, cot):
    return sum((o * cot[k].double()).sum() for k, o in zip(E.OUTS, outs))


@pytest.mark.parametrize("hidden,out", [([16, 12], 10), ([], 6)])
def test_packed_reference_equals_dense_at_equal_lengths(hidden, out):
    B, N = 3, 13
    P0 = _params(hidden, out)
    x = E.dense_input(7, B, N).double()
    cot = E.cotangents(11, {"g": (B, out), "pf": (B, N, out), "up": (B, 2 * out)})
    for frozen in (None, E.own_decisions(P0, x)):
        Pd, Pp = _leaf(P0), _leaf(P0)
        d = E.ref_dense(Pd, x, frozen)
        p = E.ref_packed(Pp, x.reshape(B * N, -1), [N] * B, frozen)
        assert torch.equal(d[0], p[0]) and torch.equal(d[1].reshape(B * N, out), p[1]) and torch.equal(d[2], p[2])
        _loss(d, cot).backward()
        _loss((p[0], p[1].reshape(B, N, out), p[2]), cot).backward()
        for k in Pd:
            a, b = Pd[k].grad, Pp[k].grad
            assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max()), k


def test_packed_reference_cloud_of_no_rows():
    """Such a cloud pools to zeros, its g is the fusion MLP of zeros, and the others' results do not notice it: what the
    per-point MLP and the pools give is bit-equal; the fusion MLP runs over four rows instead of three, which BLAS may
    sum in another order, so g and the gradients are held to 1e-12."""
    def close(x, y):
        x, y = x.detach(), y.detach()
        return float((x - y).abs().max()) <= 1e-12 * float(x.abs().max())

    P0 = _params([16], 8)
    pts = E.packed_input(5, [9, 4, 6]).double()
    Pa, Pb = _leaf(P0), _leaf(P0)
    a = E.ref_packed(Pa, pts, [9, 4, 6])
    b = E.ref_packed(Pb, pts, [9, 4, 0, 6])
    keep = [0, 1, 3]
    assert close(a[0], b[0][keep]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2][keep])
    assert not bool(b[2][2].any())
    zero = E.oracle.encoder_fusion(P0, torch.zeros(1, 16, dtype=torch.float64))
    assert close(zero[0], b[0][2])
    cot = E.cotangents(2, {"g": (3, 8), "pf": (19, 8), "up": (3, 16)})
    cb = {"g": torch.zeros(4, 8), "pf": cot["pf"], "up": torch.randn(4, 16)}
    cb["g"][keep], cb["up"][keep] = cot["g"], cot["up"]
    _loss(a, cot).backward()
    _loss(b, cb).backward()
    for k in Pa:
        assert close(Pa[k].grad, Pb[k].grad), k


@pytest.mark.parametrize("hidden,out", [([16, 12], 10), ([], 6)])
@pytest.mark.parametrize("packed", [False, True])
def test_frozen_reference_equals_unfrozen_under_its_own_decisions(hidden, out, packed):
    B, N = 3, 13
    P0 = _params(hidden, out)
    x = E.dense_input(9, B, N).double()
    frozen = E.own_decisions(P0, x)
    cot = E.cotangents(4, {"g": (B, out), "pf": (B * N, out) if packed else (B, N, out), "up": (B, 2 * out)})
    Pu, Pf = _leaf(P0), _leaf(P0)
    if packed:
        u = E.ref_packed(Pu, x.reshape(B * N, -1), [N] * B)
        f = E.ref_packed(Pf, x.reshape(B * N, -1), [N] * B, frozen)
    else:
        u, f = E.ref_dense(Pu, x), E.ref_dense(Pf, x, frozen)
    for a, b in zip(u, f):
        assert torch.equal(a, b)
    _loss(u, cot).backward()
    _loss(f, cot).backward()
    for k in Pu:
        assert torch.equal(Pu[k].grad, Pf[k].grad), k
    # and the decisions are live ones: both kinds of ReLU outcome, a cloud without a valid point, ties in the zero rows
    assert all(bool(m.any()) and not bool(m.all()) for m in frozen["relu"].values())
    assert bool((frozen["argmax"]["enc_masked"][1] == -1).all()) and bool((frozen["argmax"]["enc_masked"][0] >= 0).all())
