"""The CPU oracle at coincident vertices: the edge head's distance |c_i - c_j| is 0 there, and torch's norm backward
gives a zero gradient at 0 (the reference, models/EdgePredictor.py:130, uses torch.norm; the oracle vector_norm), not
NaN.  This pins the oracle to that rule; tests/test_degenerate_values_gpu.py holds the kernels to the oracle."""
import torch

import helpers as H
from helpers import detgen, oracle


def _params():
    arrs = detgen.fill_state_dict(H.sub_shapes("edge_predictor.", edge_hidden=64), 4)
    return {"edge_predictor." + k: torch.tensor(v, dtype=torch.float64).requires_grad_() for k, v in arrs.items()}


def _grads(v):
    P = _params()
    v = v.clone().requires_grad_()
    probs, _ = oracle.edge_forward(P, v, num_heads=2)
    cot = torch.randn(probs.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    (probs * cot).sum().backward()
    return probs, v.grad, {k: p.grad for k, p in P.items() if p.grad is not None}


def test_oracle_gradients_are_finite_at_coincident_vertices():
    g = torch.Generator().manual_seed(0)
    two_same = torch.randn(1, 6, 3, generator=g, dtype=torch.float64)
    two_same[0, 4] = two_same[0, 1]
    for v in (two_same, torch.zeros(1, 4, 3, dtype=torch.float64)):
        probs, dv, dP = _grads(v)
        assert bool(torch.isfinite(probs).all()) and bool(torch.isfinite(dv).all())
        assert len(dP) == 24
        for k, t in dP.items():
            assert bool(torch.isfinite(t).all()), k
        assert float(dv.abs().max()) > 0                  # the coordinate and embedding paths still carry a gradient


def test_distance_term_has_zero_gradient_at_zero():
    """The rule itself, for both spellings of the norm."""
    for norm in (lambda d: torch.norm(d, dim=-1), lambda d: torch.linalg.vector_norm(d, dim=-1)):
        c = torch.zeros(2, 3, dtype=torch.float64, requires_grad=True)
        norm(c[0:1] - c[1:2]).sum().backward()
        assert not c.grad.any()
