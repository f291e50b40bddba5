"""oracle/chunked.py on the CPU: the oracle run a few samples at a time gives the unchunked run's outputs and parameter
gradients (no operation of the model mixes samples), with decision-frozen masks and dropout masks sliced per chunk.
tests/test_bench_configs_gpu.py relies on it at the benchmark's sizes, on the GPU."""
import numpy as np
import pytest
import torch

import helpers as H
from helpers import oracle
from oracle import detgen
from oracle import dropout as D
from oracle.chunked import COT_KEYS, model_forward_chunked, slice_frozen

B, N, V, COUNTS = 3, 24, 6, [6, 2, 4]
WIDTHS = dict(hidden_dims=(32, 64), output_dim=32, edge_hidden=64)


def _case():
    arrs = detgen.fill_state_dict(oracle.state_dict_shapes(8, V, **WIDTHS), 5)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, N, 8, generator=g, dtype=torch.float64)
    x[0, N - N // 4:] = 0.0
    P0 = oracle.params_from_numpy(arrs, dtype=torch.float64)
    # decisions of another run (a random point): masks of every LayerNorm + ReLU, arg-max rows (-1 = none)
    relu = {}
    for name, shape in oracle.state_dict_shapes(8, V, **WIDTHS).items():
        if not name.endswith(".weight") or len(shape) != 1 or "edge_predictor" in name:
            continue
        ln = name[:-len(".weight")]
        rows = B * N if ln.startswith("encoder.mlp.") else B
        relu[ln] = torch.rand(rows, shape[0], generator=g) > 0.4
    C = WIDTHS["output_dim"]
    argmax = {k: torch.randint(-1, N, (B, C), generator=g) for k in ("enc_masked", "vert_unmasked")}
    frozen = {"relu": relu, "argmax": argmax}
    cot = {"vertices": torch.randn(B, V, 3, generator=g, dtype=torch.float64),
           "existence_probabilities": torch.randn(B, V, generator=g, dtype=torch.float64),
           "edge_probs": torch.randn(B, V * (V - 1) // 2, generator=g, dtype=torch.float64)}
    return P0, x, frozen, cot


def _params(P0):
    return {k: v.detach().clone().requires_grad_() for k, v in P0.items()}


def test_slice_frozen_rows():
    _, _, frozen, _ = _case()
    s = slice_frozen(frozen, 1, 3, N)
    assert torch.equal(s["relu"]["encoder.mlp.1"], frozen["relu"]["encoder.mlp.1"][N:3 * N])
    assert torch.equal(s["relu"]["vertex_predictor.vertex_mlp2.1"], frozen["relu"]["vertex_predictor.vertex_mlp2.1"][1:3])
    assert torch.equal(s["argmax"]["enc_masked"], frozen["argmax"]["enc_masked"][1:3])


def test_edge_head_masks_sample_range_uses_batch_offsets():
    whole = D.edge_head_masks(0xDEADBEEF, COUNTS, (0.1,) * 4, 64, 8)
    part = D.edge_head_masks(0xDEADBEEF, COUNTS, (0.1,) * 4, 64, 8, 1, 3)
    assert len(part) == 2
    for a, b in zip(whole[1:], part):
        assert sorted(a) == sorted(b)
        for k in a:
            assert np.array_equal(a[k], b[k])


@pytest.mark.parametrize("frozen_on", [False, True])
@pytest.mark.parametrize("chunk", [1, 2])
def test_chunked_equals_unchunked(chunk, frozen_on):
    P0, x, frozen, cot = _case()
    frozen = frozen if frozen_on else None
    counts = torch.tensor(COUNTS)

    def masks(s0, s1):
        return D.edge_head_masks(0x12345, COUNTS, (0.05, 0.1, 0.2, 0.3), 64, 8, s0, s1)

    P = _params(P0)
    ref = oracle.model_forward(P, x, counts, V, training=True, frozen=frozen, drop=masks(0, B))
    sum((ref[k].double() * cot[k]).sum() for k in COT_KEYS).backward()
    Pc = _params(P0)
    got = model_forward_chunked(Pc, x, counts, V, chunk, cot=cot, frozen=frozen, drop=masks)
    assert got["edge_indices"] == ref["edge_indices"]
    for k, (a, b) in H.out_errs(got, ref).items():
        assert a <= 1e-12 and b <= 1e-12, (k, a, b)
    assert torch.equal(got["actual_vertex_counts"], ref["actual_vertex_counts"])
    n = 0
    for name, t in P.items():
        if t.grad is None:
            assert Pc[name].grad is None, name
            continue
        n += 1
        assert H.elem_err(Pc[name].grad.numpy(), t.grad.numpy()) <= 1e-12, name
    assert n == len(P) - 4                       # all but the never-used spatial_proj
