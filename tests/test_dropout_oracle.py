"""The dropout-aware CPU oracle (oracle/reference_cpu.py, drop=) against the reference's own train-mode runs
(tests/golden/dropout.npz; tests/golden/make_golden_dropout.py).  The fixture holds every mask torch drew in the
reference's forward; fed those masks, the oracle has to reproduce the reference's outputs and parameter gradients in
float64 as tightly as tests/test_oracle_vs_reference.py holds it at p = 0.  This pins WHERE the oracle applies each
mask (after vertex_proj's second LayerNorm, on the softmax weights, after each edge-MLP GELU) and with which scale, so
that the GPU tests comparing the kernels with the oracle under the kernels' own masks (tests/test_dropout_gpu.py) test
the reference's semantics."""
import numpy as np
import torch

import helpers as H
import refcases
from helpers import oracle
from oracle.dropout import SITES
from refsummary import digest, violations
from test_oracle_vs_reference import check_grads, check_params

GOLD = None


def gold():
    global GOLD
    if GOLD is None:
        GOLD = H.load_golden("dropout")
    return GOLD


def masks(g, key):
    """The recorded masks of `key`, pre-scaled by torch's 1/(1-p) (float64), in recording order."""
    out = []
    for n in range(int(g[key + ".nmasks"])):
        p = float(g[f"{key}.mask{n}.p"])
        shape = tuple(int(d) for d in g[f"{key}.mask{n}.shape"])
        bits = np.unpackbits(g[f"{key}.mask{n}.bits"], count=int(np.prod(shape))).reshape(shape).astype(bool)
        out.append(torch.from_numpy(bits).double() * (1.0 / (1.0 - p)))
    return out


def site_dict(ms, heads, bs):
    """Four consecutive recorded masks (one edge-head forward) -> the oracle's {site: mask}; torch's attention mask is
    [bs * heads, V, V] with batch-major rows, the oracle's [bs, heads, V, V]."""
    d = dict(zip(SITES, ms))
    a = d["attention"]
    d["attention"] = a.reshape(bs, heads, a.shape[-2], a.shape[-1])
    return d


def test_fixture_records_four_distinct_sites_per_forward():
    g = gold()
    ps = [float(p) for p in g["sites_p"]]
    assert len(set(ps)) == 4
    for key, calls in (("edge", 1), ("model", len(g["model.counts"]))):
        assert int(g[key + ".nmasks"]) == 4 * calls
        for n in range(4 * calls):
            assert float(g[f"{key}.mask{n}.p"]) == ps[n % 4]
        # each mask drops close to its own p (torch's Bernoulli draws, so a loose sanity bound)
        for n, m in enumerate(masks(g, key)):
            frac = float((m == 0).double().mean())
            assert abs(frac - ps[n % 4]) < 6 * np.sqrt(ps[n % 4] * (1 - ps[n % 4]) / m.numel()) + 0.02, (key, n, frac)


def test_oracle_with_recorded_masks_matches_reference_edge_head():
    """EdgePredictor(3, 512, 8), one batched forward of two samples: masks span the batch."""
    from models.EdgePredictor import EdgePredictor
    g = gold()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(21)
        m = EdgePredictor(3, 512, 8)
        v = torch.randn(2, 9, 3)
    check_params(g, "edge", m)
    assert digest(v) == g["edge.v"]
    P = {"edge_predictor." + k: t for k, t in oracle.params_from_module(m, dtype=torch.float64).items()}
    v64 = v.double().requires_grad_()
    drop = site_dict(masks(g, "edge"), 8, 2)
    probs, _ = oracle.edge_forward(P, v64, num_heads=8, drop=drop)
    assert violations(g, "edge.probs", probs, 2e-6) == []
    (probs * torch.from_numpy(g["edge.cot"]).double()).sum().backward()
    assert violations(g, "edge.dv", v64.grad, 1e-5, 1e-12) == []
    check_grads(g, "edge", P, "edge_predictor.", 1e-5, 1e-12)
    # and the masks matter: without them the oracle is far from the reference's train-mode output
    with torch.no_grad():
        p0, _ = oracle.edge_forward(P, v64, num_heads=8)
    assert violations(g, "edge.probs", p0, 1e-3) != []


def test_oracle_with_recorded_masks_matches_reference_model_ragged():
    """PointCloudToWireframe(8, 12) on a ragged batch: the reference's per-sample loop, one edge-head call per sample."""
    from models.PointCloudToWireframe import PointCloudToWireframe
    g = gold()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(22)
        m = PointCloudToWireframe(8, 12)
        x = torch.randn(3, 64, 8)
        x[0, 40:] = 0
        m.vertex_predictor.ensure_point_pool_proj(1024, "cpu")     # the reference creates it here, in its forward
    assert np.array_equal(x.numpy(), g["model.x"])
    check_params(g, "model", m)
    cnt = torch.from_numpy(g["model.counts"])
    ms = masks(g, "model")
    drop = [site_dict(ms[4 * s:4 * s + 4], 8, 1) for s in range(len(cnt))]
    P = oracle.params_from_module(m, dtype=torch.float64)
    out = oracle.model_forward(P, x.double(), cnt, 12, training=True, drop=drop)
    bad = []
    for k in refcases.MODEL_OUTPUTS:
        bad += violations(g, "model.out." + k, out[k], 2e-6)
    assert bad == [], bad
    c = {k: torch.from_numpy(g["model.cot." + k]).double() for k in refcases.MODEL_COTANGENTS}
    sum((out[k] * c[k]).sum() for k in c).backward()
    check_grads(g, "model", P, "", 1e-5, 1e-12)
