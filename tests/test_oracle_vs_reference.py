"""The CPU oracle (oracle/reference_cpu.py) against results recorded from the reference's own classes
(tests/golden/refcheck_model.npz, refcheck_sizes.npz; tests/golden/make_golden_refcheck.py).  The parameters are drawn
again here by the drop-in classes under the reference's seed and checked bit for bit against the reference's, so the
oracle runs on exactly the reference's parameters and inputs; its outputs and gradients are then held to the recorded
ones (tests/refsummary.py)."""
import numpy as np
import torch

import helpers as H
import refcases
from helpers import oracle
from refsummary import digest, violations


def check_params(gold, key, m):
    got = {n: digest(p) for n, p in m.named_parameters()}
    want = dict(zip(gold[key + ".names"], gold[key + ".digests"]))
    assert set(got) == set(want), (key, sorted(set(got) ^ set(want)))
    assert [n for n in want if got[n] != want[n]] == [], key


def check_grads(gold, key, P, prefix, rtol, atol=0.0):
    none = set(gold[key + ".none_grads"])
    bad = []
    for n in gold[key + ".names"]:
        g = P[prefix + n].grad
        if n in none:
            assert g is None, (key, n)
        else:
            bad += violations(gold, f"{key}.grad.{n}", g, rtol, atol)
    assert bad == [], bad


def test_oracle_matches_imported_reference():
    """In float64 on both sides (the reference's seeded float32 parameters, converted exactly), so that the float32
    summation order of the CPU at hand does not enter the comparison."""
    from models.PointCloudToWireframe import PointCloudToWireframe
    gold = H.load_golden("refcheck_model")
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(5)
        m = PointCloudToWireframe(8, 9)
        x = torch.randn(2, 150, 8)
        x[0, 100:] = 0
        m.vertex_predictor.ensure_point_pool_proj(1024, "cpu")     # the reference creates it here, in its forward
    assert np.array_equal(x.numpy(), gold["x"])
    check_params(gold, "params", m)
    cnt = torch.from_numpy(gold["counts"])
    P = oracle.params_from_module(m, dtype=torch.float64)
    assert set(P) == set(oracle.state_dict_shapes(8, 9)), "state_dict key table drifted"
    assert all(tuple(P[k].shape) == tuple(v) for k, v in oracle.state_dict_shapes(8, 9).items())
    o2 = oracle.model_forward(P, x.double(), cnt, 9, training=True)
    assert [len(e) for e in o2["edge_indices"]] == gold["edge_indices"].tolist()
    assert [p for e in o2["edge_indices"] for p in e] == gold["edge_indices.flat"].tolist()
    bad = []
    for k in refcases.MODEL_OUTPUTS:
        bad += violations(gold, "out." + k, o2[k], 2e-6)
    assert bad == [], bad
    c = {k: torch.from_numpy(gold["cot." + k]).double() for k in refcases.MODEL_COTANGENTS}
    sum((o2[k] * c[k]).sum() for k in c).backward()
    check_grads(gold, "params", P, "", 1e-5, 1e-12)


def test_oracle_matches_imported_reference_at_other_constructor_sizes():
    """The size sweeps of tests/test_model_gpu.py compare the kernels with the oracle at widths, depths, head counts and
    vertex counts that are not the model's: here the oracle itself is held to the reference's classes at those sizes."""
    from models.PointNetEncoder import PointNetEncoder
    from models.EdgePredictor import EdgePredictor
    from models.VertexPredictor import VertexPredictor
    gold = H.load_golden("refcheck_sizes")

    def same(key, name, a, tol):
        assert violations(gold, f"{key}.{name}", a, tol) == [], (key, name)

    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1)
        for i, (hidden, out) in enumerate(refcases.ENCODER_SIZES):
            key = f"enc{i}"
            m = PointNetEncoder(8, hidden, out)
            check_params(gold, key, m)
            x = torch.randn(3, 70, 8)
            x[:, ::9] = 0
            assert digest(x) == gold[key + ".x"], key
            P = {"encoder." + k: v for k, v in oracle.params_from_module(m).items()}
            g2, pf2 = oracle.encoder_forward(P, x)
            same(key, "g", g2, 2e-6)
            same(key, "pf", pf2, 2e-6)
            cg, cp = torch.randn_like(g2), torch.randn_like(pf2)
            assert [digest(cg), digest(cp)] == list(gold[key + ".cot"]), key
            ((g2 * cg).sum() + (pf2 * cp).sum()).backward()
            check_grads(gold, key, P, "encoder.", 2e-5)
        for i, (vd, hidden, heads, cnt) in enumerate(refcases.EDGE_SIZES):
            key = f"edge{i}"
            m = EdgePredictor(vd, hidden, heads)
            check_params(gold, key, m)
            v2 = torch.randn(1, cnt, vd, requires_grad=True)
            assert digest(v2) == gold[key + ".v"], key
            P = {"edge_predictor." + k: t for k, t in oracle.params_from_module(m).items()}
            p2, idx2 = oracle.edge_forward(P, v2, num_heads=heads)
            assert np.array(idx2, dtype=np.int64).reshape(-1, 2).tolist() == gold[key + ".idx"].tolist(), key
            same(key, "probs", p2, 2e-6)
            c = torch.randn_like(p2)
            assert [digest(c)] == list(gold[key + ".cot"]), key
            (p2 * c).sum().backward()
            same(key, "dv", v2.grad, 2e-5)
            check_grads(gold, key, P, "edge_predictor.", 2e-5)
        for i, (gdim, V) in enumerate(refcases.VERTEX_SIZES):
            key = f"vert{i}"
            m = VertexPredictor(gdim, V, 4)
            g2 = torch.randn(3, gdim, requires_grad=True)
            pf2 = torch.randn(3, 9, gdim, requires_grad=True)
            assert [digest(g2), digest(pf2)] == list(gold[key + ".inputs"]), key
            m.ensure_point_pool_proj(2 * gdim, "cpu")                 # the reference creates it here, in its forward
            check_params(gold, key, m)
            P = {"vertex_predictor." + k: t for k, t in oracle.params_from_module(m).items()}
            o2 = oracle.vertex_forward(P, g2, pf2, V, 4)
            same(key, "vertices", o2["vertices"], 2e-6)
            same(key, "existence_probabilities", o2["existence_probabilities"], 2e-6)
            assert np.array_equal(o2["actual_vertex_counts"].numpy(), gold[key + ".actual_vertex_counts"]), key
            cv, ce = torch.randn_like(o2["vertices"]), torch.randn_like(o2["existence_probabilities"])
            assert [digest(cv), digest(ce)] == list(gold[key + ".cot"]), key
            ((o2["vertices"] * cv).sum() + (o2["existence_probabilities"] * ce).sum()).backward()
            same(key, "dg", g2.grad, 2e-5)
            same(key, "dpf", pf2.grad, 2e-5)
            check_grads(gold, key, P, "vertex_predictor.", 2e-5)
