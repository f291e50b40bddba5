"""The fp64 model of the encoder's and the vertex head's dropout sites (tests/dropout_sites_model.py) against the
reference's own train-mode runs (tests/golden/dropout_sites.npz; tests/golden/make_golden_dropout_sites.py), at the
bounds tests/test_dropout_oracle.py holds the edge head's oracle to.  The fixture holds every mask of the reference's
forward; fed those masks, the model has to reproduce the reference's outputs and parameter gradients.  This pins WHERE
each mask goes — behind the ReLU of its block, and in vertex_mlp3 / vertex_mlp4 before the residual add — so that the GPU
tests comparing the kernels with this model under the kernels' own masks test the reference's semantics.

And the seed rule of the two modules (host mode): site k masks with (seed + 0x9E3779B9 k) mod 2^32, EdgeFn's rule for
k <= 4, pinned by value beyond."""
import numpy as np
import torch

import dropout_sites_model as M
import helpers as H
from helpers import oracle
from oracle import dropout as D
from refsummary import digest, violations
from test_dropout_oracle import masks
from test_oracle_vs_reference import check_grads, check_params

GOLD = None


def gold():
    global GOLD
    if GOLD is None:
        GOLD = H.load_golden("dropout_sites")
    return GOLD


def encoder_case():
    from models.PointNetEncoder import PointNetEncoder
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(31)
        m = PointNetEncoder(8, [32, 64], 16)
        x = torch.randn(2, 16, 8)
        x[0, 12:] = 0
    return m, x


def vertex_case():
    from models.VertexPredictor import VertexPredictor
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(32)
        m = VertexPredictor(512, 8)
        g = torch.randn(2, 512)
        pf = torch.randn(2, 6, 16)
        m.ensure_point_pool_proj(32, "cpu")          # the reference creates it here, in its first forward
    return m, g, pf


def test_fixture_records_every_site_with_its_own_p():
    g = gold()
    for key, n in (("enc", 2), ("vert", 4)):
        ps = [float(p) for p in g[key + ".sites_p"]]
        assert len(set(ps)) == n and int(g[key + ".nmasks"]) == n
        assert [float(g[f"{key}.mask{k}.p"]) for k in range(n)] == ps
        for k, m in enumerate(masks(g, key)):
            frac = float((m == 0).double().mean())
            assert abs(frac - ps[k]) < 6 * np.sqrt(ps[k] * (1 - ps[k]) / m.numel()) + 0.02, (key, k, frac)


def test_encoder_model_with_recorded_masks_matches_reference():
    g = gold()
    m, x = encoder_case()
    check_params(g, "enc", m)
    assert digest(x) == g["enc.x"]
    P = {"encoder." + k: t for k, t in oracle.params_from_module(m, dtype=torch.float64).items()}
    drop = dict(zip(M.encoder_sites(2), masks(g, "enc")))
    gl, pf, _ = M.ref_dense(P, x.double(), drop)
    assert violations(g, "enc.g", gl, 2e-6) == [] and violations(g, "enc.pf", pf, 2e-6) == []
    ((gl * torch.from_numpy(g["enc.cot.g"]).double()).sum() + (pf * torch.from_numpy(g["enc.cot.pf"]).double()).sum()).backward()
    check_grads(g, "enc", P, "encoder.", 1e-5, 1e-12)
    # the decisions taken under the masks are the run's own: frozen to them, nothing moves
    fz = M.own_decisions(P, x.double(), drop)
    gl2, pf2, _ = M.ref_dense(P, x.double(), drop, fz)
    assert torch.equal(pf2, pf) and torch.allclose(gl2, gl, rtol=0, atol=1e-13)
    # and the masks matter, at each site: without one the model is far from the reference's train-mode output
    with torch.no_grad():
        for site in drop:
            less = {s: v for s, v in drop.items() if s != site}
            assert violations(g, "enc.pf", M.ref_dense(P, x.double(), less)[1], 1e-3) != [], site
        # a site moved in front of its ReLU would still match (relu commutes with a non-negative scale): what the fixture
        # pins is the block it belongs to — the masks swapped between the sites cannot even be applied
        assert drop["mlp.3"].shape != drop["mlp.7"].shape


def test_vertex_model_with_recorded_masks_matches_reference():
    g = gold()
    m, gf, pf = vertex_case()
    check_params(g, "vert", m)
    assert digest(gf) == g["vert.g"] and digest(pf) == g["vert.pf"]
    P = {"vertex_predictor." + k: t for k, t in oracle.params_from_module(m, dtype=torch.float64).items()}
    drop = dict(zip(M.VERTEX_SITES, masks(g, "vert")))
    g64, pf64 = gf.double().requires_grad_(), pf.double().requires_grad_()
    out = M.vertex_forward(P, g64, pf64, 8, drop=drop)
    for k in ("vertices", "existence_probabilities"):
        assert violations(g, "vert.out." + k, out[k], 2e-6) == [], k
    assert np.array_equal(out["actual_vertex_counts"].numpy(), g["vert.out.actual_vertex_counts"])
    sum((out[k] * torch.from_numpy(g["vert.cot." + k]).double()).sum() for k in ("vertices", "existence_probabilities")).backward()
    assert violations(g, "vert.dg", g64.grad, 1e-5, 1e-12) == []
    assert violations(g, "vert.dpf", pf64.grad, 1e-5, 1e-12) == []
    check_grads(g, "vert", P, "vertex_predictor.", 1e-5, 1e-12)
    with torch.no_grad():
        for site in drop:
            less = {s: v for s, v in drop.items() if s != site}
            assert violations(g, "vert.out.vertices", M.vertex_forward(P, g64, pf64, 8, drop=less)["vertices"], 1e-3) != [], site

        # the placement before the residual add: masking the SUM relu(LN(z3)) + r1 instead is far from the reference
        def after_add(P, e_in):
            pre = "vertex_predictor."
            e = e_in + oracle._lin(P, pre + "point_pool_proj", torch.cat([pf64.mean(1), pf64.max(1).values], 1))
            a = M._block(P, pre + "vertex_mlp1.0", pre + "vertex_mlp1.1", e, "vertex_mlp1.3", drop, None, None)
            b = M._block(P, pre + "vertex_mlp2.0", pre + "vertex_mlp2.1", a, "vertex_mlp2.3", drop, None, None)
            c = M._block(P, pre + "vertex_mlp3.0", pre + "vertex_mlp3.1", b, None, None, None, None)
            c = (c + oracle._lin(P, pre + "residual_proj1", e)) * drop["vertex_mlp3.3"]
            d = M._block(P, pre + "vertex_mlp4.0", pre + "vertex_mlp4.1", c, None, None, None, None)
            d = (d + oracle._lin(P, pre + "residual_proj2", e)) * drop["vertex_mlp4.3"]
            return oracle._lin(P, pre + "final_layer", d).reshape(2, 8, 4)[:, :, :3]
        assert violations(g, "vert.out.vertices", after_add(P, g64), 1e-3) != []


def test_site_seed_rule():
    """Site k = 1, 2, ... of a module that drew `seed` masks with (seed + 0x9E3779B9 k) mod 2^32: oracle.dropout.site_seeds
    for the first four, and the same rule beyond (an encoder deeper than four hidden layers, host mode), by value."""
    for seed in (0, 1, 0x2545F491, 0xDEADBEEF, 2 ** 63 - 1, -5):
        assert M.site_seeds(seed, 4) == D.site_seeds(seed)
        assert M.site_seeds(seed, 7)[:4] == D.site_seeds(seed)
    assert M.site_seeds(0xDEADBEEF, 7) == [0x7CE538A8, 0x1B1CB261, 0xB9542C1A, 0x578BA5D3, 0xF5C31F8C, 0x93FA9945, 0x323212FE]
    # the Functions derive the same seeds from a Drop (no GPU needed: only the argument handling runs)
    from wf3d.functional import Drop, _take_drop
    params, ps, sd, words = _take_drop(("w", "b", Drop((0.1, 0.0, 0.2, 0.0, 0.0, 0.3, 0.0), 0xDEADBEEF)), 7, "test")
    assert params == ("w", "b") and words is None and list(sd) == M.site_seeds(0xDEADBEEF, 7)
    assert ps == (0.1, 0.0, 0.2, 0.0, 0.0, 0.3, 0.0)
    # no Drop, or one with every p = 0: nothing is active and no seed is used
    assert _take_drop(("w", "b"), 3, "test") == (("w", "b"), (0.0,) * 3, (0,) * 3, None)
    assert _take_drop(("w", Drop((0.0, 0.0), 123)), 2, "test") == (("w",), (0.0, 0.0), (0, 0), None)
    # device words serve four sites: an active fifth is refused, an inactive one is not
    w = torch.zeros(5, dtype=torch.int32)
    assert _take_drop((Drop((0.1, 0.1, 0.1, 0.1, 0.0), w),), 5, "test")[2] == (1, 2, 3, 4, 5)
    try:
        _take_drop((Drop((0.0, 0.0, 0.0, 0.0, 0.1), w),), 5, "test")
    except ValueError as e:
        assert "four" in str(e)
    else:
        raise AssertionError("an active fifth site passed with device seed words")


def test_modules_read_validate_and_record(monkeypatch):
    """What the two modules decide on the host, no GPU needed: eval mode and p = 0 draw nothing (torch's generator is not
    consumed); train mode with an active site draws one value per module and records it; p outside [0, 1) raises naming
    the site."""
    from models.PointNetEncoder import PointNetEncoder
    from models.VertexPredictor import VertexPredictor
    from models.PointCloudToWireframe import PointCloudToWireframe
    import pytest
    enc, vp = PointNetEncoder(8, [32, 64], 16), VertexPredictor(64, 4)
    for m in (enc, vp):
        state = torch.get_rng_state()
        assert m.train()._dropout("cpu") == ()                       # defaults: every p is 0
        assert torch.equal(torch.get_rng_state(), state)
    enc.mlp[7].p = 0.25
    vp.vertex_mlp3[3].p = 0.5
    for m, n, ps in ((enc, 2, (0.0, 0.25)), (vp, 4, (0.0, 0.0, 0.5, 0.0))):
        state = torch.get_rng_state()
        assert m.eval()._dropout("cpu") == () and torch.equal(torch.get_rng_state(), state)
        torch.manual_seed(9)
        want = int(torch.empty((), dtype=torch.int64).random_().item())
        torch.manual_seed(9)
        (d,) = m.train()._dropout("cpu")
        assert d.ps == ps and d.seed == want == m.last_dropout_seed
    enc.mlp[3].p = 1.0
    with pytest.raises(ValueError, match=r"mlp\.3"):
        enc._dropout_ps()
    vp.vertex_mlp4[3].p = -0.1
    with pytest.raises(ValueError, match=r"vertex_mlp4\.3"):
        vp._dropout_ps()
    assert enc.eval()._dropout_ps() == (0.0, 0.0)                    # eval mode does not look
    model = PointCloudToWireframe(8, 4)
    assert model.set_encoder_dropout(0.2) is model and model.set_vertex_dropout(0.3) is model
    assert model.encoder.train()._dropout_ps() == (0.2,) * 4
    assert model.vertex_predictor.train()._dropout_ps() == (0.3,) * 4
    assert model.edge_predictor.train()._dropout_ps() == (0.1,) * 4  # set_dropout's sites are not touched
