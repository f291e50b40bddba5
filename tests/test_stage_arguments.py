"""What the three modules hand to their stage Functions, no GPU needed.

Which parameter sits in which positional slot — and so receives which gradient — is pinned here against state_dict key
lists written out literally (the order of the list literals the model files held before the blocks had names),
independently of the named tuples of wf3d.functional.  And the one module-side dropout function (wf3d.dropout.module_drop):
when it draws, what it records and what it refuses."""
import pytest
import torch

ENCODER_MLP_KEYS = ["mlp.0.weight", "mlp.0.bias", "mlp.1.weight", "mlp.1.bias",
                    "mlp.4.weight", "mlp.4.bias", "mlp.5.weight", "mlp.5.bias",
                    "mlp.8.weight", "mlp.8.bias", "mlp.9.weight", "mlp.9.bias",
                    "mlp.12.weight", "mlp.12.bias", "mlp.13.weight", "mlp.13.bias",
                    "mlp.16.weight", "mlp.16.bias"]
FUSION_KEYS = ["feature_fusion.0.weight", "feature_fusion.0.bias", "feature_fusion.1.weight", "feature_fusion.1.bias",
               "feature_fusion.3.weight", "feature_fusion.3.bias", "feature_fusion.4.weight", "feature_fusion.4.bias",
               "feature_fusion.6.weight", "feature_fusion.6.bias"]
VERTEX_KEYS = ["vertex_mlp1.0.weight", "vertex_mlp1.0.bias", "vertex_mlp1.1.weight", "vertex_mlp1.1.bias",
               "vertex_mlp2.0.weight", "vertex_mlp2.0.bias", "vertex_mlp2.1.weight", "vertex_mlp2.1.bias",
               "vertex_mlp3.0.weight", "vertex_mlp3.0.bias", "vertex_mlp3.1.weight", "vertex_mlp3.1.bias",
               "vertex_mlp4.0.weight", "vertex_mlp4.0.bias", "vertex_mlp4.1.weight", "vertex_mlp4.1.bias",
               "final_layer.weight", "final_layer.bias",
               "residual_proj1.weight", "residual_proj1.bias", "residual_proj2.weight", "residual_proj2.bias"]
VERTEX_POOL_KEYS = ["point_pool_proj.weight", "point_pool_proj.bias"]
EDGE_KEYS = ["vertex_proj.0.weight", "vertex_proj.0.bias", "vertex_proj.1.weight", "vertex_proj.1.bias",
             "vertex_proj.3.weight", "vertex_proj.3.bias", "vertex_proj.4.weight", "vertex_proj.4.bias",
             "attention.in_proj_weight", "attention.in_proj_bias", "attention.out_proj.weight", "attention.out_proj.bias",
             "edge_mlp.0.weight", "edge_mlp.0.bias", "edge_mlp.1.weight", "edge_mlp.1.bias",
             "edge_mlp.4.weight", "edge_mlp.4.bias", "edge_mlp.5.weight", "edge_mlp.5.bias",
             "edge_mlp.8.weight", "edge_mlp.8.bias", "edge_mlp.10.weight", "edge_mlp.10.bias"]


def assert_slots(module, params, keys):
    """The tensors of `params`, in order, ARE the module's parameters of `keys` (the objects, not equal copies)."""
    sd = module.state_dict(keep_vars=True)
    got = [p for p in params if p is not None]
    assert len(got) == len(keys)
    for i, (p, k) in enumerate(zip(got, keys)):
        assert p is sd[k], (i, k)


def test_encoder_slots():
    from models.PointNetEncoder import PointNetEncoder
    enc = PointNetEncoder(8, [16, 32, 24, 16], 8)
    assert_slots(enc, enc._mlp_params(), ENCODER_MLP_KEYS)
    assert_slots(enc, enc._fusion_params(), FUSION_KEYS)
    shallow = PointNetEncoder(8, [16, 32], 8)
    assert_slots(shallow, shallow._mlp_params(), ENCODER_MLP_KEYS[:8] + ["mlp.8.weight", "mlp.8.bias"])


def test_vertex_slots():
    from models.VertexPredictor import VertexPredictor
    vp = VertexPredictor(64, 4)
    assert_slots(vp, vp._param_list(False), VERTEX_KEYS)
    vp.ensure_point_pool_proj(32, "cpu")
    assert_slots(vp, vp._param_list(True), VERTEX_KEYS + VERTEX_POOL_KEYS)
    assert_slots(vp, vp._param_list(False), VERTEX_KEYS)                  # the lazy layer exists and is not asked for
    assert list(vp._param_list(True)[:22]) == list(vp._param_list(False)[:22])


def test_edge_slots():
    from models.EdgePredictor import EdgePredictor
    ep = EdgePredictor(3, 64, 2)
    assert_slots(ep, ep._param_list(), EDGE_KEYS)


def test_block_sizes_and_layer_records():
    from wf3d import functional as F
    assert [len(t._fields) for t in (F.FusionParams, F.VertexParams, F.EdgeParams)] == [10, 24, 24]
    assert len(set(F.VertexParams._fields)) == 24 and len(set(F.EdgeParams._fields)) == 24
    flat = list(range(10))                                                # two hidden layers and the output layer
    layers = F.mlp_layers(flat, 2)
    assert [tuple(layer) for layer in layers] == [(0, 1, 2, 3), (4, 5, 6, 7), (8, 9, None, None)]
    # gradients set by name come out in field order, None where none was set; a name the block lacks is refused
    G = F.MlpLayerGrads()
    G.beta, G.W = "dbeta", "dW"
    assert G.out() == ["dW", None, None, "dbeta"]
    G = F.EdgeGrads()
    G.M5g, G.M5b = "dgamma", "dbeta"
    out = G.out()
    assert len(out) == 24 and out[18:20] == ["dgamma", "dbeta"] and out.count(None) == 22
    with pytest.raises(AttributeError):
        G.M6w = 1


# ----------------------------------------------------------------------------------------------------------------------
# wf3d.dropout.module_drop
# ----------------------------------------------------------------------------------------------------------------------
class Owner:
    training = True
    last_dropout_seed = last_dropout_seeds = None


def sites(*ps):
    return tuple((f"site{k}", p) for k, p in enumerate(ps))


def test_eval_mode_and_all_zero_sites_draw_nothing():
    from wf3d.dropout import module_drop, site_ps
    o = Owner()
    state = torch.get_rng_state()
    assert module_drop(o, "stage", sites(0.0, 0.0, 0.0), "cpu") == ()
    o.training = False
    assert module_drop(o, "stage", sites(0.5, 2.0), "cpu") == ()         # eval mode does not look at p
    assert site_ps(o, "stage", sites(0.5, 2.0)) == (0.0, 0.0)
    assert torch.equal(torch.get_rng_state(), state)
    assert o.last_dropout_seed is None and o.last_dropout_seeds is None


def test_one_active_site_consumes_one_host_draw_and_records_it():
    from wf3d.dropout import Drop, module_drop
    o = Owner()
    torch.manual_seed(9)
    want = int(torch.empty((), dtype=torch.int64).random_().item())
    after = torch.get_rng_state()
    torch.manual_seed(9)
    (d,) = module_drop(o, "stage", sites(0.0, 0.25, 0.0), "cpu")
    assert torch.equal(torch.get_rng_state(), after)                      # exactly one draw
    assert isinstance(d, Drop) and d.ps == (0.0, 0.25, 0.0) and d.seed == want == o.last_dropout_seed
    assert o.last_dropout_seeds is None


def test_the_edge_head_records_its_host_seed():
    from models.EdgePredictor import EdgePredictor
    ep = EdgePredictor(3, 64, 2).train()
    torch.manual_seed(4)
    want = int(torch.empty((), dtype=torch.int64).random_().item())
    torch.manual_seed(4)
    (d,) = ep._dropout("cpu")
    assert d.ps == (0.1, 0.1, 0.1, 0.1) and d.seed == want == ep.last_dropout_seed


@pytest.mark.parametrize("p", [1.0, -0.1, 1.5])
def test_p_outside_the_half_open_interval_raises_naming_the_site(p):
    from wf3d.dropout import module_drop
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match=r"Owner: dropout p = .* at site2 is not supported by the HIP stage in train mode"):
        module_drop(Owner(), "stage", sites(0.1, 0.0, p), "cpu")
    assert torch.equal(torch.get_rng_state(), state)


def test_device_words_serve_four_sites():
    from wf3d import config
    from wf3d.dropout import module_drop
    old = config.dropout_rng()
    config.set_dropout_rng("device")
    try:
        o = Owner()
        with pytest.raises(ValueError, match=r"four dropout sites; site4 is active"):
            module_drop(o, "stage", sites(0.1, 0.0, 0.0, 0.0, 0.2), "cpu")
        assert o.last_dropout_seeds is None
        assert module_drop(o, "stage", sites(0.0, 0.0, 0.0, 0.0, 0.0), "cpu") == ()
    finally:
        config.set_dropout_rng(old)
