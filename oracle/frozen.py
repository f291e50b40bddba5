"""Decision capture for the decision-frozen gradient check (TEST INFRASTRUCTURE, like the rest of oracle/: used by
tests/test_frozen_grad_gpu.py, tests/test_encoder_cotangents_gpu.py and __graft_entry__.smoke()).

A ReLU / arg-max network's gradient is piecewise constant in its pre-activations; to compare a HIP backward with an fp64
oracle element by element, the oracle is run with the HIP forward's own 0/1 decisions (oracle.reference_cpu.model_forward
(frozen=...)).  This module reads those decisions off the autograd nodes of a PointCloudToWireframe output dict
(capture_decisions) or of a PointNetEncoder's outputs alone (capture_encoder_decisions)."""


def _sx8_positive(h_s, device="cpu"):
    """ReLU decision of the forward kernel itself, read off the sx8 operand it wrote: h > 0  <=>  its bf16 high part > 0
    (bf16 keeps fp32's exponent range, so no positive value rounds to zero)."""
    import torch
    R, C = h_s.shape
    planes = h_s.contiguous().view(torch.bfloat16).view(R, C // 8, 16)
    return (planes[:, :, :8] > 0).reshape(R, C).to(device)


def capture_decisions(out, model, border=5e-7, kernel_masks=False, device="cpu"):
    """Read the piecewise-constant decisions the HIP forward took (ReLU masks of every LayerNorm+ReLU,
    pool arg-max rows) off the autograd nodes of a PointCloudToWireframe output dict, BEFORE backward.

    Returns (frozen dict for oracle.model_forward(frozen=...), n_border): n_border counts activations
    whose LayerNorm output lies within `border` of 0 — there the mask recomputed here could differ from
    the one the kernels take (they evaluate the same fp32 expression in their own order), so a
    decision-frozen comparison is only meaningful on inputs with n_border == 0.

    kernel_masks=True: for the per-point layers whose activated output exists as an sx8 operand (bf16x3 mode), the mask
    is read from that operand instead — the forward kernel's own decision, exact whatever the margin — and those layers
    do not count towards n_border.  (Batches of thousands of points always contain activations within 5e-7 of 0.)

    device: where the masks and arg-max rows are put (default the CPU; the model's device keeps them where they are,
    for an oracle run on the GPU: at B = 32, N = 4096 the per-point masks alone are 600 MB)."""
    frozen, n_border, _ = capture_encoder_decisions(out["global_features"], model.encoder, border, kernel_masks, device)
    relu = frozen["relu"]
    sd = model.state_dict()
    vfn = out["existence_probabilities"].grad_fn
    assert type(vfn).__name__.startswith("VertexFn")
    pooled_v, e, z1, s1, z2, s2, z3, s3v, c, z4, s4, d = vfn.saved
    for k, (z, s) in enumerate(((z1, s1), (z2, s2), (z3, s3v), (z4, s4)), start=1):
        name = f"vertex_predictor.vertex_mlp{k}.1"
        relu[name], nb = _ln_mask(z, *s, sd[name + ".weight"], sd[name + ".bias"], border, device)
        n_border += nb
    return frozen, n_border


def _ln_mask(z, mu, rs, g, b, border, device):
    """(ReLU mask of LayerNorm(z) recomputed in fp64 from the saved pre-activation and row statistics, number of its
    elements within `border` of 0)."""
    v = ((z.double() - mu.double()[:, None]) * rs.double()[:, None]) * g.double() + b.double()
    return (v > 0).to(device), int((v.abs() < border).sum())


def capture_encoder_decisions(g, encoder, border=5e-7, kernel_masks=False, device="cpu", rows=None):
    """capture_decisions for the encoder alone: `g` is the global vector PointNetEncoder.encode / encode_packed returned
    (or a model's out["global_features"]), `encoder` the PointNetEncoder.  The decisions are read off g.grad_fn (the
    FusionFn node) and the EncoderFn* node in front of it, BEFORE backward.

    Returns (frozen, n_border, node): frozen = {"relu": masks of encoder.mlp.{4i+1} [rows, width] and of
    encoder.feature_fusion.{1,4} [B, width], "argmax": {"enc_masked", "vert_unmasked"} [B, C] int64 (-1 = none; local to
    the cloud for a packed batch, as the kernels record them)}, n_border as capture_decisions counts it (same rule, same
    kernel_masks option), node = the EncoderFn* node (its .routes and .live say which kernels ran).

    rows: only the first `rows` point rows are looked at and returned (a packed batch's live total: the rows behind it
    are pad rows, which a run under a live-row count does not even write)."""
    relu, n_border = {}, 0
    sd = encoder.state_dict()

    def mask(name, z, mu, rs):
        nonlocal n_border
        relu["encoder." + name], nb = _ln_mask(z, mu, rs, sd[name + ".weight"], sd[name + ".bias"], border, device)
        n_border += nb

    ffn = g.grad_fn
    assert type(ffn).__name__.startswith("FusionFn")
    efn = ffn.next_functions[0][0]
    assert type(efn).__name__.startswith("EncoderFn")
    x2, valid, zs, stats, hs, arg_m, arg_u, cnt = efn.saved
    for i, (z, (mu, rs)) in enumerate(zip(zs, stats)):
        if kernel_masks and hs[i] is not None:
            relu[f"encoder.mlp.{4 * i + 1}"] = _sx8_positive(hs[i][:rows], device)
        else:
            mask(f"mlp.{4 * i + 1}", z[:rows], mu[:rows], rs[:rows])
    pooled, f0, s0, f3, s3 = ffn.saved
    mask("feature_fusion.1", f0, *s0)
    mask("feature_fusion.4", f3, *s3)
    frozen = {"relu": relu,
              "argmax": {"enc_masked": arg_m.long().to(device), "vert_unmasked": arg_u.long().to(device)}}
    return frozen, n_border, efn
