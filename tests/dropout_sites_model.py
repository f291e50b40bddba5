"""fp64 restatement of the encoder's per-point MLP and of the vertex head WITH their train-mode dropout sites, shared by
tests/test_dropout_sites_model.py (pinned to the reference's own train-mode run) and the GPU tests that replay the
kernels' masks (tests/test_encoder_dropout_gpu.py, tests/test_vertex_dropout_gpu.py).

The reference holds an nn.Dropout behind every Linear, LayerNorm, ReLU block of PointNetEncoder.mlp (Sequential indices
4i + 3) and at index 3 of VertexPredictor.vertex_mlp1..4; oracle/reference_cpu.py restates those stages at p = 0.  Here
every function takes `drop = {site: pre-scaled mask}` (0 where an element is dropped, 1 / (1 - p) where it is kept; a
missing site is no dropout), with the sites named as the modules are:

    "mlp.{4i+3}"        on h_i = relu(LN(z_i)), before Linear i + 1         [rows, width_i]
    "vertex_mlp{k}.3"   on relu(LN(z_k)), k = 3, 4 before the residual add   [B, width_k]

and the `frozen` decisions of tests/enc_cases.py (ReLU masks, arg-max rows), which own_decisions takes UNDER the masks.
Built from oracle.reference_cpu._lin / _ln / _drop; nothing in oracle/ changes.

Host masks (the kernels' own bits): encoder_masks / vertex_masks from oracle.dropout.scaled(seed_k, row, col, p) with
site_seeds(seed, n)[k - 1] = (seed + 0x9E3779B9 k) mod 2^32, which is oracle.dropout.site_seeds for k <= 4."""
import numpy as np
import torch

from helpers import oracle
from oracle import dropout as D

GOLDEN = 0x9E3779B9
VERTEX_SITES = tuple(f"vertex_mlp{k}.3" for k in (1, 2, 3, 4))


def encoder_sites(n_hidden):
    return tuple(f"mlp.{4 * i + 3}" for i in range(n_hidden))


def site_seeds(seed, n):
    """Seed of site k = 1 .. n of a module that drew `seed` on the host (any depth)."""
    return [(int(seed) + GOLDEN * k) & 0xFFFFFFFF for k in range(1, n + 1)]


def row_masks(sites, seeds, ps, rows, widths):
    """{site: float64 [rows, width] pre-scaled mask} of the active sites; rows = a count (rows 0 .. rows-1) or an array."""
    r = np.arange(rows) if np.isscalar(rows) else np.asarray(rows)
    return {s: torch.from_numpy(D.scaled(sd, r[:, None], np.arange(w)[None, :], p))
            for s, sd, p, w in zip(sites, seeds, ps, widths) if p > 0}


def encoder_masks(seed, ps, rows, widths, words=None):
    """Masks of a PointNetEncoder forward that drew `seed` (host mode), or whose device words are `words` (site k uses
    words[k]).  rows: the rows of the matrix the per-point MLP ran on (B * N dense; the buffer rows of a packed batch)."""
    seeds = site_seeds(seed, len(ps)) if words is None else [int(w) & 0xFFFFFFFF for w in words[1:1 + len(ps)]]
    return row_masks(encoder_sites(len(ps)), seeds, ps, rows, widths)


def vertex_masks(seed, ps, B, widths=(4096, 2048, 2048, 1024), words=None):
    seeds = site_seeds(seed, 4) if words is None else [int(w) & 0xFFFFFFFF for w in words[1:5]]
    return row_masks(VERTEX_SITES, seeds, ps, B, widths)


# ----------------------------------------------------------------------------------------------------------------------
# the stages
# ----------------------------------------------------------------------------------------------------------------------
def _block(P, lin, ln, h, site, drop, frozen, record):
    """drop(relu(LN(Linear(h)))): the ReLU decision read from `frozen` where it holds one, recorded into `record`."""
    v = oracle._ln(P, ln, oracle._lin(P, lin, h))
    if record is not None:
        record[ln] = v > 0
    if frozen is not None and ln in frozen.get("relu", {}):
        a = v * frozen["relu"][ln].to(device=v.device, dtype=v.dtype)
    else:
        a = torch.relu(v)
    return oracle._drop(drop, site, a)


def point_mlp(P, x2d, drop=None, frozen=None, record=None, prefix="encoder."):
    mp = prefix + "mlp."
    n_lin = oracle._count_blocks(P, mp, 4)
    h = x2d
    for i in range(n_lin - 1):
        h = _block(P, f"{mp}{4 * i}", f"{mp}{4 * i + 1}", h, f"mlp.{4 * i + 3}", drop, frozen, record)
    return oracle._lin(P, f"{mp}{4 * (n_lin - 1)}", h)


def ref_dense(P, x, drop=None, frozen=None):
    """enc_cases.ref_dense with the sites' masks: (g [B, C], point_features [B, N, C], upooled [B, 2C])."""
    B, N, Din = x.shape
    pf = point_mlp(P, x.reshape(B * N, Din), drop, frozen).reshape(B, N, -1)
    mx, avg = oracle.encoder_pools(x, pf, frozen)
    g = oracle.encoder_fusion(P, torch.cat([mx, avg], dim=1), frozen=frozen)
    umax = pf.max(dim=1).values if frozen is None else oracle._max_over_points(pf, frozen, "vert_unmasked")
    return g, pf, torch.cat([pf.mean(dim=1), umax], dim=1)


def own_decisions(P, x, drop=None):
    """The decisions ref_dense(P, x, drop) takes itself, in the form `frozen` has (enc_cases.own_decisions, under the
    masks: a dropped activation changes every later layer's pre-activations and so their decisions)."""
    relu = {}
    with torch.no_grad():
        B, N, Din = x.shape
        pf = point_mlp(P, x.reshape(B * N, Din), drop, None, relu).reshape(B, N, -1)
        valid = x.abs().sum(-1) > 1e-9
        mv, mi = torch.where(valid.unsqueeze(-1), pf, torch.full_like(pf, float("-inf"))).max(dim=1)
        arg_m = torch.where(torch.isfinite(mv), mi, torch.full_like(mi, -1))
        mx = torch.where(torch.isfinite(mv), mv, torch.zeros_like(mv))
        avg = (pf * valid.unsqueeze(-1)).sum(1) / valid.sum(1, keepdim=True).clamp(min=1).to(pf.dtype)
        h = _block(P, "encoder.feature_fusion.0", "encoder.feature_fusion.1", torch.cat([mx, avg], 1), None, None, None, relu)
        _block(P, "encoder.feature_fusion.3", "encoder.feature_fusion.4", h, None, None, None, relu)
        return {"relu": relu, "argmax": {"enc_masked": arg_m, "vert_unmasked": pf.max(dim=1).indices}}


def ref_packed(P, pts, counts, drop=None, frozen=None):
    """enc_cases.ref_packed with the sites' masks: `drop` holds masks over the packed rows [>= M, width] (row r of the
    buffer), cut to each cloud's rows here."""
    import enc_cases as E
    C = P[f"encoder.mlp.{4 * (oracle._count_blocks(P, 'encoder.mlp.', 4) - 1)}.weight"].shape[0]
    pooled, pfs, ups, r0 = [], [], [], 0
    for b, n in enumerate(counts):
        if n == 0:
            pooled.append(pts.new_zeros(1, 2 * C)), ups.append(pts.new_zeros(1, 2 * C))
            continue
        x = pts[r0:r0 + n].unsqueeze(0)
        fz = E.slice_frozen(frozen, b, r0, r0 + n)
        dr = None if drop is None else {s: m[r0:r0 + n] for s, m in drop.items()}
        pf = point_mlp(P, x[0], dr, fz).unsqueeze(0)
        mx, avg = oracle.encoder_pools(x, pf, fz)
        umax = pf.max(dim=1).values if fz is None else oracle._max_over_points(pf, fz, "vert_unmasked")
        pooled.append(torch.cat([mx, avg], dim=1)), pfs.append(pf[0]), ups.append(torch.cat([pf.mean(dim=1), umax], dim=1))
        r0 += n
    assert r0 == pts.shape[0]
    return oracle.encoder_fusion(P, torch.cat(pooled), frozen=frozen), torch.cat(pfs), torch.cat(ups)


def vertex_forward(P, g, pf, max_vertices, vertex_dim=4, drop=None, frozen=None, record=None, prefix="vertex_predictor.",
                   upooled=None):
    """oracle.vertex_forward with the sites' masks: each one on relu(LN(z_k)), the residual added after it.  upooled:
    the [mean | max] pools directly (VertexPredictor.predict) instead of point_features."""
    if pf is not None:
        if frozen is not None and "vert_unmasked" in frozen.get("argmax", {}):
            umax = oracle._max_over_points(pf, frozen, "vert_unmasked")
        else:
            umax = pf.max(dim=1).values
        upooled = torch.cat([pf.mean(dim=1), umax], dim=1)
    e = g if upooled is None else g + oracle._lin(P, prefix + "point_pool_proj", upooled)

    def stage(k, h):
        return _block(P, f"{prefix}vertex_mlp{k}.0", f"{prefix}vertex_mlp{k}.1", h, f"vertex_mlp{k}.3", drop, frozen, record)

    a = stage(1, e)
    b = stage(2, a)
    c = stage(3, b) + oracle._lin(P, prefix + "residual_proj1", e)
    d = stage(4, c) + oracle._lin(P, prefix + "residual_proj2", e)
    o = oracle._lin(P, prefix + "final_layer", d).reshape(g.shape[0], max_vertices, vertex_dim)
    exist = torch.sigmoid(o[:, :, 3])
    return {"vertices": o[:, :, :3], "existence_probabilities": exist, "actual_vertex_counts": (exist > 0.5).sum(dim=1)}
