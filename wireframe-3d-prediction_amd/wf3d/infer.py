"""The forward-only paths of the per-point encoder (encoder_stream) and of the edge head (edge_stream): no autograd
Function, nothing kept for a backward.

The training forward (functional._encoder_forward_rows) keeps every layer's pre-LayerNorm z and every sx8 operand h
until it returns, and writes mu, rs, the arg-max rows and the whole point_features tensor: 18.4 KB + 18.4 KB + 2 KB per
point row at the default widths, none of it read again under torch.no_grad().  Here the rows are walked in blocks
(block_plan): each block runs the same Linears on the same kernels — the routes are decided once, from the total row
count, exactly as the training forward decides them — through block buffers that are allocated once and reused, and its
point_features are folded into the running pools (ops.PoolStream) before the next block overwrites them.  What is
allocated does not grow with the row count, apart from the [B, .] results and a point_features tensor the caller asks
for.  The first layer runs without writing z (ops.first_layer_infer).

Opt-in: wf3d.config.set_inference("stream") / WF3D_INFERENCE=stream sends the encoder stage of the drop-in classes here
when grad mode is off; PointNetEncoder.encode_stream / encode_packed_stream call it directly.

The edge head is the other stage whose activations grow with the batch: 4,608 B per edge row at hidden_dim = 512 on the
split route.  edge_stream walks the edge rows the same way; its own opt-in is wf3d.config.set_edge_inference("stream") /
WF3D_EDGE_INFERENCE=stream, and EdgePredictor.forward_stream calls it directly."""
import torch

from . import config, ops
from .functional import _SPLIT_PRODUCTS, _edge_live_fwd, _edge_routes, _edge_vertex_section, _encoder_routes, mlp_layers
from .ops import ACT_GELU, ACT_RELU, NT, Pro


def check_rows(rows):
    """A block height: a positive multiple of 8 (the sx8 operands and the 16-byte row passes come in 8-row groups)."""
    if isinstance(rows, bool) or not isinstance(rows, int) or rows <= 0 or rows % 8:
        raise ValueError(f"wf3d.infer: rows must be a positive multiple of 8 (got {rows!r})")
    return rows


def block_plan(total_rows, rows=None):
    """[(r0, n), ...]: the blocks of at most `rows` rows that cover [0, total_rows) once, in order; only the last one
    may be shorter.  rows = None: config.INFER_ROWS."""
    rows = check_rows(config.INFER_ROWS if rows is None else rows)
    if isinstance(total_rows, bool) or not isinstance(total_rows, int) or total_rows < 0:
        raise ValueError(f"wf3d.infer: total_rows must be a non-negative int (got {total_rows!r})")
    return [(r0, min(rows, total_rows - r0)) for r0 in range(0, total_rows, rows)]


class DenseRows:
    """The row offsets of a dense [B, N, .] batch as the streaming pool reads them: d_rows = int32 [B + 1] = b * N, built
    on the device."""

    def __init__(self, B, N, device):
        if (B + 1) * N > 0x7FFFFFFF:
            raise ValueError("wf3d.infer: the row total does not fit in int32")
        self.B, self.N = B, N
        self.d_rows = torch.arange(B + 1, dtype=torch.int32, device=device) * N


def encoder_stream(x2, pools_layout, n_hidden, precision, params, rows=None, want_pf=False, walk=None):
    """The per-point MLP over the rows of x2 [M, Din] (contiguous) in blocks of `rows`, pooled as the blocks pass.

    pools_layout: whose d_rows (int32 [B + 1], device memory) says which rows are which cloud's — DenseRows, an
    ops.PackedLayout or an ops.DevicePackedLayout; rows of x2 at or past d_rows[B] are computed and pooled into no
    cloud.  walk (<= M, default M): only the first `walk` rows are walked — the caller knows that no cloud has a row
    behind them; a requested point_features is zeros there.  params as EncoderFn's.  Returns (ops.PoolOut without
    arg-max rows, point_features [M, C] or None)."""
    if not x2.is_cuda:
        raise RuntimeError("wf3d: the HIP path needs CUDA (ROCm) tensors; there is no CPU fallback")
    if x2.dim() != 2 or not x2.is_contiguous():
        raise RuntimeError("wf3d.infer.encoder_stream: contiguous [rows, input_dim] points required")
    M, dev = x2.shape[0], x2.device
    walk = M if walk is None else walk
    if not 0 <= walk <= M:
        raise ValueError(f"wf3d.infer.encoder_stream: walk must be 0 .. {M} (got {walk})")
    plan = block_plan(walk, rows)
    layers = mlp_layers(params, n_hidden)
    Ws = [L.W for L in layers]
    # decided once, from the row total, as the training forward decides them: a short last block flips no layer
    routes = _encoder_routes(x2[:walk], Ws, precision in _SPLIT_PRODUCTS, want_dx=False)
    npr = _SPLIT_PRODUCTS.get(precision, 3)
    C = Ws[-1].shape[0]
    with torch.no_grad():
        # the forward orientation of every split layer's weight, once per call
        W_s = {i: ops.split_rows(Ws[i]) for i, r in enumerate(routes) if r.fwd == "split"}
        pool = ops.PoolStream(pools_layout.d_rows, C)
        pf = torch.empty(M, C, dtype=torch.float32, device=dev) if want_pf else None
        if want_pf and walk < M:
            pf[walk:].zero_()
        # Block buffers.  z_i lives in zb[i % 2] (Linear i + 1 on the fp32 route reads z_i while it writes z_{i+1}), the one
        # sx8 operand alive at a time in hb, the block's mu / rs / valid in one [3, rows] buffer.
        R = plan[0][1] if plan else 0
        zw, hw = [0, 0], 0
        for i, r in enumerate(routes):
            D = Ws[i].shape[0]
            if r.fwd != "first" and not (i == n_hidden and want_pf):
                zw[i % 2] = max(zw[i % 2], D)
            if i < n_hidden and (r.fwd == "first" or routes[i + 1].fwd == "split"):
                hw = max(hw, D)
        zb = [torch.empty(R * w, dtype=torch.float32, device=dev) if w else None for w in zw]
        hb = torch.empty(R * hw, dtype=torch.float32, device=dev) if hw else None
        rowbuf = torch.empty(3, max(R, 1), dtype=torch.float32, device=dev)
        for r0, n in plan:
            xb = x2[r0:r0 + n]
            mu, rs = rowbuf[0, :n], rowbuf[1, :n]
            valid = ops.point_valid(xb, out=rowbuf[2, :n])
            a, a_s, pro = xb, None, None
            for i, (r, (W, b, g, be)) in enumerate(zip(routes, layers)):
                D = W.shape[0]
                if r.fwd == "first":
                    a_s = ops.first_layer_infer(xb, W, b, g, be, ACT_RELU, out=hb[:n * D].view(n, D))
                    a, pro = None, None
                    continue
                out = pf[r0:r0 + n] if (i == n_hidden and want_pf) else zb[i % 2][:n * D].view(n, D)
                if r.fwd == "split":
                    z = ops.gemm_split(a_s, W_s[i], bias=b, out=out, products=npr)
                else:
                    z = ops.gemm(a, W, NT, bias=b, pro=pro, out=out)
                if i == n_hidden:
                    break
                if routes[i + 1].fwd == "split":
                    a_s = hb[:n * D].view(n, D)
                    ops.ln_prep(z, g, be, ACT_RELU, out=(mu, rs, a_s))
                else:
                    a_s = None
                    ops.row_stats(z, out=(mu, rs))
                a, pro = z, Pro(ACT_RELU, mu, rs, g, be)
            pool.fold(z, valid, r0)
        return pool.finish(), pf


def edge_stream(verts, meta, heads, precision, P, rows=None):
    """The forward-only edge head: EdgeFn's forward without dropout, with the edge rows walked in blocks of `rows`
    (default config.INFER_EDGE_ROWS) through buffers that are allocated once, sized by the block height, and reused.
    Nothing per edge row outlives its block except its logit (4 B per row).

    verts [B, V, vertex_dim] float32 (a view is fine); meta: an ops.EdgeMeta, host-built or EdgeMeta.device; P: the
    head's functional.EdgeParams block.
    Returns edge_probs [B, meta.max_e], zero padding included, as EdgeFn returns it: bit for bit when one
    block covers all rows (rows >= meta.Re), within the forward bound at other heights (the GEMMs' split-K plans follow
    the block's row count).

    The per-vertex section (sum-of-counts rows: vertex_proj, attention, Pa / Pb) runs whole, on EdgeFn's ops in its
    order.  The routes of the two wide Linears and the logits kernel are decided once, from the row total, as EdgeFn
    decides them.  A padded layout in tail="skip" mode whose two wide Linears run split and whose logits layer is the
    row-dot kernel (functional._edge_live_fwd) runs each block under its own live-row count
    (ops.block_live): a block past the live pair total costs its launches' entry checks and nothing more, and no count
    is read on the host.  The result equals tail="compute" bit for bit."""
    if not verts.is_cuda:
        raise RuntimeError("wf3d: the HIP path needs CUDA (ROCm) tensors; there is no CPU fallback")
    rows = check_rows(config.INFER_EDGE_ROWS if rows is None else rows)
    H, dev = P.M0w.shape[0], verts.device
    with torch.no_grad():
        # ---- per-vertex section: EdgeFn's, drop p = 0 ----
        x3 = precision == "bf16x3" and config.EDGE_X3
        cv, *_, Pa, Pb = _edge_vertex_section(verts, meta, heads, x3, P)
        del _
        # ---- edge-row section: decided once, from the row total; a short last block flips nothing ----
        npr = _SPLIT_PRODUCTS.get(precision, 3)
        routes = _edge_routes(meta.Re, H, precision, x3)
        split = routes[0].fwd == "split"
        rowdot = P.M10w.shape[0] == 1 and P.M10w.is_contiguous() and ops.rowdot_act_shape_ok(H // 4)
        # every launch of the loop below then honours the count; on any other route the tail is computed, as EdgeFn does
        live = _edge_live_fwd(meta, routes, rowdot)
        plan = block_plan(meta.Re, rows)
        R = plan[0][1] if plan else 0
        f32 = dict(dtype=torch.float32, device=dev)
        logit = torch.empty(meta.Re, 1, **f32)
        z2, z3 = torch.empty(R, H // 2, **f32), torch.empty(R, H // 4, **f32)
        if split:
            h1, h2 = torch.empty(R, H, **f32), torch.empty(R, H // 2, **f32)
            (M4s, _), (M8s, _) = ops.split_weights([P.M4w, P.M8w])
        else:
            pre = torch.empty(R, H, **f32)
        rowbuf = torch.empty(2, max(R, 1), **f32)            # mu / rs of the layer at hand (launches run in stream order)
        fused_tail = ops.rowdot_act_ok(z3, P.M10w)
        assert fused_tail or live is None
        blive = ops.block_live(live, rows, meta.Re, len(plan)) if live is not None else None
        for k, (e0, n) in enumerate(plan):
            mu, rs = rowbuf[0, :n], rowbuf[1, :n]
            with ops.live_rows(blive[k:k + 1] if blive is not None else None):
                if split:
                    ops.edge_pair_infer(Pa, Pb, cv, P.M0w, meta, e0, n, h1[:n], ln=(P.M1g, P.M1b, ACT_GELU))
                    ops.gemm_split(h1[:n], M4s, bias=P.M4b, out=z2[:n], products=npr)
                    ops.ln_prep(z2[:n], P.M5g, P.M5b, ACT_GELU, out=(mu, rs, h2[:n]))
                    ops.gemm_split(h2[:n], M8s, bias=P.M8b, out=z3[:n], products=npr)
                else:
                    ops.edge_pair_infer(Pa, Pb, cv, P.M0w, meta, e0, n, (pre[:n], mu, rs))
                    ops.gemm(pre[:n], P.M4w, NT, bias=P.M4b, pro=Pro(ACT_GELU, mu, rs, P.M1g, P.M1b), x3=x3, out=z2[:n])
                    ops.row_stats(z2[:n], out=(mu, rs))
                    ops.gemm(z2[:n], P.M8w, NT, bias=P.M8b, pro=Pro(ACT_GELU, mu, rs, P.M5g, P.M5b), x3=x3, out=z3[:n])
                if fused_tail:
                    ops.rowdot_act(z3[:n], P.M10w, P.M10b, ACT_GELU, out=logit[e0:e0 + n])
                else:
                    ops.gemm(z3[:n], P.M10w, NT, bias=P.M10b, pro=Pro(ACT_GELU), out=logit[e0:e0 + n])
        return ops.edge_prob_fwd(logit, meta)
