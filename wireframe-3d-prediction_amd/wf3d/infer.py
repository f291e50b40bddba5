"""The forward-only path of the per-point encoder: no autograd Function, nothing kept for a backward.

The training forward (functional._encoder_forward_rows) keeps every layer's pre-LayerNorm z and every sx8 operand h
until it returns, and writes mu, rs, the arg-max rows and the whole point_features tensor: 18.4 KB + 18.4 KB + 2 KB per
point row at the default widths, none of it read again under torch.no_grad().  Here the rows are walked in blocks
(block_plan): each block runs the same Linears on the same kernels — the routes are decided once, from the total row
count, exactly as the training forward decides them — through block buffers that are allocated once and reused, and its
point_features are folded into the running pools (ops.PoolStream) before the next block overwrites them.  What is
allocated does not grow with the row count, apart from the [B, .] results and a point_features tensor the caller asks
for.  The first layer runs without writing z (ops.first_layer_infer).

Opt-in: wf3d.config.set_inference("stream") / WF3D_INFERENCE=stream sends the encoder stage of the drop-in classes here
when grad mode is off; PointNetEncoder.encode_stream / encode_packed_stream call it directly."""
import torch

from . import config, ops
from .functional import _SPLIT_PRODUCTS, _encoder_routes
from .ops import ACT_RELU, NT, Pro


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
    Ws = [params[4 * i] for i in range(n_hidden + 1)]
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
            for i, r in enumerate(routes):
                W, b = Ws[i], params[4 * i + 1]
                D = W.shape[0]
                if r.fwd == "first":
                    a_s = ops.first_layer_infer(xb, W, b, params[2], params[3], ACT_RELU, out=hb[:n * D].view(n, D))
                    a, pro = None, None
                    continue
                out = pf[r0:r0 + n] if (i == n_hidden and want_pf) else zb[i % 2][:n * D].view(n, D)
                if r.fwd == "split":
                    z = ops.gemm_split(a_s, W_s[i], bias=b, out=out, products=npr)
                else:
                    z = ops.gemm(a, W, NT, bias=b, pro=pro, out=out)
                if i == n_hidden:
                    break
                g, be = params[4 * i + 2], params[4 * i + 3]
                if routes[i + 1].fwd == "split":
                    a_s = hb[:n * D].view(n, D)
                    ops.ln_prep(z, g, be, ACT_RELU, out=(mu, rs, a_s))
                else:
                    a_s = None
                    ops.row_stats(z, out=(mu, rs))
                a, pro = z, Pro(ACT_RELU, mu, rs, g, be)
            pool.fold(z, valid, r0)
        return pool.finish(), pf
