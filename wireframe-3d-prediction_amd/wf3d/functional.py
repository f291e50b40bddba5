"""The three stages of the hot path as torch.autograd.Function's whose forward
and backward are sequences of libwf3d.so calls (wf3d.ops).

Stage          reference lines replaced
EncoderFn      models/PointNetEncoder.py:67-118
VertexFn       models/VertexPredictor.py:63-133
EdgeFn         models/EdgePredictor.py:91-140 x the per-sample loop of
               models/PointCloudToWireframe.py:77-112 (batched, ragged)

Data layout in HBM (fp32): per Linear only its PRE-LayerNorm output z and the
per-row (mu, rstd) are stored; LN-apply + ReLU/GELU (+dropout) are re-applied in
the staging pass of whichever GEMM consumes them (forward GEMM, wgrad GEMM), so
normalised activations never exist in memory.

Which kernels a Linear of the encoder's per-point MLP or of the edge MLP's two wide layers runs on, forward and
backward, is its Route: decided once in the stage's forward (_encoder_routes, _edge_routes) and only read by backward.
"""
from collections import namedtuple
from collections.abc import Sequence

import torch

from . import config, ops
from . import skinny as sk
from .dropout import Drop, _seeded, _take_drop  # noqa: F401  (Drop: the stages' optional last argument)
from .ops import ACT_GELU, ACT_NONE, ACT_RELU, NN, NT, TN, Pro


def _saved(ctx):
    """The activations a stage kept for its backward.  They are released by the first backward (2.7 GB
    at cfg2), so a second one through the same graph (retain_graph=True) cannot be served: say so
    instead of failing on a None unpack."""
    if ctx.saved is None:
        raise RuntimeError("wf3d: backward through this graph a second time — the stage's saved activations were "
                           "released by the first backward; re-run the forward, or set wf3d.config.RETAIN_SAVED = True "
                           "(WF3D_RETAIN_SAVED=1) before the forward to keep them for backward(retain_graph=True)")
    return ctx.saved


def _keep_params(ctx, params):
    """Parameters are kept as plain attributes (save_for_backward would forbid the views the stages take of them);
    their version counters are recorded so that an in-place update between forward and backward is reported the way
    autograd reports it for saved tensors, instead of silently producing gradients against the new values."""
    ctx.params = params
    ctx.param_versions = [None if p is None else p._version for p in params]


def _params(ctx):
    for i, (p, v) in enumerate(zip(ctx.params, ctx.param_versions)):
        if p is not None and p._version != v:
            raise RuntimeError(f"wf3d: parameter {i} of this stage (shape {tuple(p.shape)}) was modified in place after the "
                               f"forward that is being differentiated (version {p._version}, expected {v}); "
                               "run backward before the optimizer step / in-place update")
    return ctx.params


def _lin_bwd(dz, a, W, pro_a):
    """Linear backward pieces for z = pro(a)·W^T + b given dz:
    dW = dz^T·pro(a) (TN, prologue re-applied to the stored pre-activation),
    d pro(a) = dz·W (NN)."""
    return ops.gemm(dz, a, TN, pro=pro_a), ops.gemm(dz, W, NN)


# Parameter blocks: a stage's parameters by name.  Each Function takes them positionally (*params, in field order) and
# rebuilds its block once in forward and once in backward; the models build the blocks by keyword, next to their module trees.
FusionParams = namedtuple("FusionParams", "F0w F0b F1g F1b F3w F3b F4g F4b F6w F6b")
VertexParams = namedtuple("VertexParams", "W1 b1 g1 be1 W2 b2 g2 be2 W3 b3 g3 be3 W4 b4 g4 be4 Wf bf Wr1 br1 Wr2 br2 Wpp bpp",
                          defaults=(None, None))                 # Wpp, bpp: point_pool_proj, created lazily
EdgeParams = namedtuple("EdgeParams", "P0w P0b P1g P1b P3w P3b P4g P4b Aw Ab Ow Ob "
                                      "M0w M0b M1g M1b M4w M4b M5g M5b M8w M8b M10w M10b")
MlpLayer = namedtuple("MlpLayer", "W b gamma beta", defaults=(None, None))


def _grads_of(block):
    """The gradient collector of a parameter block: one slot per field, set by name (a name the block does not have
    raises); out() is the gradients in field order, None where none was set."""
    def out(self):
        return [getattr(self, f, None) for f in block._fields]
    return type(block.__name__ + "Grads", (), {"__slots__": block._fields, "out": out})


FusionGrads, VertexGrads, EdgeGrads, MlpLayerGrads = map(_grads_of, (FusionParams, VertexParams, EdgeParams, MlpLayer))


def mlp_layers(params, n_hidden):
    """The encoder's flat [W_i, b_i, gamma_i, beta_i] * n_hidden + [W_out, b_out] as one MlpLayer per Linear; the output
    layer's gamma and beta are None."""
    return [MlpLayer(*params[4 * i:4 * i + 4]) for i in range(n_hidden + 1)]


_side_streams = {}


class _Leaves:
    """Runs the leaves of a backward — gradients no later kernel of the step reads — on a second stream.
    `run(fn, *reads)` makes the side stream wait for everything issued so far on the current one, then calls fn
    under it; `reads` are the tensors fn consumes (their memory must not be recycled by the current stream's
    allocator pool before the side stream is done with them).  `join(*outs)` orders the current stream after the
    side stream and hands the outputs over.  Not enabled, run() just calls fn."""

    def __init__(self, device, enable=True):
        self.on = enable and device.type == "cuda"
        if self.on:
            self.main = torch.cuda.current_stream(device)
            self.side = _side_streams.get(device.index)
            if self.side is None:
                self.side = _side_streams[device.index] = torch.cuda.Stream(device)
            self.on = self.side != self.main

    def run(self, fn, *reads):
        if not self.on:
            return fn()
        self.side.wait_stream(self.main)
        for t in reads:
            if t is not None:
                t.record_stream(self.side)
        with torch.cuda.stream(self.side):
            return fn()

    def join(self, *outs):
        if not self.on:
            return
        self.main.wait_stream(self.side)
        for t in outs:
            if t is not None:
                t.record_stream(self.main)


# ===========================================================================
# Routes of the large Linears
# ===========================================================================
def _split_ok(rows, k, split):
    """A Linear runs as a bf16x3 split GEMM when the mode asks for it, the layer is big
    enough to be MFMA-bound and its reduction width fits the 8-column sx8 groups."""
    return split and rows >= config.SPLIT_MIN_ROWS and k % 8 == 0 and k >= 32


# Modes that run the large Linears on sx8 operands, and the bf16 MFMAs per product each one issues: "bf16" runs exactly
# the GEMMs "bf16x3" runs split, one product (hi*hi) instead of three.
_SPLIT_PRODUCTS = {"bf16x3": 3, "bf16": 1}

_TN = ("tn", "tn_t")        # the wgrad forms that read the forward's sx8 input operand instead of the fp32 one


# The kernels of one Linear z = h·W^T + b, forward and backward:
# fwd    "split": gemm_split on sx8 operands; "fp32": gemm; "first": the encoder's fused first layer (first_layer_fwd)
# wgrad  dW = dz^T·h.  "tn": the transposing-read TN kernel on both sx8 operands as stored; "tn_t": the same on the
#        transposed problem dW^T = h^T·dz, the small result transposed back (the kernel tiles dW[Mo, No] with
#        Mo % 256 == 0, e.g. not dW[128, 256]); "transposes": gemm_split on materialised split_transposes (shapes the TN
#        kernel does not tile, whole 8-row groups); "fp32": gemm TN re-applying h's prologue to the stored z; "first":
#        ln_act_bwd_first (LN/ReLU backward, bias and weight gradient of the encoder's first layer in one pass)
# dgrad  dh = dz·W.  "split": gemm_split with W^T in sx8; "fp32": gemm NN; None: no input gradient
# x3     the fp32 GEMMs' operands split in their staging pass (config.EDGE_X3)
Route = namedtuple("Route", "fwd wgrad dgrad x3", defaults=(False,))


def _dz32(r):
    """Backward forms dz in fp32 (with both of its consumers on sx8 operands only the sx8 dz is written)."""
    return "fp32" in (r.wgrad, r.dgrad)


def _encoder_routes(x2, Ws, split, want_dx):
    """Routes of the per-point MLP's Linears Ws = [W_0, ..., W_out] over the rows of x2.  Linear i >= 1 runs forward
    split when its input width takes the split path (the LayerNorm pass before it then writes its operand in sx8), its
    dgrad when its output width does, and its wgrad on sx8 operands when both do.  Linear 0 (in_features <= 8) is one
    fused pass with its LayerNorm, forward and — unless the cloud requires grad: dx = dz·W needs dz — backward."""
    M = x2.shape[0]
    ok = lambda d: _split_ok(M, d, split)  # noqa: E731
    first = len(Ws) > 1 and ok(Ws[0].shape[0]) and ops.first_layer_ok(x2, Ws[0])
    dx = "fp32" if want_dx else None
    routes = [Route("first", "fp32" if want_dx else "first", dx) if first else Route("fp32", "fp32", dx)]
    for W in Ws[1:]:
        n, k = W.shape
        wgrad = "fp32"
        if ok(n) and ok(k):
            wgrad = "tn" if ops.gemm_split_tn_shape_ok(M, n, k, n, k) else "transposes" if M % 8 == 0 else "fp32"
        routes.append(Route("split" if ok(k) else "fp32", wgrad, "split" if ok(n) else "fp32"))
    return routes


def _edge_routes(Re, H, precision, x3):
    """Routes of the edge MLP's two wide Linears, edge_mlp.4 (H -> H/2) and edge_mlp.8 (H/2 -> H/4), over Re edge rows
    (52 % of the FLOPs at V=256): both split or both fp32.  H / 4, the second one's width, is the reduction width of its
    dgrad and the row length of its transposed weight: it has to be made of whole 8-column groups too
    (EdgePredictor(hidden_dim=208) used to fail in split_weights)."""
    if not (_split_ok(Re, H, precision in _SPLIT_PRODUCTS) and _split_ok(Re, H // 2, True) and (H // 4) % 8 == 0):
        return Route("fp32", "fp32", "fp32", x3), Route("fp32", "fp32", "fp32", x3)

    def wgrad(n, k):
        if ops.gemm_split_tn_shape_ok(Re, n, k, n, k):
            return "tn"
        if ops.gemm_split_tn_shape_ok(Re, k, n, k, n):
            return "tn_t"
        return "transposes" if Re % 8 == 0 else "fp32"
    return Route("split", wgrad(H // 2, H), "split", x3), Route("split", wgrad(H // 4, H // 2), "split", x3)


def _edge_live_fwd(meta, routes, fused_tail):
    """The live-row count the forward launches over edge rows can run under, or None.  It is used for a padded layout in
    tail="skip" mode whose two wide Linears run split in forward and whose logits layer is the row-dot kernel
    (fused_tail).  Every forward launch of the section then honours the count (include/wf3d.h, "LIVE ROW COUNT"): rows
    past its extent are never written and never read.  Any other route (fp32 precision, too few rows) computes the tail
    as tail="compute" does."""
    ok = meta.padded and meta.tail == "skip" and fused_tail and all(r.fwd == "split" for r in routes)
    return meta.live if ok else None


def _edge_live(meta, routes, fused_tail):
    """The live-row count the edge-row section of EdgeFn runs under, forward and backward, or None: the forward
    condition (_edge_live_fwd), and the backward's: split dgrads, with the wgrads on sx8 operands (the TN kernels or
    the "transposes" form; an fp32 wgrad, for a row total that is not a multiple of 8, does not see a count)."""
    ok = all(r.dgrad == "split" and r.wgrad in _TN + ("transposes",) for r in routes)
    return _edge_live_fwd(meta, routes, fused_tail) if ok else None


def _encoder_live(layout, routes, tail):
    """The live-row count the per-point MLP of a packed batch runs under, forward and backward, or None.  It is used in
    tail="skip" mode for a capacity layout (ops.PackedLayout(counts, capacity) or ops.DevicePackedLayout: the live row
    total is layout.d_rows[B]) whose first Linear is the fused first-layer pass, forward and backward, and whose later
    Linears all run split, forward and dgrad, with their wgrads on sx8 operands (the TN kernel or the "transposes"
    form).  Every launch over point rows then honours the count (include/wf3d.h, "LIVE ROW COUNT"): rows past its
    extent are never written and never read.  Any other route (fp32 precision, a capacity below SPLIT_MIN_ROWS, a width
    the split kernels do not take, a first layer first_layer_ok refuses) computes the tail as tail="compute" does: the
    fp32 GEMMs and wf3d_row_stats do not see a count."""
    if tail != "skip" or layout is None or layout.capacity is None:
        return None
    ok = routes[0] == Route("first", "first", None) and all(
        r.fwd == "split" and r.dgrad == "split" and r.wgrad in ("tn", "transposes") for r in routes[1:])
    return layout.d_rows[layout.B:layout.B + 1] if ok else None


def _wgrad(r, dz, dz_s, h, pro, h_s, products):
    """dW = dz^T · pro(h) by the route's wgrad form: dz (fp32) or dz_s (sx8), whichever the route formed; h the stored
    input with its prologue pro, h_s the forward's sx8 operand pro(h)."""
    if r.wgrad == "tn":
        return ops.gemm_split_tn(dz_s, h_s, products=products)
    if r.wgrad == "tn_t":
        return ops.gemm_split_tn(h_s, dz_s, products=products).t().contiguous()
    if r.wgrad == "transposes":
        # under a live-row count the transposes read no tail row and zero their tail columns; those columns are the
        # GEMM's reduction dimension, not its rows, so the GEMM runs without the count and adds exact zeros for them
        dz_t, h_t = ops.split_transpose(dz_s, in_sx8=True), ops.split_transpose(h, pro)
        with ops.live_rows(None):
            return ops.gemm_split(dz_t, h_t, products=products)
    return ops.gemm(dz, h, TN, pro=pro, x3=r.x3)


def _dgrad(r, dz, dz_s, W, W_t, products):
    """dh = dz · W by the route's dgrad form; W_t = W^T in sx8 when the forward split it, else None."""
    if r.dgrad == "split":
        if W_t is None:
            with ops.live_rows(None):                  # a weight's rows are not the count's
                W_t = ops.split_rows(W, transpose=True)
        return ops.gemm_split(dz_s, W_t, products=products)
    return ops.gemm(dz, W, NN, x3=r.x3)


# ===========================================================================
# Encoder
# ===========================================================================
class _DensePools:
    """The pools of a dense [B, N, C] batch behind the encoder's shared forward and backward."""

    def __init__(self, B, N):
        self.B, self.N = B, N

    def fwd(self, pf, valid):
        return ops.pool4_fwd(pf.view(self.B, self.N, pf.shape[1]), valid, packed=True)

    def bwd(self, valid, cnt, arg_m, arg_u, cots, dpf, C, sx8=False):
        return ops.pool4_bwd(valid, cnt, arg_m, arg_u, *cots, dpf, self.B, self.N, C, sx8=sx8).view(self.B * self.N, C)

    def colsum(self, valid, nvalid, cnt, arg_m, arg_u, cots, dpf, C):
        return ops.pool4_bwd_colsum(nvalid, cnt, arg_m, arg_u, *cots, dpf, self.B, self.N, C)


class _PackedPools:
    """The segmented pools of a packed batch: rows offsets[b] .. offsets[b+1]-1 are cloud b's.  `layout` is an
    ops.PackedLayout (table from host counts) or an ops.DevicePackedLayout (table built on the device): one code path,
    two table sources."""

    def __init__(self, layout):
        self.layout = layout

    def fwd(self, pf, valid):
        return ops.pool4_seg_fwd(pf, valid, self.layout)

    def bwd(self, valid, cnt, arg_m, arg_u, cots, dpf, C, sx8=False):
        return ops.pool4_seg_bwd(valid, cnt, arg_m, arg_u, *cots, dpf, self.layout, C, sx8=sx8)

    def colsum(self, valid, nvalid, cnt, arg_m, arg_u, cots, dpf, C):
        return ops.pool4_seg_bwd_colsum(nvalid, cnt, arg_m, arg_u, *cots, dpf, self.layout, C, valid=valid)


def _encoder_forward(ctx, x2, pools, n_hidden, precision, params, tail="compute"):
    """The per-point MLP over the rows of x2 and its pools (`pools`: _DensePools or _PackedPools): the forward of EncoderFn
    and EncoderFnPacked.  Returns (PoolOut, point_features [rows, C]).  tail="skip": a packed batch with a capacity runs
    under its live row total where the routes allow it (_encoder_live); the backward follows ctx.live.
    params may end in a Drop (train-mode dropout at mlp.{4i+3}): site i masks h_i = relu(LN(z_i)) in whichever launch
    produces or re-applies it, forward and backward (ctx.drop = [ps, site seeds, device words])."""
    rest, *ctx.drop = _take_drop(params, n_hidden, "EncoderFn")
    ctx.n_extra = len(params) - len(rest)                        # a trailing Drop takes a (None) gradient slot
    params, layers = rest, mlp_layers(rest, n_hidden)
    routes = _encoder_routes(x2, [L.W for L in layers], precision in _SPLIT_PRODUCTS, ctx.needs_input_grad[0])
    ctx.live = live = _encoder_live(getattr(pools, "layout", None), routes, tail)
    with ops.live_rows(live), _seeded(ctx.drop[2]):
        return _encoder_forward_rows(ctx, x2, pools, n_hidden, precision, params, layers, routes)


def _encoder_forward_rows(ctx, x2, pools, n_hidden, precision, params, layers, routes):
    npr = _SPLIT_PRODUCTS.get(precision, 3)
    ps, sd, _ = ctx.drop
    valid = ops.point_valid(x2)
    # both sx8 orientations (W for the forward GEMM, W^T for its dgrad) of every layer split both ways, one launch
    widx = [i for i, r in enumerate(routes) if r.fwd == "split" and r.dgrad == "split"]
    wsplit = dict(zip(widx, ops.split_weights([layers[i].W for i in widx]))) if widx else {}
    zs, stats, hs = [], [], []                 # hs[i] = sx8 operand consumed by Linear i+1 (kept for its wgrad)
    a, a_s, pro = x2, None, None
    for i, (r, (W, b, g, be)) in enumerate(zip(routes, layers)):
        if r.fwd == "first":
            # first Linear + LayerNorm + ReLU + split in one pass (K = input_dim <= 8: a pure write of z and h)
            z, mu, rs, a_s = ops.first_layer_fwd(x2, W, b, g, be, ACT_RELU, drop_p=ps[i], seed=sd[i])
        elif r.fwd == "split":
            if i in wsplit:
                W_s = wsplit[i][0]
            else:
                with ops.live_rows(None):              # a weight's rows are not the count's
                    W_s = ops.split_rows(W)
            z = ops.gemm_split(a_s, W_s, bias=b, products=npr)
            a_s = None
        else:
            z = ops.gemm(a, W, NT, bias=b, pro=pro)
        if i == n_hidden:
            pf = z
            break
        if r.fwd == "first":
            pass
        elif routes[i + 1].fwd == "split":
            mu, rs, a_s = ops.ln_prep(z, g, be, ACT_RELU, drop_p=ps[i], seed=sd[i])
        else:
            mu, rs = ops.row_stats(z)
        hs.append(a_s)
        zs.append(z)
        stats.append((mu, rs))
        pro = Pro(ACT_RELU, mu, rs, g, be, ps[i], sd[i])
        a = z
    del a_s
    C = pf.shape[1]
    po = pools.fwd(pf, valid)                                         # [max | avg] (PointNetEncoder.py:115), [mean | max]
    ctx.n_hidden, ctx.pools, ctx.width, ctx.products, ctx.routes = n_hidden, pools, C, npr, routes
    _keep_params(ctx, params)
    ctx.saved = (x2, valid, zs, stats, hs, po.arg_m, po.arg_u, po.cnt)
    ctx.nvalid = po.nvalid
    ctx.wT = {i: ws[1] for i, ws in wsplit.items()}
    # unused outputs (point_features when only its pools are consumed) must not come back as 268 MB of zeros
    ctx.set_materialize_grads(False)
    return po, pf


def _encoder_backward(ctx, dpooled, dpf, dupooled):
    """The backward of EncoderFn and EncoderFnPacked: (gradient of the rows of x2 or None, parameter gradients), under the
    live-row count the forward chose (ctx.live)."""
    with ops.live_rows(ctx.live), _seeded(ctx.drop[2]):
        return _encoder_backward_rows(ctx, dpooled, dpf, dupooled)


def _encoder_backward_rows(ctx, dpooled, dpf, dupooled):
    nh, pools, C, npr, routes = ctx.n_hidden, ctx.pools, ctx.width, ctx.products, ctx.routes
    layers = mlp_layers(_params(ctx), nh)
    ps, sd, _ = ctx.drop
    x2, valid, zs, stats, hs, arg_m, arg_u, cnt = _saved(ctx)
    Gs = [MlpLayerGrads() for _ in layers]
    # the pooled cotangents are read as strided halves of the [B, 2C] gradients: no copies
    dmmax = dmavg = dumean = dumax = None
    if dpooled is not None:
        dpooled = dpooled if dpooled.stride(1) == 1 else dpooled.contiguous()
        dmmax, dmavg = dpooled[:, :C], dpooled[:, C:]
    if dupooled is not None:
        dupooled = dupooled if dupooled.stride(1) == 1 else dupooled.contiguous()
        dumean, dumax = dupooled[:, :C], dupooled[:, C:]
    if dpf is not None:
        dpf = dpf.contiguous()
    # output layer: in front of the TN wgrad (its dgrad is then split too) dz goes straight out as an sx8 operand
    # and its column sum (the bias gradient) follows from the [B, C] cotangents
    cots = (dmmax, dmavg, dumean, dumax)
    if routes[nh].wgrad == "tn":
        dz, dz_s = None, pools.bwd(valid, cnt, arg_m, arg_u, cots, dpf, C, sx8=True)
        Gs[nh].b = pools.colsum(valid, ctx.nvalid, cnt, arg_m, arg_u, cots, dpf, C)
    else:
        dz = pools.bwd(valid, cnt, arg_m, arg_u, cots, dpf, C)
        dz_s = None
    # per-point MLP backward, output layer first.  Entering iteration i: dz = grad wrt the
    # pre-LN output of Linear i in fp32 and / or, on a split dgrad, dz_s = the same in sx8.
    for i in range(nh, -1, -1):
        r, (W, _, g, be), G = routes[i], layers[i], Gs[i]
        if r.wgrad == "first":
            # layer 0: LN/ReLU backward, bias and WEIGHT gradient in one pass over (dh, z); dz is never written
            G.gamma, G.beta, G.b, G.W = ops.ln_act_bwd_first(dh, zs[i], x2, stats[i][0], stats[i][1], g, be, ACT_RELU,
                                                             drop_p=ps[i], seed=sd[i])
            break
        if i < nh:
            mu, rs = stats[i]
            dz_s = torch.empty_like(dh) if r.dgrad == "split" else None
            dz, G.gamma, G.beta, G.b = ops.ln_act_bwd(
                dh, zs[i], mu, rs, g, be, ACT_RELU, ps[i], sd[i], inplace=True, dz_split=dz_s, want_dz=_dz32(r))
        elif dz is not None:
            G.b = ops.colsum(dz)
            if r.dgrad == "split":
                dz_s = ops.split_rows(dz)
        if i > 0:
            prev = layers[i - 1]
            h, pro, h_s = zs[i - 1], Pro(ACT_RELU, stats[i - 1][0], stats[i - 1][1], prev.gamma, prev.beta, ps[i - 1], sd[i - 1]), hs[i - 1]
        else:
            h, pro, h_s = x2, None, None
        G.W = _wgrad(r, dz, dz_s, h, pro, h_s, npr)
        if r.wgrad == "tn" and not config.RETAIN_SAVED:
            hs[i - 1] = None
        if r.dgrad is not None:
            dh = _dgrad(r, dz, dz_s, W, ctx.wT.get(i), npr)
        del dz, dz_s
        dz = dz_s = None
    dx = dh if routes[0].dgrad is not None else None
    if not config.RETAIN_SAVED:
        ctx.saved = None
    return dx, [g for G in Gs for g in G.out()][:len(ctx.params)]            # the output layer has no gamma, beta


class EncoderFn(torch.autograd.Function):
    """x[B,N,Din], params -> (pooled[B,2C] = [masked max | masked mean], point_features[B,N,C],
    upooled[B,2C] = [unmasked mean | unmasked max]).

    params = [W_i, b_i, gamma_i, beta_i]*n_hidden + [W_out, b_out]   (the per-point shared MLP), optionally followed
    by one Drop(ps, seed): train-mode dropout at mlp.{4i+3} (see Drop)
    upooled holds the UNMASKED pools the vertex head needs, already in its concatenation order
    (VertexPredictor.py:86-88), produced by the same pass as the masked ones.  The fusion MLP is its own Function (FusionFn) so that
    its gradients are handed to autograd — and to the data-parallel reducer — before the long
    per-point backward starts.

    precision "bf16x3": layers whose input width is a multiple of 8 consume the previous
    layer's relu(LN(z)) as an sx8 split operand produced by wf3d_ln_prep (which also
    yields the LN statistics), through wf3d_gemm_split; backward uses split GEMMs for
    dgrad (W^T in sx8) and wgrad (transposed sx8 operands).  Only z and (mu, rstd) are
    kept for backward in either mode.  precision "bf16": the same GEMMs on the same operands with
    one bf16 MFMA per product (hi planes only); backward uses the forward's mode (ctx.products)."""

    @staticmethod
    def forward(ctx, x, n_hidden, precision, *params):
        B, N, Din = x.shape
        M = B * N
        x2 = x.reshape(M, Din)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        po, pf = _encoder_forward(ctx, x2, _DensePools(B, N), n_hidden, precision, params)
        ctx.dims = (B, N, pf.shape[1])
        return po.masked, pf.view(B, N, -1), po.unmasked

    @staticmethod
    def backward(ctx, dpooled, dpf, dupooled):
        B, N, _ = ctx.dims
        dx, grads = _encoder_backward(ctx, dpooled, dpf, dupooled)
        return (None if dx is None else dx.view(B, N, -1), None, None, *grads, *[None] * ctx.n_extra)


class EncoderFnPacked(torch.autograd.Function):
    """EncoderFn on a packed batch: x [M, Din] = the clouds concatenated along the point axis, `layout` the
    ops.PackedLayout of their point counts -> (pooled [B, 2C], point_features [M, C], upooled [B, 2C]), each cloud's those
    of EncoderFn on that cloud alone.  With a capacity layout (host or device counts) x is [capacity, Din], its rows past
    the live total finite and otherwise arbitrary, and point_features is [capacity, C].  The per-point MLP runs over M_pad rows (M rounded up to ops.ROW_PAD, so that every
    route of _encoder_routes stays available whatever the counts); the pad rows have zero input, belong to no cloud, are
    never read by the pools and get exact zeros from their backward, so they add exact zeros to every gradient.
    ctx.saved is EncoderFn's, over the M_pad rows.  The packed input takes no gradient."""

    @staticmethod
    def forward(ctx, x, layout, n_hidden, precision, *params):
        return EncoderFnPacked._forward(ctx, "compute", x, layout, n_hidden, precision, *params)

    @staticmethod
    def _forward(ctx, tail, x, layout, n_hidden, precision, *params):
        if ctx.needs_input_grad[0]:
            raise RuntimeError("wf3d: a packed batch that requires grad is not supported (detach the points)")
        M, Din = x.shape
        x2 = x
        if layout.M_pad != M:
            x2 = x.new_zeros(layout.M_pad, Din)
            x2[:M].copy_(x)
        po, pf = _encoder_forward(ctx, x2, _PackedPools(layout), n_hidden, precision, params, tail)
        return po.masked, pf[:M], po.unmasked

    @staticmethod
    def backward(ctx, dpooled, dpf, dupooled):
        _, grads = _encoder_backward(ctx, dpooled, dpf, dupooled)
        return (None, None, None, None, *grads, *[None] * ctx.n_extra)


class EncoderFnPackedSkip(torch.autograd.Function):
    """EncoderFnPacked in tail="skip" mode: with a capacity layout whose routes all honour a live-row count
    (_encoder_live) the per-point MLP stops, forward and backward, at the 256-row boundary R256 above the live row total
    that the layout holds on the device.  Rows >= R256 of x are then not read (they may hold anything), rows >= R256 of
    point_features are unspecified, and rows >= R256 of a gradient arriving for point_features are not read; the skipped
    rows are pad rows, whose backward is exact zeros, so every other output and every gradient equals EncoderFnPacked's
    bit for bit.  Any other layout or route runs exactly as EncoderFnPacked."""

    @staticmethod
    def forward(ctx, x, layout, n_hidden, precision, *params):
        return EncoderFnPacked._forward(ctx, "skip", x, layout, n_hidden, precision, *params)

    backward = staticmethod(EncoderFnPacked.backward)


class FusionFn(torch.autograd.Function):
    """pooled[B,2C] -> global[B,C]: feature_fusion (PointNetEncoder.py:57-65,116).
    params = [F0w, F0b, F1g, F1b, F3w, F3b, F4g, F4b, F6w, F6b]

    B <= 32 rows: three launches of the weight-streaming skinny kernel forward, six backward
    (csrc/skinny.hip); otherwise the generic GEMM path."""

    @staticmethod
    def forward(ctx, pooled, *params):
        pooled = pooled if pooled.stride(1) == 1 else pooled.contiguous()
        M = pooled.shape[0]
        _keep_params(ctx, params)
        P = FusionParams(*params)
        ctx.skinny = sk.ok(M, P.F0w, P.F3w, P.F6w) and P.F0w.shape[0] % 16 == 0 and P.F3w.shape[0] % 16 == 0 \
            and pooled.stride(0) % 4 == 0
        if ctx.skinny:
            (f0, p0, _), = sk.fwd(M, sk.Fwd(pooled, P.F0w, P.F0b, stats=True))
            (f3, p3, s0), = sk.fwd(M, sk.Fwd(f0, P.F3w, P.F3b, ln=sk.LNIn(P.F1g, P.F1b, ACT_RELU, part=p0), stats=True))
            (gl, _, s3), = sk.fwd(M, sk.Fwd(f3, P.F6w, P.F6b, ln=sk.LNIn(P.F4g, P.F4b, ACT_RELU, part=p3)))
        else:
            f0 = ops.gemm(pooled, P.F0w, NT, bias=P.F0b)
            s0 = ops.row_stats(f0)
            f3 = ops.gemm(f0, P.F3w, NT, bias=P.F3b, pro=Pro(ACT_RELU, s0[0], s0[1], P.F1g, P.F1b))
            s3 = ops.row_stats(f3)
            gl = ops.gemm(f3, P.F6w, NT, bias=P.F6b, pro=Pro(ACT_RELU, s3[0], s3[1], P.F4g, P.F4b))
        ctx.saved = (pooled, f0, s0, f3, s3)
        return gl

    @staticmethod
    def backward(ctx, dgl):
        P = FusionParams(*_params(ctx))
        pooled, f0, s0, f3, s3 = _saved(ctx)
        G = FusionGrads()
        dgl = dgl.contiguous()
        if ctx.skinny:
            M = dgl.shape[0]
            l3 = sk.LNIn(P.F4g, P.F4b, ACT_RELU, mu=s3[0], rs=s3[1])
            l0 = sk.LNIn(P.F1g, P.F1b, ACT_RELU, mu=s0[0], rs=s0[1])
            (G.F6w, G.F6b, sl), = sk.bwd(M, sk.Bwd(dgl, P.F6w, f3, x_ln=l3))
            _, g3, G.F4g, G.F4b, rp3 = sk.reduce(M, P.F6w.shape[1], [sl], want_dh=False, ln=(f3, s3[0], s3[1], P.F4g, P.F4b, ACT_RELU))
            (G.F3w, G.F3b, sl), = sk.bwd(M, sk.Bwd(g3, P.F3w, f0, ln_out=sk.LNOut(f3, s3[0], s3[1], rp3), x_ln=l0))
            _, g0, G.F1g, G.F1b, rp0 = sk.reduce(M, P.F3w.shape[1], [sl], want_dh=False, ln=(f0, s0[0], s0[1], P.F1g, P.F1b, ACT_RELU))
            (G.F0w, G.F0b, sl), = sk.bwd(M, sk.Bwd(g0, P.F0w, pooled, ln_out=sk.LNOut(f0, s0[0], s0[1], rp0)))
            dpooled, *_ = sk.reduce(M, P.F0w.shape[1], [sl])
        else:
            G.F6b = ops.colsum(dgl)
            G.F6w, dh = _lin_bwd(dgl, f3, P.F6w, Pro(ACT_RELU, s3[0], s3[1], P.F4g, P.F4b))
            dz, G.F4g, G.F4b, G.F3b = ops.ln_act_bwd(dh, f3, s3[0], s3[1], P.F4g, P.F4b, ACT_RELU, inplace=True)
            G.F3w, dh = _lin_bwd(dz, f0, P.F3w, Pro(ACT_RELU, s0[0], s0[1], P.F1g, P.F1b))
            dz, G.F1g, G.F1b, G.F0b = ops.ln_act_bwd(dh, f0, s0[0], s0[1], P.F1g, P.F1b, ACT_RELU, inplace=True)
            G.F0w, dpooled = _lin_bwd(dz, pooled, P.F0w, None)
        if not config.RETAIN_SAVED:
            ctx.saved = None
        return (dpooled, *G.out())


# ===========================================================================
# Vertex head
# ===========================================================================
class VertexFn(torch.autograd.Function):
    """(g[B,C], upooled[B,2C] = [mean | max] or None, params) -> (vertices[B,V,3] (view of o[B,V,vd]), exist[B,V], counts[B] int64)

    params = [W1,b1,g1,be1, W2,b2,g2,be2, W3,b3,g3,be3, W4,b4,g4,be4, Wf,bf, Wr1,br1, Wr2,br2, (Wpp,bpp)]

    B <= 32 rows: six weight-streaming launches forward (the three Linears that read `e` share one; the residual sums
    c = relu(LN(z3)) + r1, d = relu(LN(z4)) + r2 are applied on load and never materialised), thirteen backward
    (csrc/skinny.hip); otherwise the generic GEMM path.

    params may end in one Drop(ps, seed): train-mode dropout at vertex_mlp{k}.3, k = 1..4, on relu(LN(z_k)) — before the
    residual add for k = 3, 4 (VertexPredictor.py:110,114) — with row = sample index.  While a site is active the stage
    takes the generic GEMM path whatever B is (the skinny kernels draw no masks); with none active the choice is
    unchanged."""

    @staticmethod
    def forward(ctx, g, upooled, V, vd, *params):
        rest, *ctx.drop = _take_drop(params, 4, "VertexFn")
        ctx.n_extra = len(params) - len(rest)                    # a trailing Drop takes a (None) gradient slot
        with _seeded(ctx.drop[2]):
            return VertexFn._forward(ctx, g, upooled, V, vd, *rest)

    @staticmethod
    def _forward(ctx, g, upooled, V, vd, *params):
        ps, sd, _ = ctx.drop
        g = g.contiguous()
        B = g.shape[0]
        P = VertexParams(*params)
        if upooled is not None:
            upooled = upooled if upooled.stride(1) == 1 else upooled.contiguous()
        mats = [P.W1, P.W2, P.W3, P.W4, P.Wf, P.Wr1, P.Wr2] + ([P.Wpp] if upooled is not None else [])
        ctx.skinny = sk.ok(B, *mats) and all(w.shape[0] % 16 == 0 for w in (P.W1, P.W2, P.W3, P.W4)) \
            and (upooled is None or upooled.stride(0) % 4 == 0) and not any(ps)
        if ctx.skinny:
            if upooled is not None:
                (e, _, _), = sk.fwd(B, sk.Fwd(upooled, P.Wpp, P.bpp, out_add=g))     # enhanced = g + proj (:99-100)
            else:
                e = g
            (z1, p1, _), (r1, _, _), (r2, _, _) = sk.fwd(B, sk.Fwd(e, P.W1, P.b1, stats=True), sk.Fwd(e, P.Wr1, P.br1), sk.Fwd(e, P.Wr2, P.br2))
            (z2, p2, s1), = sk.fwd(B, sk.Fwd(z1, P.W2, P.b2, ln=sk.LNIn(P.g1, P.be1, ACT_RELU, part=p1), stats=True))
            (z3, p3, s2), = sk.fwd(B, sk.Fwd(z2, P.W3, P.b3, ln=sk.LNIn(P.g2, P.be2, ACT_RELU, part=p2), stats=True))
            # residual after the ReLU (:110,:114), applied on load
            (z4, p4, s3), = sk.fwd(B, sk.Fwd(z3, P.W4, P.b4, ln=sk.LNIn(P.g3, P.be3, ACT_RELU, part=p3), in_add=r1, stats=True))
            (o, _, s4), = sk.fwd(B, sk.Fwd(z4, P.Wf, P.bf, ln=sk.LNIn(P.g4, P.be4, ACT_RELU, part=p4), in_add=r2))
            c, d = r1, r2
        else:
            if upooled is not None:
                e = ops.gemm(upooled, P.Wpp, NT, bias=P.bpp, addend=g)
            else:
                e = g
            z1 = ops.gemm(e, P.W1, NT, bias=P.b1); s1 = ops.row_stats(z1)
            z2 = ops.gemm(z1, P.W2, NT, bias=P.b2, pro=Pro(ACT_RELU, s1[0], s1[1], P.g1, P.be1, ps[0], sd[0])); s2 = ops.row_stats(z2)
            z3 = ops.gemm(z2, P.W3, NT, bias=P.b3, pro=Pro(ACT_RELU, s2[0], s2[1], P.g2, P.be2, ps[1], sd[1])); s3 = ops.row_stats(z3)
            r1 = ops.gemm(e, P.Wr1, NT, bias=P.br1)
            # residual after the ReLU and its dropout (:110)
            c = ops.ln_act_apply(z3, s3[0], s3[1], P.g3, P.be3, ACT_RELU, addend=r1, drop_p=ps[2], seed=sd[2])
            z4 = ops.gemm(c, P.W4, NT, bias=P.b4); s4 = ops.row_stats(z4)
            r2 = ops.gemm(e, P.Wr2, NT, bias=P.br2)
            d = ops.ln_act_apply(z4, s4[0], s4[1], P.g4, P.be4, ACT_RELU, addend=r2, drop_p=ps[3], seed=sd[3])
            o = ops.gemm(d, P.Wf, NT, bias=P.bf)
        exist, counts = ops.vertex_finalize_fwd(o, V, vd)
        _keep_params(ctx, params)
        ctx.dims = (B, V, vd)
        # skinny path: c / d hold r1 / r2 (the sums are rebuilt on load)
        ctx.saved = (upooled, e, z1, s1, z2, s2, z3, s3, c, z4, s4, d)
        ctx.save_for_backward(exist)
        ctx.mark_non_differentiable(counts)
        # `vertices` = the first three channels, a non-contiguous view as in the reference (VertexPredictor.py:122); handing
        # the view out directly spares autograd's slice backward (a zero-fill and a strided copy per step)
        return o.view(B, V, vd)[:, :, :3], exist, counts

    @staticmethod
    def backward(ctx, do3, dexist, _dcounts):
        with _seeded(ctx.drop[2]):
            de, dupooled, G = VertexFn._backward(ctx, do3, dexist)
        if not config.RETAIN_SAVED:
            ctx.saved = None
        # Wpp, bpp take a slot only when they were passed
        return (de, dupooled, None, None, *G.out()[:len(ctx.params)], *[None] * ctx.n_extra)

    @staticmethod
    def _backward(ctx, do3, dexist):
        ps, sd, _ = ctx.drop
        B, V, vd = ctx.dims
        P = VertexParams(*_params(ctx))
        pooled, e, z1, s1, z2, s2, z3, s3, c, z4, s4, d = _saved(ctx)
        (exist,) = ctx.saved_tensors
        G = VertexGrads()
        do = ops.vertex_finalize_bwd(exist, dexist.contiguous() if dexist is not None else None,
                                     do3.contiguous() if do3 is not None else None, B, V, vd)
        if ctx.skinny:
            r1, r2 = c, d
            R = ACT_RELU
            ln = [None, sk.LNIn(P.g1, P.be1, R, mu=s1[0], rs=s1[1]), sk.LNIn(P.g2, P.be2, R, mu=s2[0], rs=s2[1]),
                  sk.LNIn(P.g3, P.be3, R, mu=s3[0], rs=s3[1]), sk.LNIn(P.g4, P.be4, R, mu=s4[0], rs=s4[1])]
            # final layer: input d = relu(LN(z4)) + r2
            (G.Wf, G.bf, sl), = sk.bwd(B, sk.Bwd(do, P.Wf, z4, x_ln=ln[4], x_add=r2))
            dd, G4, G.g4, G.be4, rp4 = sk.reduce(B, P.Wf.shape[1], [sl], ln=(z4, s4[0], s4[1], P.g4, P.be4, R))
            # residual_proj2 (plain dz = dd) and vertex_mlp4 (input c = relu(LN(z3)) + r1) in one launch
            (G.Wr2, G.br2, sl_e2), (G.W4, G.b4, sl) = sk.bwd(
                B, sk.Bwd(dd, P.Wr2, e), sk.Bwd(G4, P.W4, z3, ln_out=sk.LNOut(z4, s4[0], s4[1], rp4), x_ln=ln[3], x_add=r1))
            dc, G3, G.g3, G.be3, rp3 = sk.reduce(B, P.W4.shape[1], [sl], ln=(z3, s3[0], s3[1], P.g3, P.be3, R))
            (G.Wr1, G.br1, sl_e1), (G.W3, G.b3, sl) = sk.bwd(
                B, sk.Bwd(dc, P.Wr1, e), sk.Bwd(G3, P.W3, z2, ln_out=sk.LNOut(z3, s3[0], s3[1], rp3), x_ln=ln[2]))
            _, G2, G.g2, G.be2, rp2 = sk.reduce(B, P.W3.shape[1], [sl], want_dh=False, ln=(z2, s2[0], s2[1], P.g2, P.be2, R))
            (G.W2, G.b2, sl), = sk.bwd(B, sk.Bwd(G2, P.W2, z1, ln_out=sk.LNOut(z2, s2[0], s2[1], rp2), x_ln=ln[1]))
            _, G1, G.g1, G.be1, rp1 = sk.reduce(B, P.W2.shape[1], [sl], want_dh=False, ln=(z1, s1[0], s1[1], P.g1, P.be1, R))
            (G.W1, G.b1, sl_e0), = sk.bwd(B, sk.Bwd(G1, P.W1, e, ln_out=sk.LNOut(z1, s1[0], s1[1], rp1)))
            de, *_ = sk.reduce(B, P.W1.shape[1], [sl_e0, sl_e1, sl_e2])
            dupooled = None
            if pooled is not None:
                (G.Wpp, G.bpp, sl), = sk.bwd(B, sk.Bwd(de, P.Wpp, pooled))
                dupooled, *_ = sk.reduce(B, P.Wpp.shape[1], [sl])
            return de, dupooled, G
        G.bf = ops.colsum(do)
        G.Wf, dd = _lin_bwd(do, d, P.Wf, None)
        # d = relu(LN(z4)) + r2
        G.br2 = ops.colsum(dd)
        G.Wr2 = ops.gemm(dd, e, TN)
        de = ops.gemm(dd, P.Wr2, NN)
        dz4, G.g4, G.be4, G.b4 = ops.ln_act_bwd(dd, z4, s4[0], s4[1], P.g4, P.be4, ACT_RELU, ps[3], sd[3])
        G.W4, dc = _lin_bwd(dz4, c, P.W4, None)
        # c = relu(LN(z3)) + r1
        G.br1 = ops.colsum(dc)
        G.Wr1 = ops.gemm(dc, e, TN)
        ops.gemm(dc, P.Wr1, NN, out=de, accumulate=True)
        dz3, G.g3, G.be3, G.b3 = ops.ln_act_bwd(dc, z3, s3[0], s3[1], P.g3, P.be3, ACT_RELU, ps[2], sd[2])
        G.W3, dh = _lin_bwd(dz3, z2, P.W3, Pro(ACT_RELU, s2[0], s2[1], P.g2, P.be2, ps[1], sd[1]))
        dz2, G.g2, G.be2, G.b2 = ops.ln_act_bwd(dh, z2, s2[0], s2[1], P.g2, P.be2, ACT_RELU, ps[1], sd[1], inplace=True)
        G.W2, dh = _lin_bwd(dz2, z1, P.W2, Pro(ACT_RELU, s1[0], s1[1], P.g1, P.be1, ps[0], sd[0]))
        dz1, G.g1, G.be1, G.b1 = ops.ln_act_bwd(dh, z1, s1[0], s1[1], P.g1, P.be1, ACT_RELU, ps[0], sd[0], inplace=True)
        G.W1 = ops.gemm(dz1, e, TN)
        ops.gemm(dz1, P.W1, NN, out=de, accumulate=True)
        dupooled = None
        if pooled is not None:
            G.bpp = ops.colsum(de)
            G.Wpp = ops.gemm(de, pooled, TN)
            dupooled = ops.gemm(de, P.Wpp, NN)
        return de, dupooled, G


# ===========================================================================
# Edge head (all samples of the batch in one pass, ragged)
# ===========================================================================
def _edge_vertex_section(verts, meta, heads, x3, P, drop_ps=(0.0, 0.0), seeds=(0, 0)):
    """The per-vertex section of the edge head (sum-of-counts rows): vertex_proj, attention with its residual, and the
    two projections Pa / Pb of edge_mlp.0 that the pair combine adds per edge.  EdgeFn._forward and infer.edge_stream
    both run it on their EdgeParams block P; drop_ps / seeds: the stage's, of which vertex_proj.5 and attention lead.
    Returns cv, za, sa, zb, sb, f, qkv, cx, lse, Fm, Pa, Pb."""
    M0w, H = P.M0w, P.P3w.shape[0]
    cv = ops.edge_gather_verts(verts, meta)
    za = ops.gemm(cv, P.P0w, NT, bias=P.P0b); sa = ops.row_stats(za)
    # per-vertex Linears: in bf16x3 mode the fp32 operands are split inside the GEMM's staging pass (x3), forward and
    # backward; the K = 3 coordinate products stay exact fp32
    zb = ops.gemm(za, P.P3w, NT, bias=P.P3b, pro=Pro(ACT_GELU, sa[0], sa[1], P.P1g, P.P1b), x3=x3); sb = ops.row_stats(zb)
    f = ops.ln_act_apply(zb, sb[0], sb[1], P.P4g, P.P4b, ACT_NONE, drop_p=drop_ps[0], seed=seeds[0])
    qkv = ops.gemm(f, P.Aw, NT, bias=P.Ab, x3=x3)
    cx, lse = ops.attn_fwd(qkv, meta, H, heads, drop_ps[1], seeds[1])
    Fm = ops.gemm(cx, P.Ow, NT, bias=P.Ob, addend=f, x3=x3)              # residual (EdgePredictor.py:114)
    vd = cv.shape[1]                                   # coordinates per vertex (EdgePredictor(vertex_dim=...): 3 in the model)
    Wa, Wb, Wc, Wd = M0w[:, :H], M0w[:, H:2 * H], M0w[:, 2 * H:2 * H + vd], M0w[:, 2 * H + vd:2 * H + 2 * vd]
    if vd <= 4:
        # the coordinate columns ride on the two GEMMs as a rank-vd epilogue term (exact fp32)
        Pa = ops.gemm(Fm, Wa, NT, bias=P.M0b, x3=x3, lowrank=(cv, Wc))
        Pb = ops.gemm(Fm, Wb, NT, x3=x3, lowrank=(cv, Wd))
    else:
        Pa = ops.gemm(Fm, Wa, NT, bias=P.M0b, x3=x3)
        ops.gemm(cv, Wc, NT, out=Pa, accumulate=True)
        Pb = ops.gemm(Fm, Wb, NT, x3=x3)
        ops.gemm(cv, Wd, NT, out=Pb, accumulate=True)
    return cv, za, sa, zb, sb, f, qkv, cx, lse, Fm, Pa, Pb


class EdgeFn(torch.autograd.Function):
    """verts[B,V,3] (view ok) -> edge_probs[B, max_E] zero-padded.

    `counts` is a tuple of host ints, or a padded ops.EdgeMeta built on the device (EdgeMeta.device): then every
    launch covers the worst-case B*V vertex and B*V(V-1)/2 edge rows, max_E = V(V-1)/2, and the kernels keep the rows
    past the live totals finite in forward and zero in backward (include/wf3d.h, "PADDED layouts").

    params = the fields of EdgeParams (vertex_proj.{0,1,3,4}, attention.{in_proj,out_proj}, edge_mlp.{0,1,4,5,8,10})

    params may end in one Drop(ps, seed): train-mode dropout at vertex_proj.5, attention, edge_mlp.3 and edge_mlp.7.  With
    the device seed words of wf3d.random (dropout_rng "device") the four site seeds are indices 1..4 into those words,
    which every mask kernel of the forward and of the backward loads at run time."""

    @staticmethod
    def forward(ctx, verts, counts, heads, precision, *params):
        rest, *ctx.drop = _take_drop(params, 4, "EdgeFn")
        ctx.n_extra = len(params) - len(rest)
        with _seeded(ctx.drop[2]):
            return EdgeFn._forward(ctx, verts, counts, heads, precision, *rest)

    @staticmethod
    def _forward(ctx, verts, counts, heads, precision, *params):
        P = EdgeParams(*params)
        ps, sd, _ = ctx.drop
        _, _, p1_, p2_ = ps                                 # vertex_proj.5, attention, edge_mlp.3, edge_mlp.7
        B, V, _ = verts.shape
        H = P.P3w.shape[0]
        # counts: host ints, or an EdgeMeta already built on the device (EdgePredictor.forward_padded)
        meta = counts if isinstance(counts, ops.EdgeMeta) else ops.EdgeMeta.get(counts, verts.device)
        x3 = precision == "bf16x3" and config.EDGE_X3
        cv, za, sa, zb, sb, f, qkv, cx, lse, Fm, Pa, Pb = _edge_vertex_section(verts, meta, heads, x3, P, ps, sd)
        npr = _SPLIT_PRODUCTS.get(precision, 3)
        routes = _edge_routes(meta.Re, H, precision, x3)
        # decided once, here; backward only reads it (and the logits kernel chosen below)
        rowdot = P.M10w.shape[0] == 1 and P.M10w.is_contiguous() and ops.rowdot_act_shape_ok(H // 4)
        ctx.live = live = _edge_live(meta, routes, rowdot)
        # the launches over meta.Re edge rows: pair combine, edge_mlp.4 / .8 / .10, sigmoid
        with ops.live_rows(live):
            if routes[0].fwd == "split":
                # the pair kernel holds each edge row in registers: it also emits gelu(LN(pre)) as the next GEMM's operand.
                # `pre` itself (2 KB per edge row) is stored only when something in backward reads it: with the wgrad of the
                # second edge layer on the transposing-read kernel (operand h1) and the LayerNorm backward rebuilding the
                # row from Pa / Pb (ops.edge_pair_ln_bwd, H <= 1024), nothing does.
                keep_pre = routes[0].wgrad not in _TN or H > 1024
                pre, mu0, rs0, delta, h1 = ops.edge_pair_fwd(Pa, Pb, cv, P.M0w, meta, ln=(P.M1g, P.M1b, ACT_GELU, p1_, sd[2]), keep_pre=keep_pre)
                (M4s, M4t), (M8s, M8t) = ops.split_weights([P.M4w, P.M8w])
                z2 = ops.gemm_split(h1, M4s, bias=P.M4b, products=npr)
                mu2, rs2, h2 = ops.ln_prep(z2, P.M5g, P.M5b, ACT_GELU, drop_p=p2_, seed=sd[3])
                s2 = (mu2, rs2)
                z3 = ops.gemm_split(h2, M8s, bias=P.M8b, products=npr)
            else:
                pre, mu0, rs0, delta = ops.edge_pair_fwd(Pa, Pb, cv, P.M0w, meta)
                h1 = h2 = M4t = M8t = None
                z2 = ops.gemm(pre, P.M4w, NT, bias=P.M4b, pro=Pro(ACT_GELU, mu0, rs0, P.M1g, P.M1b, p1_, sd[2]), x3=x3); s2 = ops.row_stats(z2)
                z3 = ops.gemm(z2, P.M8w, NT, bias=P.M8b, pro=Pro(ACT_GELU, s2[0], s2[1], P.M5g, P.M5b, p2_, sd[3]), x3=x3)
            fused_tail = ops.rowdot_act_ok(z3, P.M10w)
            assert fused_tail or live is None           # the count was chosen for the row-dot kernel: no fp32 GEMM under it
            if fused_tail:
                logit = ops.rowdot_act(z3, P.M10w, P.M10b, ACT_GELU)          # one-output Linear: a row dot product, not a GEMM
            else:
                logit = ops.gemm(z3, P.M10w, NT, bias=P.M10b, pro=Pro(ACT_GELU))
            probs = ops.edge_prob_fwd(logit, meta)
        if pre is not None:
            Pa = Pb = None
        _keep_params(ctx, params)
        ctx.cfg = (B, V, H, heads, meta)
        ctx.routes, ctx.wT, ctx.x3, ctx.products, ctx.fused_tail = routes, (M4t, M8t), x3, npr, fused_tail
        ctx.saved = (cv, za, sa, zb, sb, f, qkv, cx, lse, Fm, pre, mu0, rs0, delta, z2, s2, z3, h1, h2, Pa, Pb)
        ctx.save_for_backward(probs)
        return probs

    @staticmethod
    def backward(ctx, dprobs):
        # autograd's own thread: the seed source is set again here (the _Leaves side stream runs inside it)
        with _seeded(ctx.drop[2]):
            return (*EdgeFn._backward(ctx, dprobs), *[None] * ctx.n_extra)

    @staticmethod
    def _backward(ctx, dprobs):
        P = EdgeParams(*_params(ctx))
        B, V, H, heads, meta = ctx.cfg
        (pf_, pa_, p1_, p2_), sd, _ = ctx.drop
        cv, za, sa, zb, sb, f, qkv, cx, lse, Fm, pre, mu0, rs0, delta, z2, s2, z3, h1, h2, Pa, Pb = _saved(ctx)
        (probs,) = ctx.saved_tensors
        G = EdgeGrads()
        x3, npr = ctx.x3, ctx.products
        # weight / bias gradients run beside the dgrad chain while the launches are small enough to share the chip
        # (cfg2, 64.5 k edge rows: +0.7 % on the step; cfg5, 1.04 M rows: -1.3 %, every kernel fills it alone)
        lv = _Leaves(dprobs.device, enable=meta.Re <= (1 << 18))
        # the edge-row section: under the live-row count the forward chose (autograd runs this in its own thread, so it is
        # set again here; the _Leaves side stream runs inside the same thread)
        with ops.live_rows(ctx.live):
            dlogit = ops.edge_prob_bwd(probs, dprobs.contiguous(), meta)                      # [Re,1]
            G.M10b = ops.colsum(dlogit)
            fused_tail = ctx.fused_tail
            if fused_tail:
                dh3 = z3            # shape / dtype stand-in: the fused kernel below produces dz3 directly
            elif P.M10w.shape[0] == 1:
                # one-output Linear: dW[c] = sum_r dlogit[r]*gelu(z3[r,c]) is a weighted column sum,
                # d gelu(z3) = dlogit (outer) W — no 128x128 MFMA tile wasted on a 1-wide problem
                G.M10w = ops.colsum(z3, dlogit.view(-1), ACT_GELU).view(1, -1)
                dh3 = ops.gemm(dlogit, P.M10w, NN)
            else:
                G.M10w, dh3 = _lin_bwd(dlogit, z3, P.M10w, Pro(ACT_GELU))
            p2 = Pro(ACT_GELU, s2[0], s2[1], P.M5g, P.M5b, p2_, sd[3])
            p1 = Pro(ACT_GELU, mu0, rs0, P.M1g, P.M1b, p1_, sd[2])
            r2, r3 = ctx.routes

            def wgrad(r, dz, dz_s, h, pro, h_s):
                return lv.run(lambda: _wgrad(r, dz, dz_s, h, pro, h_s, npr), dz_s, dz, h_s if r.wgrad in _TN else h)
            # edge_mlp.8, then edge_mlp.4: dz in sx8 for split dgrads, in fp32 where a consumer reads it
            dz3_s = torch.empty_like(dh3) if r3.dgrad == "split" else None            # dz3 has dh3's shape
            if fused_tail:
                # logits-layer backward + GELU backward + both column sums in one pass over z3
                dz3, G.M10w, G.M8b = ops.rowdot_act_bwd(z3, dlogit, P.M10w, ACT_GELU, want_dz=_dz32(r3), dz_split=dz3_s)
            else:
                dz3, _, _, G.M8b = ops.ln_act_bwd(dh3, z3, None, None, None, None, ACT_GELU, inplace=True,
                                                  dz_split=dz3_s, want_dz=_dz32(r3))
            G.M8w = wgrad(r3, dz3, dz3_s, z2, p2, h2)
            dh2 = _dgrad(r3, dz3, dz3_s, P.M8w, ctx.wT[1], npr)
            del dz3, dz3_s
            dz2_s = torch.empty_like(dh2) if r2.dgrad == "split" else None
            dz2, G.M5g, G.M5b, G.M4b = ops.ln_act_bwd(dh2, z2, s2[0], s2[1], P.M5g, P.M5b, ACT_GELU, p2_, sd[3],
                                                      inplace=True, dz_split=dz2_s, want_dz=_dz32(r2))
            G.M4w = wgrad(r2, dz2, dz2_s, pre, p1, h1)
            dh1 = _dgrad(r2, dz2, dz2_s, P.M4w, ctx.wT[0], npr)
            del dz2, dz2_s
            # LN/GELU backward of the first edge layer; the same pass yields the gradient of its distance-weight column
            if pre is None:
                dpre, G.M1g, G.M1b, wsum = ops.edge_pair_ln_bwd(dh1, Pa, Pb, delta, P.M0w, meta, mu0, rs0, P.M1g, P.M1b, ACT_GELU, p1_, sd[2])
            else:
                dpre, G.M1g, G.M1b, wsum = ops.ln_act_bwd_wsum(dh1, pre, delta, mu0, rs0, P.M1g, P.M1b, ACT_GELU, p1_, sd[2], inplace=True)
            # split first layer backward
            vd = cv.shape[1]
            dW0 = torch.empty_like(P.M0w)           # every column is written below: Wa | Wb | Wc | Wd | w_delta
            dW0[:, 2 * H + 2 * vd].copy_(wsum)
            dPa, dPb, dcv = ops.edge_pair_bwd(dpre, delta, cv, P.M0w, meta, coord=True)     # dcv includes dPa·Wc + dPb·Wd

        def first_layer_leaves():
            ops.gemm(dPa, Fm, TN, out=dW0[:, :H], x3=x3)
            ops.gemm(dPb, Fm, TN, out=dW0[:, H:2 * H], x3=x3)
            ops.gemm(dPa, cv, TN, out=dW0[:, 2 * H:2 * H + vd])
            ops.gemm(dPb, cv, TN, out=dW0[:, 2 * H + vd:2 * H + 2 * vd])
            return ops.colsum(dPa)
        G.M0b = lv.run(first_layer_leaves, dPa, dPb, Fm, cv, dW0)
        G.M0w = dW0
        Wa, Wb = P.M0w[:, :H], P.M0w[:, H:2 * H]
        dF = ops.gemm(dPa, Wa, NN, x3=x3)
        ops.gemm(dPb, Wb, NN, out=dF, accumulate=True, x3=x3)
        # F = f + out_proj(ctx)
        G.Ob, G.Ow = lv.run(lambda: (ops.colsum(dF), ops.gemm(dF, cx, TN, x3=x3)), dF, cx)
        dcx = ops.gemm(dF, P.Ow, NN, x3=x3)
        dqkv = ops.attn_bwd(qkv, dcx, cx, lse, meta, H, heads, pa_, sd[1])
        G.Ab, G.Aw = lv.run(lambda: (ops.colsum(dqkv), ops.gemm(dqkv, f, TN, x3=x3)), dqkv, f)
        df = ops.gemm(dqkv, P.Aw, NN, addend=dF, x3=x3)
        # f = drop(LN(zb))
        dzb, G.P4g, G.P4b, G.P3b = ops.ln_act_bwd(df, zb, sb[0], sb[1], P.P4g, P.P4b, ACT_NONE, pf_, sd[0], inplace=True)
        pa = Pro(ACT_GELU, sa[0], sa[1], P.P1g, P.P1b)
        G.P3w = lv.run(lambda: ops.gemm(dzb, za, TN, pro=pa, x3=x3), dzb, za)
        dha = ops.gemm(dzb, P.P3w, NN, x3=x3)
        dza, G.P1g, G.P1b, G.P0b = ops.ln_act_bwd(dha, za, sa[0], sa[1], P.P1g, P.P1b, ACT_GELU, inplace=True)
        G.P0w = lv.run(lambda: ops.gemm(dza, cv, TN), dza, cv)
        ops.gemm(dza, P.P0w, NN, out=dcv, accumulate=True)
        lv.join(G.M8w, G.M4w, G.M0b, dW0, G.Ob, G.Ow, G.Ab, G.Aw, G.P3w, G.P0w)
        dverts = ops.edge_scatter_dverts(dcv, meta, B, V)
        if not config.RETAIN_SAVED:
            ctx.saved = None
        return (dverts, None, None, None, *G.out())


class _FrozenList(list):
    """A list that refuses in-place mutation.  edge_index_lists hands the SAME cached object to every
    sample and every forward with that vertex count (the reference builds fresh lists each call,
    EdgePredictor.py:88-89,140 — 63 ms per sample at V=256); a caller that filtered one in place would
    corrupt every later forward, so mutation raises instead.  Compares equal to / converts like a list."""
    __slots__ = ()

    def _ro(self, *a, **k):
        raise TypeError("edge_indices lists are shared between calls and read-only: copy first "
                        "(e.g. [list(p) for p in out['edge_indices'][i]])")

    append = extend = insert = remove = pop = clear = sort = reverse = _ro
    __setitem__ = __delitem__ = __iadd__ = __imul__ = _ro


class EdgeIndexLists(Sequence):
    """`edge_indices` of a padded edge head: a read-only sequence over the batch that equals
    edge_index_lists(counts).  The counts stay on the device until the first access reads them (one device->host
    copy); len() needs no read."""
    __slots__ = ("_counts", "_lists")

    def __init__(self, counts):
        self._counts, self._lists = counts, None

    def _get(self):
        if self._lists is None:
            self._lists = edge_index_lists([int(c) for c in self._counts.tolist()])
        return self._lists

    def __len__(self):
        return int(self._counts.shape[0])

    def __getitem__(self, i):
        return self._get()[i]

    def __eq__(self, other):
        return list(self._get()) == list(other)

    def __repr__(self):
        return repr(self._get())

    def _ro(self, *a, **k):
        raise TypeError("edge_indices is read-only: copy first (e.g. [list(p) for p in out['edge_indices'][i]])")

    append = extend = insert = remove = pop = clear = sort = reverse = _ro
    __setitem__ = __delitem__ = __iadd__ = __imul__ = _ro
    __hash__ = None


_EDGE_LIST_CACHE = {}          # vertex count -> _FrozenList of _FrozenList([i, j]); LRU, bounded
_EDGE_LIST_CACHE_MAX = 128     # 2.6 MB of host memory per entry at V=256


def edge_index_lists(counts):
    """Per-sample list of [i, j] pairs, i < j, lexicographic — bit-identical to
    EdgePredictor._get_edge_indices(...).tolist() (reference :70-89,140), but
    built once per vertex count and cached (LRU) instead of re-looped on every call."""
    out = []
    for c in counts:
        lst = _EDGE_LIST_CACHE.pop(c, None)
        if lst is None:
            lst = _FrozenList(_FrozenList((i, j)) for i in range(c) for j in range(i + 1, c))
            if len(_EDGE_LIST_CACHE) >= _EDGE_LIST_CACHE_MAX:
                _EDGE_LIST_CACHE.pop(next(iter(_EDGE_LIST_CACHE)))
        _EDGE_LIST_CACHE[c] = lst          # (re-)insert as most recently used
        out.append(lst)
    return out


class UnmaskedPoolFn(torch.autograd.Function):
    """point_features[B,N,C] -> [mean_n | max_n] as one [B, 2C] tensor: the vertex head's own pooling and its
    concatenation (VertexPredictor.py:86-88) when it is used outside PointCloudToWireframe."""

    @staticmethod
    def forward(ctx, pf):
        pf = pf.contiguous()
        B, N, C = pf.shape
        ones = torch.ones(B * N, dtype=torch.float32, device=pf.device)
        po = ops.pool4_fwd(pf, ones, packed=True)
        ctx.dims, ctx.saved = (B, N, C), (ones, po.cnt, po.arg_m, po.arg_u)
        return po.unmasked

    @staticmethod
    def backward(ctx, dup):
        B, N, C = ctx.dims
        ones, cnt, arg_m, arg_u = _saved(ctx)
        dup = dup if dup.stride(1) == 1 else dup.contiguous()
        return ops.pool4_bwd(ones, cnt, arg_m, arg_u, None, None, dup[:, :C], dup[:, C:], None, B, N, C)
