"""Thin torch-tensor wrappers over the C ABI (one Python function per entry
point of include/wf3d.h).  torch is used for device memory and the current
stream only; every FLOP happens in libwf3d.so.  CPU tensors are rejected —
there is no fallback path.
"""
import contextlib
import ctypes
import threading

import torch

from . import _lib
from ._lib import GemmDesc, check

ACT_NONE, ACT_RELU, ACT_GELU = (_lib.DEFINES["WF3D_ACT_" + n] for n in ("NONE", "RELU", "GELU"))
NT, NN, TN = (_lib.DEFINES["WF3D_" + n] for n in ("NT", "NN", "TN"))
LN_EPS = 1e-5

_scratch = {}


def _need_cuda(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("wf3d: the HIP path needs CUDA (ROCm) tensors; there is no CPU fallback")
        if t.dtype not in (torch.float32, torch.int32, torch.int64):
            raise RuntimeError(f"wf3d: unsupported dtype {t.dtype}")


def _p(t):
    # plain int (or None): every pointer parameter is declared c_void_p in _lib.SIGNATURES, ctypes converts
    return None if t is None else t.data_ptr()


try:                                     # raw handle of the current stream without building a Stream object (~10x cheaper;
    _raw_stream = torch._C._cuda_getCurrentRawStream      # the heads issue ~200 launches of 5-20 us per step: CPU-bound there)
except AttributeError:                   # pragma: no cover
    _raw_stream = None


def _stream():
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def scratch(nbytes, device, slot=0):
    """Grow-only per-(device, stream, slot) scratch buffer.  Kernels run in
    stream order, so reuse across consecutive calls on one stream is safe."""
    if nbytes <= 0:
        return None
    key = (device.index, _stream(), slot)
    buf = _scratch.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _scratch[key] = buf
    return buf


def _row_bufs(what, R, *bufs):
    """Caller-provided per-row outputs: contiguous float32 [R] device tensors."""
    for t in bufs:
        _need_cuda(t)
        if t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != R or not t.is_contiguous():
            raise RuntimeError(f"wf3d.{what}: an out buffer must be a contiguous float32 [{R}] tensor")


def _rows2d(t):
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise RuntimeError("wf3d: expected a 2-D tensor with unit inner stride")
    return t


_tls = threading.local()


@contextlib.contextmanager
def live_rows(rows):
    """Edge-row launches on this thread inside the block run under a live-row count (wf3d_set_live_rows,
    include/wf3d.h "LIVE ROW COUNT"): `rows` is a one-element int32 device tensor that the kernels read when they run,
    so a captured block follows the value of each replay.  rows = None: no count (also inside an outer block, for
    launches over other rows)."""
    if rows is not None:
        _need_cuda(rows)
        if rows.dtype != torch.int32 or rows.numel() != 1:
            raise RuntimeError("wf3d.live_rows: needs a one-element int32 device tensor")
    prev = getattr(_tls, "live", None)
    ptr = rows.data_ptr() if rows is not None else None
    if ptr == prev:
        yield
        return
    lib = _lib.load()
    check(lib.wf3d_set_live_rows(ptr), "set_live_rows")
    _tls.live = ptr
    try:
        yield
    finally:
        check(lib.wf3d_set_live_rows(prev), "set_live_rows")
        _tls.live = prev


class Pro:
    """Prologue spec for `gemm`: v' = drop(act(LN-affine(v))) on the activation operand."""
    __slots__ = ("act", "mu", "rs", "gamma", "beta", "drop_p", "seed")

    def __init__(self, act, mu=None, rs=None, gamma=None, beta=None, drop_p=0.0, seed=0):
        self.act, self.mu, self.rs, self.gamma, self.beta = act, mu, rs, gamma, beta
        self.drop_p, self.seed = float(drop_p), int(seed) & 0xFFFFFFFF


def gemm(a, b, layout, bias=None, addend=None, out=None, accumulate=False, pro=None, x3=False, lowrank=None):
    """C = pro(A)·B (+bias) (+addend) (+C).  NT: a[M,K] b[N,K]; NN: a[M,K] b[K,N]; TN: a[K,M] b[K,N].
    x3=True: bf16x3 arithmetic on the fp32 operands (split while staged; see wf3d_gemm_t.x3); default exact fp32.
    lowrank=(U[M,k], V[N,k]), k <= 4: C += U·V^T in the epilogue (exact fp32; unit inner stride, any row stride)."""
    _need_cuda(a, b, bias, addend, out)
    a, b = _rows2d(a), _rows2d(b)
    if layout == NT:
        M, K = a.shape; N, K2 = b.shape
    elif layout == NN:
        M, K = a.shape; K2, N = b.shape
    elif layout == TN:
        K, M = a.shape; K2, N = b.shape
    else:
        raise ValueError("bad layout")
    if K != K2:
        raise RuntimeError(f"wf3d.gemm: reduction dims differ ({K} vs {K2})")
    if out is None:
        if accumulate:
            raise RuntimeError("wf3d.gemm: accumulate needs `out`")
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    else:
        _rows2d(out)
        if tuple(out.shape) != (M, N):
            raise RuntimeError(f"wf3d.gemm: out shape {tuple(out.shape)} != {(M, N)}")
    if bias is not None and (bias.numel() != N or not bias.is_contiguous()):
        raise RuntimeError("wf3d.gemm: bias must be contiguous [N]")
    if addend is not None:
        _rows2d(addend)
        if tuple(addend.shape) != (M, N):
            raise RuntimeError("wf3d.gemm: addend shape mismatch")
    d = GemmDesc()
    d.A, d.B, d.C = _p(a), _p(b), _p(out)
    d.bias, d.addend = _p(bias), _p(addend)
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = a.stride(0) if a.shape[0] > 1 else max(a.shape[1], 1), \
        b.stride(0) if b.shape[0] > 1 else max(b.shape[1], 1), out.stride(0) if M > 1 else max(N, 1)
    d.ld_addend = (addend.stride(0) if M > 1 else N) if addend is not None else 0
    d.layout = layout
    if pro is not None:
        if layout == NN:
            raise RuntimeError("wf3d.gemm: no prologue on NN")
        rows, cols = (M, K) if layout == NT else (K, N)
        for nm, t, n in (("mu", pro.mu, rows), ("rs", pro.rs, rows), ("gamma", pro.gamma, cols), ("beta", pro.beta, cols)):
            if t is not None:
                _need_cuda(t)
                if t.numel() != n or not t.is_contiguous():
                    raise RuntimeError(f"wf3d.gemm: prologue {nm} must be contiguous [{n}]")
        d.pro_enable, d.pro_act = 1, pro.act
        d.pro_mu, d.pro_rs, d.pro_gamma, d.pro_beta = _p(pro.mu), _p(pro.rs), _p(pro.gamma), _p(pro.beta)
        d.drop_p, d.drop_seed = pro.drop_p, pro.seed
    d.accumulate = 1 if accumulate else 0
    d.x3 = 1 if x3 else 0
    if lowrank is not None:
        u, v = lowrank
        _need_cuda(u, v)
        if u.dim() != 2 or v.dim() != 2 or u.shape[0] != M or v.shape[0] != N or u.shape[1] != v.shape[1] or u.shape[1] > 4 \
                or u.stride(1) != 1 or v.stride(1) != 1:
            raise RuntimeError("wf3d.gemm: lowrank needs U[M,k], V[N,k] with k <= 4 and unit inner stride")
        d.lr_u, d.lr_v, d.lr_k = _p(u), _p(v), u.shape[1]
        d.ld_lr_u, d.ld_lr_v = u.stride(0) if M > 1 else u.shape[1], v.stride(0) if N > 1 else v.shape[1]
    lib = _lib.load()
    nb = lib.wf3d_gemm_ws_bytes(M, N, K, layout)
    ws = scratch(nb, a.device)
    d.ws, d.ws_bytes = _p(ws), (ws.numel() if ws is not None else 0)
    if M and N:
        check(lib.wf3d_gemm(ctypes.byref(d), _stream()), "gemm")
    return out


def row_stats(z, eps=LN_EPS, out=None):
    """(mu, rs) of the rows of z; out = (mu, rs): contiguous float32 [R] buffers to write instead of new ones."""
    _need_cuda(z)
    z = _rows2d(z)
    R, D = z.shape
    if out is not None:
        mu, rs = out
        _row_bufs("row_stats", R, mu, rs)
    else:
        mu = torch.empty(R, dtype=torch.float32, device=z.device)
        rs = torch.empty(R, dtype=torch.float32, device=z.device)
    ld = z.stride(0) if R > 1 else D
    check(_lib.load().wf3d_row_stats(_p(z), R, D, ld, eps, _p(mu), _p(rs), _stream()), "row_stats")
    return mu, rs


def ln_act_apply(z, mu, rs, gamma, beta, act, addend=None, drop_p=0.0, seed=0, out=None):
    _need_cuda(z, mu, rs, gamma, beta, addend)
    if not z.is_contiguous() or (addend is not None and not addend.is_contiguous()):
        raise RuntimeError("wf3d.ln_act_apply: contiguous tensors required")
    R, D = z.shape
    if out is None:
        out = torch.empty_like(z)
    check(_lib.load().wf3d_ln_act_apply(_p(z), R, D, _p(mu), _p(rs), _p(gamma), _p(beta), act, _p(addend),
                                        float(drop_p), int(seed) & 0xFFFFFFFF, _p(out), _stream()), "ln_act_apply")
    return out


def ln_act_bwd(dh, z, mu, rs, gamma, beta, act, drop_p=0.0, seed=0, want_affine=True, want_bias=True, inplace=False,
               dz_split=None, want_dz=True):
    """Returns (dz, dgamma, dbeta, dbias); `dz_split` (optional sx8 buffer) also receives dz, and
    with want_dz=False the fp32 dz is not written at all (returned as None)."""
    _need_cuda(dh, z, mu, rs, gamma, beta)
    if not (dh.is_contiguous() and z.is_contiguous()):
        raise RuntimeError("wf3d.ln_act_bwd: contiguous tensors required")
    R, D = z.shape
    if not want_dz and dz_split is None:
        raise RuntimeError("wf3d.ln_act_bwd: want_dz=False needs dz_split")
    dz = None if not want_dz else (dh if inplace else torch.empty_like(z))
    dev = z.device
    if want_affine and gamma is not None and want_bias:
        # one [3, D] buffer -> the C side finalises all three column sums in a single pass
        trio = torch.empty(3, D, dtype=torch.float32, device=dev)
        dgamma, dbeta, dbias = trio[0], trio[1], trio[2]
    else:
        dgamma = torch.empty(D, dtype=torch.float32, device=dev) if (want_affine and gamma is not None) else None
        dbeta = torch.empty(D, dtype=torch.float32, device=dev) if (want_affine and gamma is not None) else None
        dbias = torch.empty(D, dtype=torch.float32, device=dev) if want_bias else None
    lib = _lib.load()
    ws = scratch(lib.wf3d_ln_act_bwd_ws_bytes(R, D), dev)
    check(lib.wf3d_ln_act_bwd(_p(dh), _p(z), R, D, _p(mu), _p(rs), _p(gamma), _p(beta), act, float(drop_p),
                              int(seed) & 0xFFFFFFFF, _p(dz), _p(dz_split), _p(dgamma), _p(dbeta), _p(dbias), _p(ws),
                              ws.numel() if ws is not None else 0, _stream()), "ln_act_bwd")
    return dz, dgamma, dbeta, dbias


def ln_act_bwd_wsum(dh, z, wrow, mu, rs, gamma, beta, act, drop_p=0.0, seed=0, inplace=False):
    """(dz, dgamma, dbeta, wsum) with wsum[c] = sum_r dz[r, c] * wrow[r] from the same pass."""
    _need_cuda(dh, z, wrow, mu, rs, gamma, beta)
    if not (dh.is_contiguous() and z.is_contiguous() and wrow.is_contiguous()):
        raise RuntimeError("wf3d.ln_act_bwd_wsum: contiguous tensors required")
    R, D = z.shape
    dz = dh if inplace else torch.empty_like(z)
    duo = torch.empty(2, D, dtype=torch.float32, device=z.device)
    wsum = torch.empty(D, dtype=torch.float32, device=z.device)
    lib = _lib.load()
    ws = scratch(lib.wf3d_ln_act_bwd_wsum_ws_bytes(R, D), z.device)
    check(lib.wf3d_ln_act_bwd_wsum(_p(dh), _p(z), _p(wrow), R, D, _p(mu), _p(rs), _p(gamma), _p(beta), act, float(drop_p),
                                   int(seed) & 0xFFFFFFFF, _p(dz), None, _p(duo[0]), _p(duo[1]), _p(wsum), _p(ws),
                                   ws.numel(), _stream()), "ln_act_bwd_wsum")
    return dz, duo[0], duo[1], wsum


def colsum(x, w=None, act=ACT_NONE):
    """out[c] = sum_r act(x[r, c]) * w[r]"""
    _need_cuda(x, w)
    x = _rows2d(x)
    R, D = x.shape
    out = torch.empty(D, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    ws = scratch(lib.wf3d_colsum_ws_bytes(R, D), x.device)
    ld = x.stride(0) if R > 1 else D
    check(lib.wf3d_colsum(_p(x), R, D, ld, _p(w), act, _p(out), _p(ws), ws.numel() if ws is not None else 0, _stream()),
          "colsum")
    return out


def rowdot_act_ok(z, W):
    """The row-dot kernels take a one-output Linear on a contiguous [R, D] with D = 8 * 2^k <= 512."""
    return (W.shape[0] == 1 and z.dim() == 2 and z.is_contiguous() and W.is_contiguous()
            and bool(_lib.load().wf3d_rowdot_act_ok(z.shape[1])))


def rowdot_act_shape_ok(D):
    """The same width test from the shape alone (before z exists)."""
    return bool(_lib.load().wf3d_rowdot_act_ok(D))


def rowdot_act(z, W, bias, act, out=None):
    """[R, 1] = act(z) @ W^T + bias for a one-output Linear W [1, D].  out: a contiguous float32 buffer of R elements to
    write instead of a new one."""
    _need_cuda(z, W, bias, out)
    R, D = z.shape
    if out is None:
        out = torch.empty(R, 1, dtype=torch.float32, device=z.device)
    elif out.dtype != torch.float32 or out.numel() != R or not out.is_contiguous():
        raise RuntimeError(f"wf3d.rowdot_act: out must be a contiguous float32 buffer of {R} elements")
    check(_lib.load().wf3d_rowdot_act(_p(z), R, D, _p(W), _p(bias), act, _p(out), _stream()), "rowdot_act")
    return out


def rowdot_act_bwd(z, dlogit, W, act, want_dz=True, dz_split=None):
    """Backward of rowdot_act fused with the activation backward: (dz | None, dW [1, D], dbias_z [D]);
    `dz_split` (optional sx8 buffer) also receives dz."""
    _need_cuda(z, dlogit, W, dz_split)
    R, D = z.shape
    if not want_dz and dz_split is None:
        raise RuntimeError("wf3d.rowdot_act_bwd: want_dz=False needs dz_split")
    dz = torch.empty_like(z) if want_dz else None
    duo = torch.empty(2, D, dtype=torch.float32, device=z.device)
    lib = _lib.load()
    ws = scratch(lib.wf3d_rowdot_act_bwd_ws_bytes(R, D), z.device)
    check(lib.wf3d_rowdot_act_bwd(_p(z), _p(dlogit), R, D, _p(W), act, _p(dz), _p(dz_split), _p(duo[0]), _p(duo[1]),
                                  _p(ws), ws.numel(), _stream()), "rowdot_act_bwd")
    return dz, duo[0].view(1, D), duo[1]


def point_valid(x, out=None):
    _need_cuda(x)
    if not x.is_contiguous():
        raise RuntimeError("wf3d.point_valid: contiguous input required")
    M, D = x.numel() // x.shape[-1], x.shape[-1]
    if out is not None:
        _row_bufs("point_valid", M, out)
    valid = out if out is not None else torch.empty(M, dtype=torch.float32, device=x.device)
    check(_lib.load().wf3d_point_valid(_p(x), M, D, _p(valid), _stream()), "point_valid")
    return valid


class PoolOut:
    """Everything one pooling pass yields.  `masked` = [masked max | masked mean] and `unmasked` = [mean | max] are
    [B, 2C] tensors in the order the reference concatenates them (PointNetEncoder.py:115, VertexPredictor.py:88);
    mmax/mavg/umean/umax are views of their halves."""
    __slots__ = ("masked", "unmasked", "mmax", "mavg", "umean", "umax", "arg_m", "arg_u", "cnt", "nvalid")

    def __init__(self, B, C, dev, argmax=True):
        """Uninitialised outputs of B clouds x C channels for a pooling launch to fill."""
        self.masked = torch.empty(B, 2 * C, dtype=torch.float32, device=dev)
        self.unmasked = torch.empty(B, 2 * C, dtype=torch.float32, device=dev)
        self.mmax, self.mavg = self.masked[:, :C], self.masked[:, C:]
        self.umean, self.umax = self.unmasked[:, :C], self.unmasked[:, C:]
        self.arg_m = torch.empty(B, C, dtype=torch.int32, device=dev) if argmax else None
        self.arg_u = torch.empty(B, C, dtype=torch.int32, device=dev) if argmax else None
        cn = torch.empty(2, B, dtype=torch.float32, device=dev)
        self.cnt, self.nvalid = cn[0], cn[1]


def pool4_fwd(pf, valid, packed=False):
    """pf [B,N,C], valid [B*N] -> (mmax, mavg, umean, umax, arg_m, arg_u, cnt), or a PoolOut with packed=True."""
    _need_cuda(pf, valid)
    if not pf.is_contiguous():
        raise RuntimeError("wf3d.pool4_fwd: contiguous point_features required")
    B, N, C = pf.shape
    dev = pf.device
    o = PoolOut(B, C, dev)
    lib = _lib.load()
    ws = scratch(lib.wf3d_pool4_ws_bytes(B, N, C), dev)
    check(lib.wf3d_pool4_fwd(_p(pf), _p(valid), B, N, C, _p(o.mmax), _p(o.mavg), _p(o.umean), _p(o.umax), 2 * C,
                             _p(o.arg_m), _p(o.arg_u), _p(o.cnt), _p(o.nvalid), _p(ws), ws.numel(), _stream()), "pool4_fwd")
    if packed:
        return o
    return o.mmax, o.mavg, o.umean, o.umax, o.arg_m, o.arg_u, o.cnt


def _pair_ld(a, b, what):
    """Row stride shared by a pair of [B, C] cotangents (the two halves of one [B, 2C] gradient, or contiguous)."""
    ld = None
    for t in (a, b):
        if t is None:
            continue
        if t.dim() != 2 or t.stride(1) != 1:
            raise RuntimeError(f"wf3d.pool4_bwd: {what} cotangents need unit inner stride")
        s = t.stride(0) if t.shape[0] > 1 else t.shape[1]
        if ld is not None and s != ld:
            raise RuntimeError(f"wf3d.pool4_bwd: the two {what} cotangents must share one row stride")
        ld = s
    return ld or 0


def pool4_bwd(valid, cnt, arg_m, arg_u, dmmax, dmavg, dumean, dumax, dpf_direct, B, N, C, sx8=False):
    """sx8=True: the result is written as an sx8 split operand (C % 8 == 0) instead of fp32.  The cotangents may be
    strided views (halves of a [B, 2C] gradient)."""
    _need_cuda(valid, cnt, arg_m, arg_u, dmmax, dmavg, dumean, dumax, dpf_direct)
    if dpf_direct is not None and not dpf_direct.is_contiguous():
        raise RuntimeError("wf3d.pool4_bwd: contiguous dpf_direct required")
    ldm, ldu = _pair_ld(dmmax, dmavg, "masked"), _pair_ld(dumean, dumax, "unmasked")
    dpf = torch.empty(B, N, C, dtype=torch.float32, device=valid.device)
    fn = _lib.load().wf3d_pool4_bwd_sx8 if sx8 else _lib.load().wf3d_pool4_bwd
    check(fn(_p(valid), _p(cnt), _p(arg_m), _p(arg_u), _p(dmmax), _p(dmavg), ldm, _p(dumean), _p(dumax), ldu,
             _p(dpf_direct), B, N, C, _p(dpf), _stream()), "pool4_bwd")
    return dpf


def pool4_bwd_colsum(nvalid, cnt, arg_m, arg_u, dmmax, dmavg, dumean, dumax, dpf_direct, B, N, C):
    """Column sums over all B*N rows of what pool4_bwd writes, from the [B, C] cotangents alone:
    sum_n of  valid*dmavg/cnt + dumean/N + [n==arg_m]*dmmax + [n==arg_u]*dumax  (+ dpf_direct).
    nvalid [B] = number of valid points per cloud (PoolOut.nvalid)."""
    _need_cuda(cnt, arg_m, arg_u, dmmax, dmavg, dumean, dumax, dpf_direct, nvalid)
    ldm, ldu = _pair_ld(dmmax, dmavg, "masked"), _pair_ld(dumean, dumax, "unmasked")
    out = torch.empty(C, dtype=torch.float32, device=cnt.device)
    check(_lib.load().wf3d_pool4_bwd_bias(_p(cnt), _p(nvalid), _p(arg_m), _p(arg_u), _p(dmmax), _p(dmavg), ldm, _p(dumean),
                                          _p(dumax), ldu, B, C, _p(out), _stream()), "pool4_bwd_bias")
    if dpf_direct is not None:              # point_features itself received a gradient (never on the model's own path)
        out += colsum(dpf_direct.view(B * N, C))
    return out


# ---------------------------------------------------------------------------
# packed batches: clouds of different lengths concatenated along the point axis
# ---------------------------------------------------------------------------
ROW_PAD = 256        # packed row totals are rounded up to this: every GEMM route of the encoder stays available


def point_counts_list(point_counts):
    """Per-cloud point counts as a validated list of Python ints (a list / tuple, or a CPU int tensor)."""
    if torch.is_tensor(point_counts):
        if point_counts.is_cuda:
            raise RuntimeError("wf3d: point counts are host values (a list or a CPU int tensor)")
        if point_counts.dim() != 1 or point_counts.dtype.is_floating_point:
            raise ValueError("wf3d: point_counts must be a 1-D integer tensor")
        point_counts = point_counts.tolist()
    counts = [int(c) for c in point_counts]
    if not counts:
        raise ValueError("wf3d: a packed batch needs at least one cloud")
    if min(counts) < 1:
        raise ValueError(f"wf3d: every cloud of a packed batch needs at least one point (got a count of {min(counts)})")
    if sum(counts) + ROW_PAD > 0x7FFFFFFF:
        raise ValueError("wf3d: the packed row total does not fit in int32")
    return counts


def check_capacity(capacity):
    """The row capacity of a packed batch as an int: a positive multiple of ROW_PAD that fits in int32."""
    if isinstance(capacity, bool) or not isinstance(capacity, int):
        raise ValueError(f"wf3d: capacity must be an int (got {capacity!r})")
    if capacity <= 0 or capacity % ROW_PAD or capacity > 0x7FFFFFFF:
        raise ValueError(f"wf3d: capacity must be a positive multiple of {ROW_PAD} below 2^31 (got {capacity})")
    return capacity


def chunk_rows_of(rows):
    """Rows per chunk of a packed batch of `rows` rows: about 256 chunks in all, at least 256 rows each."""
    return max(256, -(-(-(-rows // 256)) // 64) * 64)


def capacity_dims(B, capacity):
    """(chunk_rows, nchunk_cap) of a capacity table (include/wf3d.h, "PACKED batches, capacity form")."""
    chunk_rows = chunk_rows_of(capacity)
    return chunk_rows, -(-capacity // chunk_rows) + B + 1


class PackedLayout:
    """Row layout of a packed batch, from host point counts: cloud b owns rows offsets[b] .. offsets[b+1]-1 of the
    [M_pad, ...] tensors, M = sum of the counts, M_pad = M rounded up to ROW_PAD; rows M .. M_pad-1 belong to no cloud.

    `chunks` [nchunk_bwd, 4] = (cloud, its first row, r0, r1) cuts every cloud into pieces of at most `chunk_rows` rows,
    about 256 pieces in all whatever the counts, so that a long and a short cloud both spread over the chip
    (include/wf3d.h, "PACKED batches"); chunk_offsets[b] .. chunk_offsets[b+1]-1 are cloud b's.  The last entry, when
    M_pad > M, is the pad rows' (-1, 0, M, M_pad).  The host arrays are numpy; to(device) puts them into device memory in
    one asynchronous copy from pinned memory (nothing is read back), get() caches that per (device, counts, capacity):
    use get().

    With `capacity` (a multiple of ROW_PAD, >= M) the table is the capacity form's: M_pad = capacity, chunk_rows from
    capacity, and always capacity_dims(B, capacity)[1] entries, forward and backward alike — the clouds' chunks, the pad
    rows M .. capacity-1 in pieces of chunk_rows, then dead entries (-1, 0, capacity, capacity).  Every launch shape then
    depends on (B, capacity) alone, and DevicePackedLayout builds the same table, integer for integer, from counts in
    device memory.  `M_abi` is the M the pools' entry points are given (capacity in this form: they only check it)."""
    _cache = {}
    status = None                                       # DevicePackedLayout's clamp flags; host counts are validated

    def __init__(self, point_counts, capacity=None):
        import numpy as np
        self.counts = tuple(point_counts_list(point_counts))
        self.capacity = None if capacity is None else check_capacity(capacity)
        self.B = len(self.counts)
        self.offsets = np.zeros(self.B + 1, dtype=np.int32)
        np.cumsum(self.counts, out=self.offsets[1:])
        self.M = int(self.offsets[-1])
        if capacity is not None and self.M > capacity:
            raise ValueError(f"wf3d: point counts sum to {self.M}, above the capacity of {capacity} rows")
        self.M_pad = -(-self.M // ROW_PAD) * ROW_PAD if capacity is None else capacity
        self.M_abi = self.M if capacity is None else capacity
        self.chunk_rows = chunk_rows_of(self.M_pad if capacity is not None else self.M)
        chunks, coff = [], [0]
        for b, n in enumerate(self.counts):
            first = int(self.offsets[b])
            for r0 in range(first, first + n, self.chunk_rows):
                chunks.append((b, first, r0, min(r0 + self.chunk_rows, first + n)))
            coff.append(len(chunks))
        self.nchunk = len(chunks)                      # the clouds' chunks (forward)
        if capacity is not None:
            nchunk_cap = capacity_dims(self.B, capacity)[1]
            chunks += [(-1, 0, r0, min(r0 + self.chunk_rows, capacity)) for r0 in range(self.M, capacity, self.chunk_rows)]
            chunks += [(-1, 0, capacity, capacity)] * (nchunk_cap - len(chunks))
            assert len(chunks) == nchunk_cap
            self.nchunk = nchunk_cap                   # forward and backward walk the whole table
        elif self.M_pad > self.M:
            chunks.append((-1, 0, self.M, self.M_pad))
        self.nchunk_bwd = len(chunks)                  # ... and the pad rows' (backward)
        self.chunks = np.array(chunks, dtype=np.int32).reshape(-1, 4)
        self.chunk_offsets = np.array(coff, dtype=np.int32)
        self.device = None

    def row_map(self):
        """int32 [M_pad] host array: the cloud of every row, -1 for the pad rows.  An aid for callers and tests that slice
        per-row tensors by cloud; the kernels work from the chunk table and never see it."""
        import numpy as np
        m = np.full(self.M_pad, -1, dtype=np.int32)
        m[:self.M] = np.repeat(np.arange(self.B, dtype=np.int32), self.counts)
        return m

    def to(self, device):
        """Upload on the current stream; `ready` is recorded behind the copy so that use() can order other streams."""
        import numpy as np
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("wf3d: the row layout of these point counts would be built inside a graph capture (its upload "
                               "comes from a staging buffer that does not outlive the capture); run a warm-up step with the "
                               "same point counts before capturing")
        B = self.B
        a0 = -(-2 * (B + 1) // 4) * 4                  # the chunk table starts 16-byte aligned
        host = torch.zeros(a0 + 4 * self.nchunk_bwd, dtype=torch.int32).pin_memory()
        host[:B + 1] = torch.from_numpy(self.offsets)
        host[B + 1:2 * (B + 1)] = torch.from_numpy(self.chunk_offsets)
        host[a0:] = torch.from_numpy(np.ascontiguousarray(self.chunks).reshape(-1))
        buf = host.to(device, non_blocking=True)
        self.device = device
        self.d_rows, self.d_cchunk, self.d_chunks = buf[:B + 1], buf[B + 1:2 * (B + 1)], buf[a0:]
        self.ready = torch.cuda.Event()
        self.ready.record()
        return self

    def use(self):
        """Called before the layout's launches: until the upload is known to have finished, the current stream waits for
        it (the layout may be used from a stream other than the one that uploaded it).  Under a capture the layout is
        marked `captured`: the graph holds its device addresses, so get() never evicts it."""
        if torch.cuda.is_current_stream_capturing():
            self.captured = True
            self.ready = None                          # torch synchronizes the device when a capture begins
        elif self.ready is not None:
            if self.ready.query():
                self.ready = None
            else:
                torch.cuda.current_stream().wait_event(self.ready)
        return self

    captured = False
    _cache_max = 64

    @classmethod
    def get(cls, point_counts, device, capacity=None):
        """The layout of these counts (and this capacity) on `device`, built and uploaded on first use and kept in an LRU
        cache of _cache_max entries.  A layout that a graph capture has used is never evicted."""
        key = (device.index, tuple(int(c) for c in point_counts)) + (() if capacity is None else (capacity,))
        m = cls._cache.pop(key, None)
        if m is None:
            m = cls(point_counts, capacity).to(device)
            free = [k for k, v in cls._cache.items() if not v.captured]
            if len(free) >= cls._cache_max:
                del cls._cache[free[0]]
        cls._cache[key] = m                            # (re-)insert as most recently used
        return m.use()


class DevicePackedLayout:
    """The capacity form of PackedLayout with the table built on the device (wf3d_packed_layout_build) from a CUDA count
    tensor that is never read on the host: PackedLayout(counts, capacity)'s d_rows / d_cchunk / d_chunks for counts that
    pass its checks, clamped otherwise (`status`, one int32 on the device: bit 0 = clamped for capacity, bit 1 = some
    cloud has no rows).  The buffers belong to this object; build() may be called again with other counts.  The model
    allocates one per forward and keeps it for that forward's backward: a table shared between calls would be rewritten
    by a second forward before the first one's backward; under a graph capture the buffers come from the capture's
    pool, so a replay finds them where the capture left them."""
    counts = offsets = M = None                         # live values exist on the device only (d_rows)

    def __init__(self, B, capacity, device):
        self.capacity = self.M_pad = self.M_abi = check_capacity(capacity)
        if not 0 < B <= 65535:
            raise ValueError(f"wf3d: a packed batch on device counts holds 1..65535 clouds (got {B})")
        cr, nc = ctypes.c_int(), ctypes.c_int()
        check(_lib.load().wf3d_packed_layout_dims(B, capacity, ctypes.byref(cr), ctypes.byref(nc)), "packed_layout_dims")
        self.B, self.chunk_rows, self.nchunk = B, cr.value, nc.value
        self.nchunk_bwd = self.nchunk
        a0 = -(-2 * (B + 1) // 4) * 4                   # the chunk table starts 16-byte aligned, as PackedLayout.to's
        buf = torch.empty(a0 + 4 * self.nchunk + 1, dtype=torch.int32, device=device)
        self.device = device
        self.d_rows, self.d_cchunk, self.d_chunks = buf[:B + 1], buf[B + 1:2 * (B + 1)], buf[a0:a0 + 4 * self.nchunk]
        self.status = buf[a0 + 4 * self.nchunk:]

    def build(self, counts):
        """counts: CUDA int64 or int32 [B], contiguous.  One launch on the current stream; capturable."""
        _need_cuda(counts)
        if counts.dtype not in (torch.int64, torch.int32) or counts.dim() != 1 or counts.shape[0] != self.B \
                or not counts.is_contiguous():
            raise ValueError(f"wf3d: device point counts must be a contiguous int64 or int32 tensor [{self.B}]")
        lib = _lib.load()
        fn = lib.wf3d_packed_layout_build if counts.dtype == torch.int64 else lib.wf3d_packed_layout_build_i32
        check(fn(_p(counts), self.B, self.capacity, _p(self.d_rows), _p(self.d_cchunk), _p(self.d_chunks), _p(self.status),
                 _stream()), "packed_layout_build")
        return self


def pool4_seg_fwd(pf, valid, layout):
    """pf [M_pad, C], valid [M_pad], a PackedLayout or DevicePackedLayout on pf's device -> PoolOut of its B clouds (pool4_fwd(packed=True))."""
    _need_cuda(pf, valid)
    if pf.dim() != 2 or not pf.is_contiguous() or pf.shape[0] != layout.M_pad or valid.numel() != layout.M_pad:
        raise RuntimeError(f"wf3d.pool4_seg_fwd: contiguous point_features [{layout.M_pad}, C] and valid [{layout.M_pad}] required")
    B, C, dev = layout.B, pf.shape[1], pf.device
    o = PoolOut(B, C, dev)
    lib = _lib.load()
    ws = scratch(lib.wf3d_pool4_seg_ws_bytes(layout.nchunk, C), dev)
    check(lib.wf3d_pool4_seg_fwd(_p(pf), _p(valid), _p(layout.d_rows), _p(layout.d_cchunk), _p(layout.d_chunks), B, layout.M_abi,
                                 layout.nchunk, C, _p(o.mmax), _p(o.mavg), _p(o.umean), _p(o.umax), 2 * C, _p(o.arg_m),
                                 _p(o.arg_u), _p(o.cnt), _p(o.nvalid), _p(ws), ws.numel(), _stream()), "pool4_seg_fwd")
    return o


def pool4_seg_bwd(valid, cnt, arg_m, arg_u, dmmax, dmavg, dumean, dumax, dpf_direct, layout, C, sx8=False):
    """pool4_bwd of a packed batch: dpf [M_pad, C] (sx8=True: as an sx8 operand), its pad rows exact zeros.
    dpf_direct: [M, C] or [M_pad, C], contiguous ([capacity, C] for a capacity layout)."""
    _need_cuda(valid, cnt, arg_m, arg_u, dmmax, dmavg, dumean, dumax, dpf_direct)
    if dpf_direct is not None and not (dpf_direct.is_contiguous() and dpf_direct.dim() == 2 and dpf_direct.shape[1] == C
                                       and dpf_direct.shape[0] >= layout.M_abi):
        raise RuntimeError("wf3d.pool4_seg_bwd: contiguous dpf_direct with at least M rows required")
    ldm, ldu = _pair_ld(dmmax, dmavg, "masked"), _pair_ld(dumean, dumax, "unmasked")
    dpf = torch.empty(layout.M_pad, C, dtype=torch.float32, device=valid.device)
    fn = _lib.load().wf3d_pool4_seg_bwd_sx8 if sx8 else _lib.load().wf3d_pool4_seg_bwd
    check(fn(_p(valid), _p(cnt), _p(arg_m), _p(arg_u), _p(dmmax), _p(dmavg), ldm, _p(dumean), _p(dumax), ldu,
             _p(dpf_direct), _p(layout.d_rows), _p(layout.d_chunks), layout.B, layout.M_abi, layout.M_pad, layout.nchunk_bwd,
             layout.chunk_rows, C, _p(dpf), _stream()), "pool4_seg_bwd")
    return dpf


def pool4_seg_bwd_colsum(nvalid, cnt, arg_m, arg_u, dmmax, dmavg, dumean, dumax, dpf_direct, layout, C, valid=None):
    """Column sums over all rows of what pool4_seg_bwd writes.  The sum over a cloud's rows of its backward depends on
    the [B, C] cotangents alone, not on where the rows lie, so this is the dense form's kernel.  A capacity layout's live
    total may exist on the device only: with a dpf_direct (never on the model's own path) the sum is taken over what the
    backward writes (`valid` is needed for that), whose pad rows are zeros whatever dpf_direct holds there."""
    if dpf_direct is not None and layout.capacity is not None:
        if valid is None:
            raise RuntimeError("wf3d.pool4_seg_bwd_colsum: a capacity layout with a dpf_direct needs `valid`")
        return colsum(pool4_seg_bwd(valid, cnt, arg_m, arg_u, dmmax, dmavg, dumean, dumax, dpf_direct, layout, C))
    out = pool4_bwd_colsum(nvalid, cnt, arg_m, arg_u, dmmax, dmavg, dumean, dumax, None, layout.B, 0, C)
    if dpf_direct is not None:
        out += colsum(dpf_direct[:layout.M])
    return out


# ---------------------------------------------------------------------------
# streaming pools of the forward-only encoder (wf3d.infer)
# ---------------------------------------------------------------------------
class PoolStream:
    """The running 4-way pool of B clouds x C channels (include/wf3d.h, "STREAMING 4-way pool"): fold() the blocks of
    point_features as they pass, then finish().  `offsets`: int32 [B + 1] row offsets in device memory (a packed
    layout's d_rows; b * N for a dense batch); they are never read on the host."""

    def __init__(self, offsets, C):
        _need_cuda(offsets)
        if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.shape[0] < 2 or not offsets.is_contiguous():
            raise RuntimeError("wf3d.PoolStream: offsets must be a contiguous int32 [B + 1] device tensor")
        self.offsets, self.B, self.C = offsets, offsets.shape[0] - 1, int(C)
        lib = _lib.load()
        nb = lib.wf3d_pool4_stream_state_bytes(self.B, self.C)
        self.state = torch.empty(nb // 4, dtype=torch.float32, device=offsets.device)
        check(lib.wf3d_pool4_stream_init(_p(self.state), self.B, self.C, _stream()), "pool4_stream_init")

    def fold(self, pf, valid, r0):
        """pf [rows, C] (contiguous), valid [rows]: rows r0 .. r0 + rows - 1 of the flat row space."""
        _need_cuda(pf, valid)
        if pf.dim() != 2 or pf.shape[1] != self.C or not pf.is_contiguous() or pf.dtype != torch.float32:
            raise RuntimeError(f"wf3d.PoolStream.fold: contiguous float32 point_features [rows, {self.C}] required")
        rows = pf.shape[0]
        if valid.dtype != torch.float32 or valid.numel() != rows or not valid.is_contiguous():
            raise RuntimeError(f"wf3d.PoolStream.fold: valid must be a contiguous float32 [{rows}]")
        lib = _lib.load()
        ws = scratch(lib.wf3d_pool4_stream_ws_bytes(rows, self.C), pf.device)
        check(lib.wf3d_pool4_stream(_p(pf), _p(valid), _p(self.offsets), self.B, int(r0), rows, self.C, _p(self.state),
                                    _p(ws), ws.numel() if ws is not None else 0, _stream()), "pool4_stream")

    def finish(self):
        """PoolOut of the B clouds, without arg-max rows (arg_m = arg_u = None)."""
        o = PoolOut(self.B, self.C, self.state.device, argmax=False)
        check(_lib.load().wf3d_pool4_stream_finish(_p(self.state), _p(self.offsets), self.B, self.C, _p(o.mmax), _p(o.mavg),
                                                   _p(o.umean), _p(o.umax), 2 * self.C, _p(o.cnt), _p(o.nvalid), _stream()),
              "pool4_stream_finish")
        return o


# ---------------------------------------------------------------------------
# vertex-head tail and edge head
# ---------------------------------------------------------------------------
def vertex_finalize_fwd(o, V, vd):
    _need_cuda(o)
    B = o.shape[0]
    exist = torch.empty(B, V, dtype=torch.float32, device=o.device)
    counts = torch.empty(B, dtype=torch.int64, device=o.device)
    check(_lib.load().wf3d_vertex_finalize_fwd(_p(o), B, V, vd, _p(exist), _p(counts), _stream()), "vertex_finalize_fwd")
    return exist, counts


def vertex_finalize_bwd(exist, dexist, d_o_in, B, V, vd):
    """d_o_in: gradient of o [B, V, vd] or of the `vertices` view o[:, :, :3] ([B, V, 3]), contiguous, or None."""
    _need_cuda(exist, dexist, d_o_in)
    for t in (dexist, d_o_in):
        if t is not None and not t.is_contiguous():
            raise RuntimeError("wf3d.vertex_finalize_bwd: contiguous cotangents required")
    in_dim = d_o_in.shape[-1] if d_o_in is not None else vd
    d_o = torch.empty(B, V * vd, dtype=torch.float32, device=exist.device)
    check(_lib.load().wf3d_vertex_finalize_bwd(_p(exist), _p(dexist), _p(d_o_in), in_dim, B, V, vd, _p(d_o), _stream()),
          "vertex_finalize_bwd")
    return d_o


class EdgeMeta:
    """Compact ragged row layout of one batch: sample s owns vertex rows
    voff[s]..voff[s+1]-1 and edge rows eoff[s]..eoff[s+1]-1.

    Built from host ints (EdgeMeta(counts) / .get), or on the device from an int64 count tensor (EdgeMeta.device):
    then `padded` is True, the host sizes Rv, Re, vmax, max_e are the worst case of the padded width V, the rows past
    the live totals map to sample -1, and `counts` (clamped) and `width` (max_s E_s) are device tensors.  `live` is
    the live edge-row total, a one-element int32 view of eoff[B:] for ops.live_rows; `tail` says what the edge-row
    launches do with the rows past it: "compute" (all Re rows) or "skip" (EdgeFn runs them under `live`)."""
    _cache = {}
    padded = False
    live = None
    tail = "compute"

    @classmethod
    def device(cls, counts, B, V, tail="compute"):
        """Layout of int64 counts [B] (device memory, never read on the host) for a batch padded to V vertices: one
        launch of wf3d_edge_layout on the current stream, rebuilt on every call (and every replay of a capture)."""
        if tail not in ("compute", "skip"):
            raise ValueError("edge tail must be 'compute' or 'skip'")
        _need_cuda(counts)
        if counts.dtype != torch.int64 or counts.shape != (B,) or not counts.is_contiguous():
            raise RuntimeError(f"wf3d.EdgeMeta.device: counts must be a contiguous int64 [{B}] tensor")
        dev = counts.device
        E = V * (V - 1) // 2
        if B * E > 0x7FFFFFFF:
            raise RuntimeError(f"wf3d.EdgeMeta.device: B*V(V-1)/2 = {B * E} edge rows do not fit in int32")
        m = cls.__new__(cls)
        m.padded, m.tail = True, tail
        m.B, m.Rv, m.Re, m.vmax, m.max_e = B, B * V, B * E, V, E
        i32 = dict(dtype=torch.int32, device=dev)
        m.voff, m.eoff = torch.empty(B + 1, **i32), torch.empty(B + 1, **i32)
        m.vsample, m.esample = torch.empty(B * V, **i32), torch.empty(B * E, **i32)
        m.live = m.eoff[B:]
        m.counts = torch.empty(B, dtype=torch.int64, device=dev)
        m.width = torch.empty((), dtype=torch.int64, device=dev)
        check(_lib.load().wf3d_edge_layout(_p(counts), B, V, _p(m.voff), _p(m.eoff), _p(m.vsample), _p(m.esample),
                                           _p(m.counts), _p(m.width), _stream()), "edge_layout")
        return m

    def __init__(self, counts, device):
        self.counts = tuple(int(c) for c in counts)
        self.B = len(self.counts)
        ecount = [c * (c - 1) // 2 for c in self.counts]
        voff, eoff = [0], [0]
        for c, e in zip(self.counts, ecount):
            voff.append(voff[-1] + c)
            eoff.append(eoff[-1] + e)
        self.Rv, self.Re = voff[-1], eoff[-1]
        self.vmax = max(self.counts, default=0)
        self.max_e = max(ecount, default=0)
        i32 = dict(dtype=torch.int32, device=device)
        self.voff = torch.tensor(voff, **i32)
        self.eoff = torch.tensor(eoff, **i32)
        sid = torch.arange(self.B, **i32)
        self.vsample = torch.repeat_interleave(sid, torch.tensor(self.counts, dtype=torch.int64, device=device))
        self.esample = torch.repeat_interleave(sid, torch.tensor(ecount, dtype=torch.int64, device=device))

    @classmethod
    def get(cls, counts, device):
        key = (device.index, tuple(int(c) for c in counts))
        m = cls._cache.get(key)
        if m is None:
            if len(cls._cache) > 64:
                cls._cache.clear()
            m = cls._cache[key] = cls(counts, device)
        return m


def edge_gather_verts(verts, meta):
    """verts [B, V, d] (any strides with unit inner stride; d = vertex_dim, 1..8) -> cv [Rv, d]."""
    _need_cuda(verts)
    if verts.stride(2) != 1:
        raise RuntimeError("wf3d.edge_gather_verts: inner stride must be 1")
    d = verts.shape[2]
    cv = torch.empty(meta.Rv, d, dtype=torch.float32, device=verts.device)
    check(_lib.load().wf3d_edge_gather_verts(_p(verts), verts.stride(0), verts.stride(1), _p(meta.voff),
                                             _p(meta.vsample), meta.Rv, d, _p(cv), _stream()), "edge_gather_verts")
    return cv


def edge_scatter_dverts(dcv, meta, B, V):
    d = dcv.shape[1]
    out = torch.empty(B, V, d, dtype=torch.float32, device=dcv.device)
    check(_lib.load().wf3d_edge_scatter_dverts(_p(dcv), _p(meta.voff), B, V, d, _p(out), _stream()), "edge_scatter_dverts")
    return out


def attn_kernel(E, heads, vmax):
    """Which kernels serve attn_fwd / attn_bwd at these dims under the current options (wf3d_set_option "attn_tiled"):
    0 = VALU, 1 = MFMA with the sample resident in LDS (head width 64, vmax <= 256), 2 = MFMA key-tiled (head width 64
    beyond 256 vertices; head widths 68..128 at every vmax).  Needs no GPU."""
    k = _lib.load().wf3d_attn_kernel(int(E), int(heads), int(vmax))
    check(min(k, 0), "attn_kernel")
    return k


def attn_fwd(qkv, meta, E, heads, drop_p=0.0, seed=0):
    """(ctx [Rv, E], lse [Rv, heads]) of the self-attention over each sample's rows of qkv [Rv, 3E].  Head widths E / heads
    in 64..128 (multiples of 4) run on the matrix cores at any vertex count; widths up to 60 and above 128 on the VALU
    kernels, which refuse a width above 64 once its staged rows no longer fit the LDS (include/wf3d.h)."""
    _need_cuda(qkv)
    alloc = torch.zeros if meta.padded else torch.empty       # the kernels write real samples' rows only
    ctx = alloc(meta.Rv, E, dtype=torch.float32, device=qkv.device)
    lse = alloc(meta.Rv, heads, dtype=torch.float32, device=qkv.device)
    check(_lib.load().wf3d_attn_fwd(_p(qkv), _p(meta.voff), meta.B, meta.vmax, E, heads, float(drop_p),
                                    int(seed) & 0xFFFFFFFF, _p(ctx), _p(lse), _stream()), "attn_fwd")
    return ctx, lse


def attn_bwd(qkv, dctx, ctx, lse, meta, E, heads, drop_p=0.0, seed=0):
    """dqkv [Rv, 3E] from the forward's ctx and lse; served by the kernel family that served attn_fwd (attn_kernel)."""
    _need_cuda(qkv, dctx, ctx, lse)
    if not (dctx.is_contiguous() and ctx.is_contiguous()):
        raise RuntimeError("wf3d.attn_bwd: contiguous dctx / ctx required")
    dqkv = torch.zeros_like(qkv) if meta.padded else torch.empty_like(qkv)
    check(_lib.load().wf3d_attn_bwd(_p(qkv), _p(dctx), _p(ctx), _p(lse), _p(meta.voff), meta.B, meta.vmax, E, heads,
                                    float(drop_p), int(seed) & 0xFFFFFFFF, _p(dqkv), _stream()), "attn_bwd")
    return dqkv


_wdelta_cache = [None, -1, None]       # (weight tensor, its version, contiguous distance column)


def _wdelta(W0, H):
    """Distance column (the last one) of edge_mlp.0.weight [H, 2H + 2d + 1], gathered once into a contiguous vector (a
    strided per-lane gather of it inside the pair kernels costs 512 uncoalesced loads per edge row).
    Forward and backward of one step see the same weight version and share the copy."""
    if W0.dim() != 2 or W0.shape[0] != H or W0.shape[1] < 2 * H + 3 or (W0.shape[1] - 2 * H - 1) % 2:
        raise RuntimeError("wf3d: edge_mlp.0.weight must be [H, 2H + 2*vertex_dim + 1]")
    c = _wdelta_cache
    if c[0] is W0 and c[1] == W0._version:
        return c[2], 1
    col = W0.detach()[:, W0.shape[1] - 1].contiguous()
    c[0], c[1], c[2] = W0, W0._version, col
    return col, 1


def edge_pair_fwd(Pa, Pb, cv, W0, meta, eps=LN_EPS, ln=None, keep_pre=True):
    """ln = (gamma, beta, act, drop_p, seed): also return h = drop(act(LayerNorm(pre))) as an sx8 operand.
    keep_pre=False (with ln): the pre-activation is not stored (returned as None); edge_pair_ln_bwd rebuilds it."""
    _need_cuda(Pa, Pb, cv, W0)
    H = Pa.shape[1]
    wd, stride = _wdelta(W0, H)
    dev = Pa.device
    pre = torch.empty(meta.Re, H, dtype=torch.float32, device=dev) if (keep_pre or ln is None) else None
    mu = torch.empty(meta.Re, dtype=torch.float32, device=dev)
    rs = torch.empty(meta.Re, dtype=torch.float32, device=dev)
    delta = torch.empty(meta.Re, dtype=torch.float32, device=dev)
    if ln is None:
        check(_lib.load().wf3d_edge_pair_fwd(_p(Pa), _p(Pb), _p(cv), _p(wd), stride, _p(meta.voff), _p(meta.eoff),
                                             _p(meta.esample), meta.Re, H, cv.shape[1], eps, _p(pre), _p(mu), _p(rs), _p(delta),
                                             _stream()), "edge_pair_fwd")
        return pre, mu, rs, delta
    gamma, beta, act, drop_p, seed = ln
    _need_cuda(gamma, beta)
    h = torch.empty(meta.Re, H, dtype=torch.float32, device=dev)
    check(_lib.load().wf3d_edge_pair_fwd_ln(_p(Pa), _p(Pb), _p(cv), _p(wd), stride, _p(meta.voff), _p(meta.eoff),
                                            _p(meta.esample), meta.Re, H, cv.shape[1], eps, _p(pre), _p(mu), _p(rs), _p(delta),
                                            _p(gamma), _p(beta), act, float(drop_p), int(seed) & 0xFFFFFFFF, _p(h),
                                            _stream()), "edge_pair_fwd_ln")
    return pre, mu, rs, delta, h


def edge_pair_infer(Pa, Pb, cv, W0, meta, e0, n, out, ln=None, eps=LN_EPS):
    """The pair combine of edge rows [e0, e0 + n) of the layout into block buffers indexed by e - e0 (forward-only path;
    include/wf3d.h, "PAIR COMBINE OF A BLOCK"): the rows of edge_pair_fwd bit for bit, without dropout, delta or any store
    that only a backward reads.  e0: a multiple of 8.
    ln = (gamma, beta, act): out = h [n, H], which receives act(LayerNorm(pre)) as an sx8 operand; returns h.
    ln = None: out = (pre [n, H], mu [n], rs [n]); returns them."""
    _need_cuda(Pa, Pb, cv, W0)
    H = Pa.shape[1]
    e0, n = int(e0), int(n)
    if e0 < 0 or n < 0 or e0 + n > meta.Re:
        raise RuntimeError(f"wf3d.edge_pair_infer: rows [{e0}, {e0 + n}) are not inside the layout's {meta.Re} edge rows")
    wd, stride = _wdelta(W0, H)

    def buf(t, what):
        _need_cuda(t)
        if t.dtype != torch.float32 or tuple(t.shape) != (n, H) or not t.is_contiguous():
            raise RuntimeError(f"wf3d.edge_pair_infer: {what} must be a contiguous float32 [{n}, {H}]")
        return t
    if ln is not None:
        gamma, beta, act = ln
        _need_cuda(gamma, beta)
        pre = mu = rs = None
        h = buf(out, "out h")
    else:
        gamma = beta = h = None
        act = ACT_NONE
        pre, mu, rs = out
        buf(pre, "out pre")
        _row_bufs("edge_pair_infer", n, mu, rs)
    check(_lib.load().wf3d_edge_pair_infer(_p(Pa), _p(Pb), _p(cv), _p(wd), stride, _p(meta.voff), _p(meta.eoff),
                                           _p(meta.esample), e0, n, H, cv.shape[1], eps, _p(gamma), _p(beta), act,
                                           _p(pre), _p(mu), _p(rs), _p(h), _stream()), "edge_pair_infer")
    return out


def block_live(total, rows, Re, nblocks):
    """int32 [nblocks]: the live rows of each block of a walk of Re rows in blocks of `rows`, from the live total `total`
    (a one-element int32 device tensor, EdgeMeta.live), which is not read on the host."""
    _need_cuda(total)
    if total.dtype != torch.int32 or total.numel() != 1:
        raise RuntimeError("wf3d.block_live: needs a one-element int32 device tensor")
    rows, Re, nblocks = int(rows), int(Re), int(nblocks)
    if rows <= 0 or Re < 0 or nblocks < 0:
        raise ValueError(f"wf3d.block_live: bad dims rows={rows} Re={Re} nblocks={nblocks}")
    blive = torch.empty(nblocks, dtype=torch.int32, device=total.device)
    check(_lib.load().wf3d_block_live(_p(total), rows, Re, nblocks, _p(blive), _stream()), "block_live")
    return blive


def edge_pair_ln_bwd(dh, Pa, Pb, delta, W0, meta, mu, rs, gamma, beta, act, drop_p=0.0, seed=0):
    """LayerNorm / activation backward of the first edge layer whose pre-activation was not stored: rebuilt from Pa / Pb.
    Returns (dpre (in place of dh), dgamma, dbeta, wsum) like ln_act_bwd_wsum(..., inplace=True)."""
    _need_cuda(dh, Pa, Pb, delta, W0, mu, rs, gamma, beta)
    if not (dh.is_contiguous() and Pa.is_contiguous() and Pb.is_contiguous() and delta.is_contiguous()):
        raise RuntimeError("wf3d.edge_pair_ln_bwd: contiguous tensors required")
    Re, H = dh.shape
    wd, stride = _wdelta(W0, H)
    duo = torch.empty(2, H, dtype=torch.float32, device=dh.device)
    wsum = torch.empty(H, dtype=torch.float32, device=dh.device)
    lib = _lib.load()
    ws = scratch(lib.wf3d_edge_pair_ln_bwd_ws_bytes(Re, H), dh.device)
    check(lib.wf3d_edge_pair_ln_bwd(_p(dh), _p(Pa), _p(Pb), _p(delta), _p(wd), stride, _p(meta.voff), _p(meta.eoff),
                                    _p(meta.esample), Re, H, _p(mu), _p(rs), _p(gamma), _p(beta), act, float(drop_p),
                                    int(seed) & 0xFFFFFFFF, _p(dh), _p(duo[0]), _p(duo[1]), _p(wsum), _p(ws), ws.numel(),
                                    _stream()), "edge_pair_ln_bwd")
    return dh, duo[0], duo[1], wsum


def edge_pair_bwd(dpre, delta, cv, W0, meta, coord=False):
    """coord=True: dcv also receives dPa·Wc + dPb·Wd (the coordinate columns 2H..2H+2d-1 of W0, d = cv.shape[1])."""
    _need_cuda(dpre, delta, cv, W0)
    H = dpre.shape[1]
    d = cv.shape[1]
    wd, stride = _wdelta(W0, H)
    wc = W0[:, 2 * H:2 * H + 2 * d] if coord else None
    if coord and (W0.dim() != 2 or W0.shape[1] < 2 * H + 2 * d or W0.stride(1) != 1):
        raise RuntimeError("wf3d.edge_pair_bwd: W0 must be [H, >= 2H + 2*vertex_dim] with unit inner stride")
    dev = dpre.device
    dPa = torch.empty(meta.Rv, H, dtype=torch.float32, device=dev)
    dPb = torch.empty(meta.Rv, H, dtype=torch.float32, device=dev)
    dcv = torch.empty(meta.Rv, d, dtype=torch.float32, device=dev)
    check(_lib.load().wf3d_edge_pair_bwd(_p(dpre), _p(delta), _p(cv), _p(wd), stride, _p(meta.voff), _p(meta.eoff),
                                         _p(meta.vsample), meta.Rv, H, d, _p(dPa), _p(dPb), _p(dcv), _p(wc),
                                         W0.stride(0) if coord else 0, _stream()),
          "edge_pair_bwd")
    return dPa, dPb, dcv


def edge_prob_fwd(logit, meta):
    _need_cuda(logit)
    probs = torch.empty(meta.B, meta.max_e, dtype=torch.float32, device=logit.device)   # the kernel writes the 0.0 padding too
    check(_lib.load().wf3d_edge_prob_fwd(_p(logit), _p(meta.eoff), meta.B, meta.max_e, _p(probs), _stream()), "edge_prob_fwd")
    return probs


def edge_prob_bwd(probs, dprobs, meta):
    _need_cuda(probs, dprobs)
    if not dprobs.is_contiguous():
        raise RuntimeError("wf3d.edge_prob_bwd: contiguous dprobs required")
    dlogit = torch.empty(meta.Re, 1, dtype=torch.float32, device=probs.device)
    check(_lib.load().wf3d_edge_prob_bwd(_p(probs), _p(dprobs), _p(meta.eoff), _p(meta.esample), meta.Re, meta.max_e,
                                         _p(dlogit), _stream()), "edge_prob_bwd")
    return dlogit


# ---------------------------------------------------------------------------
# bf16x3 split-precision path ("sx8" operands, see include/wf3d.h)
# ---------------------------------------------------------------------------
def split_rows(t, transpose=False):
    """fp32 [R, C] -> sx8 tensor of the same shape (C % 8 == 0); transpose=True gives split(t.T)."""
    _need_cuda(t)
    t = _rows2d(t)
    if transpose:
        R, C, rs, cs = t.shape[1], t.shape[0], 1, t.stride(0)
    else:
        R, C, rs, cs = t.shape[0], t.shape[1], t.stride(0), 1
    out = torch.empty(R, C, dtype=torch.float32, device=t.device)
    check(_lib.load().wf3d_split_rows(_p(t), rs, cs, R, C, _p(out), _stream()), "split_rows")
    return out


def split_weights(weights):
    """[(split(W), split(W^T)) for W in weights] — both sx8 orientations of up to 4 weight matrices per launch
    (the forward GEMM's operand and its dgrad's)."""
    out = []
    for i in range(0, len(weights), 4):
        chunk = weights[i:i + 4]
        n = 2 * len(chunk)
        ins, outs = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)()
        rs, cs = (ctypes.c_long * n)(), (ctypes.c_long * n)()
        Rr, Cc = (ctypes.c_int * n)(), (ctypes.c_int * n)()
        res = []
        for k, W in enumerate(chunk):
            _need_cuda(W)
            W = _rows2d(W)
            N, K = W.shape
            a = torch.empty(N, K, dtype=torch.float32, device=W.device)
            b = torch.empty(K, N, dtype=torch.float32, device=W.device)
            ins[2 * k], outs[2 * k], rs[2 * k], cs[2 * k], Rr[2 * k], Cc[2 * k] = W.data_ptr(), a.data_ptr(), W.stride(0), 1, N, K
            ins[2 * k + 1], outs[2 * k + 1], rs[2 * k + 1], cs[2 * k + 1], Rr[2 * k + 1], Cc[2 * k + 1] = \
                W.data_ptr(), b.data_ptr(), 1, W.stride(0), K, N
            res.append((a, b))
        check(_lib.load().wf3d_split_rows_multi(ins, rs, cs, Rr, Cc, outs, n, _stream()), "split_rows_multi")
        out += res
    return out


def ln_prep(z, gamma, beta, act, eps=LN_EPS, drop_p=0.0, seed=0, out=None):
    """(mu, rs, h_sx8) with h = drop(act(LayerNorm(z))); z contiguous [R, D], D % 8 == 0.  out = (mu, rs, h): buffers
    to write instead of new ones (mu, rs contiguous float32 [R], h contiguous [R, D])."""
    _need_cuda(z, gamma, beta)
    if not z.is_contiguous():
        raise RuntimeError("wf3d.ln_prep: contiguous z required")
    R, D = z.shape
    if out is not None:
        mu, rs, h = out
        _row_bufs("ln_prep", R, mu, rs)
        _need_cuda(h)
        if tuple(h.shape) != (R, D) or not h.is_contiguous() or h.dtype != torch.float32:
            raise RuntimeError(f"wf3d.ln_prep: out h must be a contiguous float32 [{R}, {D}]")
    else:
        mu = torch.empty(R, dtype=torch.float32, device=z.device)
        rs = torch.empty(R, dtype=torch.float32, device=z.device)
        h = torch.empty_like(z)
    check(_lib.load().wf3d_ln_prep(_p(z), R, D, _p(gamma), _p(beta), act, eps, float(drop_p), int(seed) & 0xFFFFFFFF,
                                   _p(mu), _p(rs), _p(h), _stream()), "ln_prep")
    return mu, rs, h


def first_layer_ok(x, W):
    """Shapes the fused first-layer kernels take: in_features <= 8, out_features a multiple of 8 up to 1024."""
    return x.dim() == 2 and x.shape[1] <= 8 and W.shape[0] % 8 == 0 and W.shape[0] <= 1024 and x.stride(1) == 1 and W.stride(1) == 1


def first_layer_fwd(x, W, bias, gamma, beta, act, eps=LN_EPS, drop_p=0.0, seed=0):
    """x [R, K<=8] -> (z = x·W^T + b, mu, rs, h_sx8 = drop(act(LayerNorm(z)))) in one pass.  drop_p = 0 is the call
    without a mask (wf3d_first_layer_fwd), whatever the seed."""
    _need_cuda(x, W, bias, gamma, beta)
    R, K = x.shape
    D = W.shape[0]
    z = torch.empty(R, D, dtype=torch.float32, device=x.device)
    h = torch.empty_like(z)
    mu = torch.empty(R, dtype=torch.float32, device=x.device)
    rs = torch.empty(R, dtype=torch.float32, device=x.device)
    if drop_p:
        check(_lib.load().wf3d_first_layer_fwd_drop(_p(x), R, K, x.stride(0), _p(W), W.stride(0), _p(bias), D, _p(gamma),
                                                    _p(beta), act, eps, float(drop_p), int(seed) & 0xFFFFFFFF, _p(z), _p(mu),
                                                    _p(rs), _p(h), _stream()), "first_layer_fwd_drop")
        return z, mu, rs, h
    check(_lib.load().wf3d_first_layer_fwd(_p(x), R, K, x.stride(0), _p(W), W.stride(0), _p(bias), D, _p(gamma), _p(beta),
                                           act, eps, _p(z), _p(mu), _p(rs), _p(h), _stream()), "first_layer_fwd")
    return z, mu, rs, h


def first_layer_infer(x, W, bias, gamma, beta, act, eps=LN_EPS, out=None):
    """x [R, K<=8] -> h_sx8 = act(LayerNorm(x·W^T + b)) alone: first_layer_fwd's h bit for bit, no z, mu or rs
    (forward-only path).  out: a contiguous float32 [R, D] buffer to write instead of a new one."""
    _need_cuda(x, W, bias, gamma, beta, out)
    R, K = x.shape
    D = W.shape[0]
    if out is None:
        out = torch.empty(R, D, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (R, D) or not out.is_contiguous() or out.dtype != torch.float32:
        raise RuntimeError(f"wf3d.first_layer_infer: out must be a contiguous float32 [{R}, {D}]")
    check(_lib.load().wf3d_first_layer_infer(_p(x), R, K, x.stride(0), _p(W), W.stride(0), _p(bias), D, _p(gamma), _p(beta),
                                             act, eps, _p(out), _stream()), "first_layer_infer")
    return out


def ln_act_bwd_first(dh, z, x, mu, rs, gamma, beta, act, drop_p=0.0, seed=0):
    """Backward of drop(act(LayerNorm(z))) for the first layer: (dgamma, dbeta, dbias, dW[D, K]); dz is not materialised."""
    _need_cuda(dh, z, x, mu, rs, gamma, beta)
    if not (dh.is_contiguous() and z.is_contiguous()):
        raise RuntimeError("wf3d.ln_act_bwd_first: contiguous tensors required")
    R, D = z.shape
    K = x.shape[1]
    trio = torch.empty(3, D, dtype=torch.float32, device=z.device)
    dW = torch.empty(D, K, dtype=torch.float32, device=z.device)
    lib = _lib.load()
    ws = scratch(lib.wf3d_ln_act_bwd_first_ws_bytes(R, D), z.device)
    if drop_p:
        check(lib.wf3d_ln_act_bwd_first_drop(_p(dh), _p(z), _p(x), R, D, K, x.stride(0), _p(mu), _p(rs), _p(gamma), _p(beta),
                                             act, float(drop_p), int(seed) & 0xFFFFFFFF, _p(trio[0]), _p(trio[1]), _p(trio[2]),
                                             _p(dW), _p(ws), ws.numel(), _stream()), "ln_act_bwd_first_drop")
        return trio[0], trio[1], trio[2], dW
    check(lib.wf3d_ln_act_bwd_first(_p(dh), _p(z), _p(x), R, D, K, x.stride(0), _p(mu), _p(rs), _p(gamma), _p(beta), act,
                                    _p(trio[0]), _p(trio[1]), _p(trio[2]), _p(dW), _p(ws), ws.numel(), _stream()),
          "ln_act_bwd_first")
    return trio[0], trio[1], trio[2], dW


def _products(products):
    if products not in (1, 3):
        raise ValueError(f"wf3d: products must be 1 (bf16) or 3 (bf16x3), got {products!r}")
    return products


def gemm_split(a_s, b_s, bias=None, out=None, accumulate=False, products=3):
    """C[M,N] = A·B^T (+bias) with A = sx8[M,K], B = sx8[N,K] (products=3, bf16x3: hi*hi + hi*lo + lo*hi; products=1,
    bf16: hi*hi only, wf3d_gemm_bf16; fp32 accumulate)."""
    _products(products)
    _need_cuda(a_s, b_s, bias, out)
    a_s, b_s = _rows2d(a_s), _rows2d(b_s)
    M, K = a_s.shape
    N, K2 = b_s.shape
    if K != K2:
        raise RuntimeError("wf3d.gemm_split: reduction dims differ")
    if out is None:
        if accumulate:
            raise RuntimeError("wf3d.gemm_split: accumulate needs `out`")
        out = torch.empty(M, N, dtype=torch.float32, device=a_s.device)
    lib = _lib.load()
    ws = scratch(lib.wf3d_gemm_split_ws_bytes(M, N, K), a_s.device)
    fn = lib.wf3d_gemm_split if products == 3 else lib.wf3d_gemm_bf16
    check(fn(_p(a_s), _p(b_s), _p(out), _p(bias), M, N, K, a_s.stride(0), b_s.stride(0),
             out.stride(0), 1 if accumulate else 0, _p(ws), ws.numel() if ws is not None else 0,
             _stream()), "gemm_split" if products == 3 else "gemm_bf16")
    return out


def split_transpose(t, pro=None, in_sx8=False):
    """sx8 [C, R] = split(pro(t)^T) for fp32 t [R, C] (R % 8 == 0); pro = Pro(act, mu, rs, gamma, beta) or None.
    in_sx8=True: t is itself an sx8 matrix and is transposed plane-wise (no prologue)."""
    _need_cuda(t)
    t = _rows2d(t)
    R, C = t.shape
    out = torch.empty(C, R, dtype=torch.float32, device=t.device)
    mu = rs = gamma = beta = None
    act, drop_p, seed = ACT_NONE, 0.0, 0
    if pro is not None:
        mu, rs, gamma, beta, act, drop_p, seed = pro.mu, pro.rs, pro.gamma, pro.beta, pro.act, pro.drop_p, pro.seed
    check(_lib.load().wf3d_split_transpose(_p(t), R, C, t.stride(0), _p(mu), _p(rs), _p(gamma), _p(beta), act,
                                           float(drop_p), int(seed) & 0xFFFFFFFF, 1 if in_sx8 else 0, _p(out),
                                           _stream()), "split_transpose")
    return out


def gemm_split_tn_ok(a_s, b_s):
    return bool(_lib.load().wf3d_gemm_split_tn_ok(a_s.shape[1], b_s.shape[1], a_s.shape[0], a_s.stride(0), b_s.stride(0)))


def gemm_split_tn_shape_ok(K, Mo, No, lda, ldb):
    """Same test from shapes alone (before the operand exists)."""
    return bool(_lib.load().wf3d_gemm_split_tn_ok(Mo, No, K, lda, ldb))


def gemm_split_tn(a_s, b_s, out=None, accumulate=False, products=3):
    """C[Mo,No] = A^T·B with A = sx8[K,Mo], B = sx8[K,No] (wgrad on operands as stored); products as in gemm_split."""
    _products(products)
    _need_cuda(a_s, b_s, out)
    a_s, b_s = _rows2d(a_s), _rows2d(b_s)
    K, Mo = a_s.shape
    K2, No = b_s.shape
    if K != K2:
        raise RuntimeError("wf3d.gemm_split_tn: reduction dims differ")
    if out is None:
        if accumulate:
            raise RuntimeError("wf3d.gemm_split_tn: accumulate needs `out`")
        out = torch.empty(Mo, No, dtype=torch.float32, device=a_s.device)
    lib = _lib.load()
    ws = scratch(lib.wf3d_gemm_split_tn_ws_bytes(Mo, No, K), a_s.device)
    fn = lib.wf3d_gemm_split_tn if products == 3 else lib.wf3d_gemm_bf16_tn
    check(fn(_p(a_s), _p(b_s), _p(out), Mo, No, K, a_s.stride(0), b_s.stride(0), out.stride(0),
             1 if accumulate else 0, _p(ws), ws.numel() if ws is not None else 0, _stream()),
          "gemm_split_tn" if products == 3 else "gemm_bf16_tn")
    return out


# ---------------------------------------------------------------------------
# row f-1: WireframeLoss on device
# ---------------------------------------------------------------------------
def loss_cost_matrix(verts, exist, tverts, counts):
    """verts [B,V,3] (view ok), exist [B,V], tverts [B,Vt,3], counts int64 [B] -> cost [B,V,V]."""
    _need_cuda(verts, exist, tverts, counts)
    if verts.stride(2) != 1 or not exist.is_contiguous() or not tverts.is_contiguous() or counts.dtype != torch.int64:
        raise RuntimeError("wf3d.loss_cost_matrix: bad layout / dtype")
    B, V, _ = verts.shape
    cost = torch.empty(B, V, V, dtype=torch.float32, device=verts.device)
    check(_lib.load().wf3d_loss_cost_matrix(_p(verts), verts.stride(0), verts.stride(1), _p(exist), _p(tverts),
                                            tverts.shape[1], _p(counts), B, V, _p(cost), _stream()), "loss_cost_matrix")
    return cost


def _loss_launch(name, verts, exist, edge, tverts, texist, tlabel, match, weights, balance=()):
    """One launch of wf3d_<name>, a wf3d_loss_terms* entry point: they differ only in `match`, the arguments between Et
    and B that say which prediction is matched to which target, and in `balance`, the (pos_weight, focal_gamma) that the
    _bal entry takes after the weights.  Allocates and returns (losses, dverts, dexist, dedge)."""
    B, V, _ = verts.shape
    Ep = edge.shape[1] if edge is not None else 0
    Et = tlabel.shape[1] if tlabel is not None else 0
    dev = verts.device
    dverts = torch.empty(B, V, 3, dtype=torch.float32, device=dev)
    dexist = torch.empty(B, V, dtype=torch.float32, device=dev)
    dedge = torch.empty(B, Ep, dtype=torch.float32, device=dev)
    losses = torch.empty(4, dtype=torch.float32, device=dev)
    ws = scratch(B * 3 * 4, dev)
    check(getattr(_lib.load(), "wf3d_" + name)(
        _p(verts), verts.stride(0), verts.stride(1), _p(exist), _p(edge), Ep, _p(tverts), tverts.shape[1], _p(texist),
        _p(tlabel), Et, *match, B, V, float(weights[0]), float(weights[1]), float(weights[2]), *balance, _p(dverts),
        _p(dexist), _p(dedge), _p(losses), _p(ws), ws.numel(), _stream()), name)
    return losses, dverts, dexist, dedge


def loss_terms(verts, exist, edge, tverts, texist, tlabel, m_pred, m_tgt, m_off, n_match, weights):
    """Returns (losses[4] = vertex, existence, edge, total; dverts [B,V,3]; dexist [B,V]; dedge [B,Ep])."""
    _need_cuda(verts, exist, edge, tverts, texist, tlabel, m_pred, m_tgt, m_off)
    return _loss_launch("loss_terms", verts, exist, edge, tverts, texist, tlabel,
                        (_p(m_pred), _p(m_tgt), _p(m_off), int(n_match)), weights)


def loss_assign(cost, counts=None):
    """cost [B,V,V] -> col4row int32 [B,V]: optimal assignment per sample, computed on the device.  With `counts`
    (int64 [B]; columns >= counts[b] are the wireframe cost's identical dummy columns) only the real targets are
    augmented: same matches to real targets, unmatched predictions on the dummy columns in order."""
    _need_cuda(cost, counts)
    B, V, _ = cost.shape
    out = torch.empty(B, V, dtype=torch.int32, device=cost.device)
    if counts is None:
        check(_lib.load().wf3d_loss_assign(_p(cost), B, V, _p(out), _stream()), "loss_assign")
    else:
        check(_lib.load().wf3d_loss_assign_counts(_p(cost), _p(counts), B, V, _p(out), _stream()), "loss_assign_counts")
    return out


def loss_terms_assigned(verts, exist, edge, tverts, texist, tlabel, col4row, counts, weights, edge_width=None):
    """edge_width: int64 0-d device tensor, the prediction's edge width (a padded edge head's), read by the kernel
    instead of edge.shape[1]."""
    _need_cuda(verts, exist, edge, tverts, texist, tlabel, col4row, counts, edge_width)
    if edge_width is None:
        return _loss_launch("loss_terms_assigned", verts, exist, edge, tverts, texist, tlabel,
                            (_p(col4row), _p(counts)), weights)
    if edge_width.dtype != torch.int64 or edge_width.numel() != 1:
        raise RuntimeError("wf3d.loss_terms_assigned: edge_width must be a one-element int64 tensor")
    return _loss_launch("loss_terms_assigned_ew", verts, exist, edge, tverts, texist, tlabel,
                        (_p(edge_width), _p(col4row), _p(counts)), weights)


def loss_terms_assigned_bal(verts, exist, edge, tverts, texist, tlabel, col4row, counts, weights, edge_pos_weight,
                            edge_focal_gamma, edge_width=None):
    """loss_terms_assigned with the class-balanced / focal edge element (include/wf3d.h, wf3d_loss_terms_assigned_bal):
    positives weighted by edge_pos_weight > 0, each side modulated by (1 - its probability)^edge_focal_gamma, gamma >= 0.
    edge_width as in loss_terms_assigned, or None."""
    _need_cuda(verts, exist, edge, tverts, texist, tlabel, col4row, counts, edge_width)
    if edge_width is not None and (edge_width.dtype != torch.int64 or edge_width.numel() != 1):
        raise RuntimeError("wf3d.loss_terms_assigned_bal: edge_width must be a one-element int64 tensor")
    return _loss_launch("loss_terms_assigned_bal", verts, exist, edge, tverts, texist, tlabel,
                        (_p(edge_width), _p(col4row), _p(counts)), weights,
                        balance=(float(edge_pos_weight), float(edge_focal_gamma)))


def edge_labels_matched(edge_labels, assignment, counts, width, pair_counts=None):
    """The edge labels under an assignment, on the device (wf3d.targets.matched_edge_labels is the specification; the
    result equals it element for element).  edge_labels fp32 [B, Et], assignment int32 [B, V], counts int64 [B] (target
    counts), pair_counts int64 [B] or None (the counts whose pair order the prediction row has) -> fp32 [B, width].
    One launch, nothing read on the host."""
    _need_cuda(edge_labels, assignment, counts, pair_counts)
    if (edge_labels.dtype != torch.float32 or edge_labels.dim() != 2 or assignment.dtype != torch.int32 or assignment.dim() != 2
            or counts.dtype != torch.int64 or (pair_counts is not None and pair_counts.dtype != torch.int64)
            or not (edge_labels.is_contiguous() and assignment.is_contiguous() and counts.is_contiguous())
            or (pair_counts is not None and not pair_counts.is_contiguous())):
        raise RuntimeError("wf3d.edge_labels_matched: bad layout / dtype")
    B, V = assignment.shape
    if edge_labels.shape[0] != B or counts.numel() != B or (pair_counts is not None and pair_counts.numel() != B):
        raise RuntimeError("wf3d.edge_labels_matched: batch sizes differ")
    out = torch.empty(B, int(width), dtype=torch.float32, device=assignment.device)
    check(_lib.load().wf3d_edge_labels_matched(_p(edge_labels), edge_labels.shape[1], _p(assignment), _p(counts),
                                               _p(pair_counts), B, V, int(width), _p(out), _stream()), "edge_labels_matched")
    return out
