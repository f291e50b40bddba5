"""Every kernel form, pitch and tile edge of csrc/skinny.hip (Linear layers over M <= 32 rows) against fp64 torch math
on the CPU, through the C ABI structs (SkinnyFwd / SkinnyBwd / SkinnyRed) so that each pitch, `nc` and pointer is the
test's own: wf3d/skinny.py always passes contiguous, 16-byte aligned operands, nc = 64 and ReLU.

Bounds are the ones of tests/test_skinny_gpu.py: forward outputs and statistics rel_err < 1e-5 of the tensor scale,
every gradient elem_err < 1e-4 of max(|g|, rms(g)).  Wherever an fp64 reference goes through a ReLU or a GELU, its
LayerNorm output has no element within 1e-6 of 0 (asserted on the CPU values before anything runs), except in
test_one_relu_decision_at_three_sites, where borderline elements are the subject.

Buffers the kernels write are views into NaN-filled allocations: whatever lies outside the window, or in the 64-float
bands before and after it, must still be NaN afterwards."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402

NONE, RELU, GELU = 0, 1, 2
EPS = 1e-5
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
NAN = float("nan")
GUARD = 64            # floats of NaN before and after every buffer a kernel writes (keeps 16-byte alignment)

_PITCH = {"X": "ldx", "W": "ldw", "Y": "ldy", "in_addend": "ld_in_addend", "out_addend": "ld_out_addend", "dY": "lddy",
          "z": "ldz", "xadd": "ldxadd", "dW": "lddw", "extra": "ldextra", "dh": "lddh", "G": "ldg"}
_COUNT = {"in_part": "in_nblk", "rowpart": "rowpart_nblk"}


def dev():
    return torch.device("cuda:0")


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------
# calling the C ABI: a problem is a dict of struct fields; tensors become addresses, and a 2-D tensor also sets its
# pitch field from its row stride unless the dict names that pitch itself
# ------------------------------------------------------------------------------------------------------------------
def _fill(d, kw, counts=True):
    for k, v in kw.items():
        if v is None:
            continue
        if torch.is_tensor(v):
            assert v.is_cuda and v.dtype == torch.float32 and v.stride(-1) == 1, k
            setattr(d, k, v.data_ptr())
            if k in _PITCH and _PITCH[k] not in kw:
                setattr(d, _PITCH[k], v.stride(0) if v.dim() == 2 else v.shape[-1])
            if counts and k in _COUNT and _COUNT[k] not in kw:
                setattr(d, _COUNT[k], v.shape[0])
            if k == "W" and "N" not in kw:
                d.N, d.K = v.shape
        else:
            setattr(d, k, v)


def _api():
    from wf3d import _lib
    from wf3d.ops import _stream
    return _lib, _lib.load(), _stream()


def fwd(M, *probs, eps=EPS):
    lib, L, st = _api()
    arr = (lib.SkinnyFwd * max(1, len(probs)))()
    for d, kw in zip(arr, probs):
        _fill(d, kw)
    return L.wf3d_skinny_fwd(arr, len(probs), M, eps, st)


def bwd(M, *probs):
    lib, L, st = _api()
    arr = (lib.SkinnyBwd * max(1, len(probs)))()
    for d, kw in zip(arr, probs):
        _fill(d, kw)
    return L.wf3d_skinny_bwd(arr, len(probs), M, st)


def red(M, sets=(), **kw):
    lib, L, st = _api()
    d = lib.SkinnyRed()
    for i, s in enumerate(sets):
        d.slabs[i], d.nslab[i] = s.data_ptr(), s.shape[0]
    _fill(d, kw, counts=False)
    return L.wf3d_skinny_reduce(ctypes.byref(d), M, st)


def ok(rc):
    assert rc == OK, (rc, _api()[1].wf3d_last_error().decode(errors="replace"))


def refused(rc, code, text):
    msg = _api()[1].wf3d_last_error().decode(errors="replace")
    assert rc == code and text in msg, (rc, msg)


class Win:
    """A [*shape] window (row pitch `ld`, `off` floats past a 16-byte boundary) inside a NaN-filled buffer with GUARD floats before
    and after it.  `.t` is the tensor to hand to a kernel."""

    def __init__(self, shape, ld=None, off=0, src=None):
        shape = tuple(shape)
        n = shape[-1]
        rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
        ld = ld or n
        assert ld == n or len(shape) == 2
        self.buf = torch.full((GUARD + off + rows * ld + GUARD,), NAN, dtype=torch.float32, device=dev())
        self.geom = ((rows, n), (ld, 1), GUARD + off)
        v = torch.as_strided(self.buf, *self.geom)
        if src is not None:
            v.copy_(src.reshape(rows, n))
        self.t = v if len(shape) == 2 else v.view(shape)

    def untouched_outside(self):
        c = self.buf.clone()
        torch.as_strided(c, *self.geom).fill_(NAN)
        return bool(c.isnan().all())


def out(*shape, ld=None, off=0):
    return Win(shape, ld, off)


def place(t, ld=None, off=0):
    """A copy of the 2-D tensor `t` with row pitch `ld`, starting `off` floats past a 16-byte boundary; NaN around it."""
    return Win(t.shape, ld, off, src=t.to(dev())).t


def g(t):
    return None if t is None else t.to(dev())


def c64(t):
    return t.detach().double().cpu().numpy()


def randn(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


def ln64(x, gam, bet, mu=None, rs=None):
    if mu is None:
        mu = x.mean(1)
        rs = 1 / torch.sqrt(((x - mu[:, None]) ** 2).mean(1) + EPS)
    return (x - mu[:, None]) * rs[:, None] * gam + bet


def act64(act, v):
    return torch.relu(v) if act == RELU else torch.nn.functional.gelu(v) if act == GELU else v


def no_borderline(v, act=RELU):
    """The fp64 LayerNorm output decides alone whether an input may be compared through an activation."""
    assert act == NONE or int((v.detach().abs() < 1e-6).sum()) == 0, "LayerNorm output within 1e-6 of 0: pick another seed"


def stats64(x):
    mu = x.mean(1)
    return mu, 1 / torch.sqrt(((x - mu[:, None]) ** 2).mean(1) + EPS)


def part64(y):
    """[N/16][M][2]: mean and M2 (sum of squared deviations from that mean) of every 16-column block."""
    M, N = y.shape
    b = y.reshape(M, N // 16, 16)
    mean = b.mean(-1)
    return torch.stack([mean, ((b - mean[..., None]) ** 2).sum(-1)], -1).permute(1, 0, 2)


def extras(gen, M, K, N, on):
    """(bias, in_addend, out_addend), or three None's."""
    return (randn(gen, N), randn(gen, M, K), randn(gen, M, N)) if on else (None, None, None)


def add(a, b):
    return a if b is None else a + b.double()


# ------------------------------------------------------------------------------------------------------------------
# 1. forward forms
# ------------------------------------------------------------------------------------------------------------------
MID = (200, 80)
PLAIN = [(M, *MID) for M in (1, 9, 15, 16, 17, 31, 32)] + \
        [(M, K, N) for M in (2, 17) for K, N in ((4, 1), (36, 17), (512, 64), (516, 65), (528, 48))]


def plain_case(M, K, N, ex):
    gen = torch.Generator().manual_seed(11 * M + K + 1000 * ex)
    X, W = randn(gen, M, K), randn(gen, N, K, scale=K ** -0.5)
    b, A, R = extras(gen, M, K, N, ex)
    want = add(add(add(X.double(), A) @ W.double().t(), b), R)
    return X, W, b, A, R, want


@pytest.mark.parametrize("ex", [0, 1], ids=["bare", "bias+addends"])
@pytest.mark.parametrize("M,K,N", PLAIN)
def test_forward_plain(M, K, N, ex):
    """Y = (X + A)·W^T + b + R, and Y's (mean, M2) partials where N % 16 == 0."""
    X, W, b, A, R, want = plain_case(M, K, N, ex)
    Y = out(M, N)
    part = out(N // 16, M, 2) if N % 16 == 0 else None
    ok(fwd(M, dict(X=g(X), W=g(W), Y=Y.t, bias=g(b), in_addend=g(A), out_addend=g(R), stat_part=part and part.t)))
    assert H.rel_err(c64(Y.t), want.numpy()) < 1e-5
    assert Y.untouched_outside()
    if part:
        assert H.rel_err(c64(part.t), part64(want).numpy()) < 1e-5
        assert part.untouched_outside()


LN_PART = [(16, 24), (528, 65), (4112, 32)]      # in_nblk = 1, 33; K > 4096: affine vectors read from global memory
LN_GIVEN = [(36, 17), (4100, 32)]
K0 = 20


def ln_case(M, K, N, act, ex, given):
    """(mu, rs)-given: X is an input.  From partials: X = X0·W0^T + b0 is the producer launch's output."""
    gen = torch.Generator().manual_seed(7 * M + K + 100 * act + 1000 * ex)
    if given:
        X0 = W0 = b0 = None
        X = randn(gen, M, K, scale=1.5) + 0.3
        x64 = X.double()
    else:
        X0, W0, b0 = randn(gen, M, K0), randn(gen, K, K0, scale=K0 ** -0.5), randn(gen, K)
        X = None
        x64 = X0.double() @ W0.double().t() + b0.double()
    gam, bet = 1 + 0.1 * randn(gen, K), 0.1 * randn(gen, K)
    W = randn(gen, N, K, scale=K ** -0.5)
    b, A, R = extras(gen, M, K, N, ex)
    mu, rs = stats64(x64)
    v = ln64(x64, gam.double(), bet.double())
    no_borderline(v, act)
    want = add(add(add(act64(act, v), A) @ W.double().t(), b), R)
    return dict(X0=X0, W0=W0, b0=b0, X=X, x64=x64, gam=gam, bet=bet, W=W, b=b, A=A, R=R, mu=mu, rs=rs, want=want)


@pytest.mark.parametrize("ex", [0, 1], ids=["bare", "bias+addends"])
@pytest.mark.parametrize("act", [RELU, GELU, NONE], ids=["relu", "gelu", "none"])
@pytest.mark.parametrize("K,N", LN_PART)
@pytest.mark.parametrize("M", [2, 17])
def test_forward_layernorm_from_partials(M, K, N, act, ex):
    """The producer launch leaves per-16-column (mean, M2) partials of X; the consumer merges them on load."""
    c = ln_case(M, K, N, act, ex, given=False)
    X, part = out(M, K), out(K // 16, M, 2)
    ok(fwd(M, dict(X=g(c["X0"]), W=g(c["W0"]), bias=g(c["b0"]), Y=X.t, stat_part=part.t)))
    Y, mu, rs = out(M, N), out(M), out(M)
    ok(fwd(M, dict(X=X.t, W=g(c["W"]), Y=Y.t, bias=g(c["b"]), gamma=g(c["gam"]), beta=g(c["bet"]), act=act, in_part=part.t,
                   mu_out=mu.t, rs_out=rs.t, in_addend=g(c["A"]), out_addend=g(c["R"]))))
    assert H.rel_err(c64(X.t), c["x64"].numpy()) < 1e-5
    assert H.rel_err(c64(part.t), part64(c["x64"]).numpy()) < 1e-5
    assert H.rel_err(c64(mu.t), c["mu"].numpy()) < 1e-5
    assert H.rel_err(c64(rs.t), c["rs"].numpy()) < 1e-5
    assert H.rel_err(c64(Y.t), c["want"].numpy()) < 1e-5
    assert all(w.untouched_outside() for w in (X, part, Y, mu, rs))


@pytest.mark.parametrize("ex", [0, 1], ids=["bare", "bias+addends"])
@pytest.mark.parametrize("act", [RELU, GELU, NONE], ids=["relu", "gelu", "none"])
@pytest.mark.parametrize("K,N", LN_GIVEN)
@pytest.mark.parametrize("M", [2, 17])
def test_forward_layernorm_from_given_statistics(M, K, N, act, ex):
    c = ln_case(M, K, N, act, ex, given=True)
    Y = out(M, N)
    ok(fwd(M, dict(X=g(c["X"]), W=g(c["W"]), Y=Y.t, bias=g(c["b"]), gamma=g(c["gam"]), beta=g(c["bet"]), act=act,
                   mu=g(c["mu"].float()), rs=g(c["rs"].float()), in_addend=g(c["A"]), out_addend=g(c["R"]))))
    assert H.rel_err(c64(Y.t), c["want"].numpy()) < 1e-5
    assert Y.untouched_outside()


# ------------------------------------------------------------------------------------------------------------------
# 2. pitched operands and canaries
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [5, 32])
def test_forward_pitches_change_no_bit_and_write_only_the_window(M):
    K, N = 528, 80
    c = ln_case(M, K, N, RELU, 1, given=True)
    mu, rs = g(c["mu"].float()), g(c["rs"].float())
    common = dict(W=g(c["W"]), bias=g(c["b"]), gamma=g(c["gam"]), beta=g(c["bet"]), act=RELU, mu=mu, rs=rs)
    Y0, P0 = out(M, N), out(N // 16, M, 2)
    ok(fwd(M, dict(common, X=g(c["X"]), Y=Y0.t, in_addend=g(c["A"]), out_addend=g(c["R"]), stat_part=P0.t)))
    assert H.rel_err(c64(Y0.t), c["want"].numpy()) < 1e-5
    Y1, P1 = out(M, N, ld=N + 3), out(N // 16, M, 2)
    ok(fwd(M, dict(common, X=place(c["X"], ld=K + 4), Y=Y1.t, in_addend=place(c["A"], ld=K + 8),
                   out_addend=place(c["R"], ld=N + 1), stat_part=P1.t)))
    assert Y1.t.stride(0) == N + 3
    assert torch.equal(Y1.t, Y0.t) and torch.equal(P1.t, P0.t)
    assert all(w.untouched_outside() for w in (Y0, P0, Y1, P1))


def reduce_case(M, K, layout, seed=0):
    gen = torch.Generator().manual_seed(5 * M + K + 31 * sum(layout) + seed)
    sets = [randn(gen, n, M, K) for n in layout]
    extra = randn(gen, M, K) if len(layout) in (0, 2) else None
    z = randn(gen, M, K, scale=1.5) + 0.3
    gam, bet = 1 + 0.1 * randn(gen, K), 0.1 * randn(gen, K)
    mu, rs = (t.float() for t in stats64(z.double()))
    v = add(sum((s.double().sum(0) for s in sets), torch.zeros(M, K, dtype=torch.float64)), extra)
    xh = (z.double() - mu.double()[:, None]) * rs.double()[:, None]
    y = xh * gam.double() + bet.double()
    no_borderline(y)
    return dict(sets=sets, extra=extra, z=z, gam=gam, bet=bet, mu=mu, rs=rs, v=v, xh=xh, y=y)


def reduce_ref(c, act):
    y = c["y"].clone().requires_grad_()
    act64(act, y).backward(c["v"])
    d = y.grad
    G = d * c["gam"].double()
    M, K = G.shape
    nb = cdiv(K, 64)
    pad = torch.zeros(M, nb * 64 - K, dtype=torch.float64)
    blk = lambda t: torch.cat([t, pad], 1).reshape(M, nb, 64).sum(-1).t()      # noqa: E731
    return G, (d * c["xh"]).sum(0), d.sum(0), torch.stack([blk(G), blk(G * c["xh"])], -1)


def test_backward_and_reduce_pitches_change_no_bit_and_write_only_the_window():
    M, N, K, nc = 17, 130, 260, 64
    gen = torch.Generator().manual_seed(2)
    dY, W, X = g(randn(gen, M, N)), g(randn(gen, N, K, scale=K ** -0.5)), g(randn(gen, M, K))
    ns = cdiv(N, nc)
    dW0, db0, sl0 = out(N, K), out(N), out(ns, M, K)
    ok(bwd(M, dict(dY=dY, W=W, X=X, dW=dW0.t, db=db0.t, slabs=sl0.t, nc=nc)))
    dW1, db1, sl1 = out(N, K, ld=K + 5), out(N), out(ns, M, K)
    ok(bwd(M, dict(dY=dY, W=W, X=X, dW=dW1.t, db=db1.t, slabs=sl1.t, nc=nc)))
    assert H.elem_err(c64(dW0.t), c64(dY).T @ c64(X)) < 1e-4
    assert H.elem_err(c64(db0.t), c64(dY).sum(0)) < 1e-4
    assert torch.equal(dW1.t, dW0.t) and torch.equal(db1.t, db0.t) and torch.equal(sl1.t, sl0.t)
    assert all(w.untouched_outside() for w in (dW0, db0, sl0, dW1, db1, sl1))

    c = reduce_case(M, K, (ns,))
    ln = dict(z=g(c["z"]), mu=g(c["mu"]), rs=g(c["rs"]), gamma=g(c["gam"]), beta=g(c["bet"]), act=RELU)
    res, extra = [], randn(gen, M, K)
    for ld in (K, K + 3):
        w = dict(dh=out(M, K, ld=ld), G=out(M, K, ld=ld + 1), dgamma=out(K), dbeta=out(K), rowpart=out(cdiv(K, 64), M, 2))
        ok(red(M, [sl0.t], K=K, extra=place(extra, ld=ld + 2), **ln, **{k: v.t for k, v in w.items()}))
        assert all(v.untouched_outside() for v in w.values())
        res.append(w)
    for k in res[0]:
        assert torch.equal(res[0][k].t, res[1][k].t), k
    assert H.rel_err(c64(res[1]["dh"].t), c64(sl0.t).sum(0) + c64(extra)) < 1e-5


# ------------------------------------------------------------------------------------------------------------------
# 3. backward forms against fp64 autograd
# ------------------------------------------------------------------------------------------------------------------
#         K    N1   N2      N2: Linear whose output is not LayerNorm'd (any width); N1: LayerNorm'd (statistics: % 16)
CHAIN = [(4, 16, 6), (256, 32, 17), (260, 64, 63), (512, 256, 65), (516, 512, 129), (20, 48, 64), (36, 80, 128)]
FORMS = {
    "plain": {},
    "dy_pitch": dict(dy_ld=1),            # lddy = N + 1: scalar dz loads although N % 4 == 0 (plain and LayerNorm form)
    "dy_offset": dict(dy_off=1),          # dY one float past a 16-byte boundary, lddy % 4 == 0
    "z_pitch": dict(z_ld=1),              # ldz = N + 1
    "x_offset": dict(x_off=1),            # scalar staging of the weight-gradient tile
    "x_pitch": dict(x_ld=1),
    "xadd_offset": dict(xadd_off=1),
    "xadd_pitch": dict(xadd_ld=1),
    "no_dw": dict(dw=False),
    "no_dx": dict(dx=False),
    "gelu": dict(act=GELU),
    "none": dict(act=NONE),
}


def up4(n):
    return (n + 3) // 4 * 4


def pick_nc(N):
    return 64 if N >= 64 else max(2, N + (N & 1))


_chain_cache = {}


def chain_case(M, K, N1, N2, act):
    """z1 = X·W1^T + b1 ; r = X·Wr^T + br ; h = act(LN(z1)) + r ; y = h·W2^T + b2 ; loss = sum(y * C): inputs and the
    fp64 autograd gradients, computed once per (shape, activation)."""
    key = (M, K, N1, N2, act)
    if key not in _chain_cache:
        # + 10000: the first draw of this shape has a LayerNorm output within 1e-6 of 0
        gen = torch.Generator().manual_seed(M * 77 + K + N2 + (10000 if (M, K) == (32, 512) else 0))
        T = dict(X=randn(gen, M, K), W1=randn(gen, N1, K, scale=K ** -0.5), b1=randn(gen, N1),
                 Wr=randn(gen, N1, K, scale=K ** -0.5), br=randn(gen, N1), g=1 + 0.1 * randn(gen, N1), be=0.1 * randn(gen, N1),
                 W2=randn(gen, N2, N1, scale=N1 ** -0.5), b2=randn(gen, N2))
        C = randn(gen, M, N2)
        P = {k: v.double().requires_grad_() for k, v in T.items()}
        v = ln64(P["X"] @ P["W1"].t() + P["b1"], P["g"], P["be"])
        no_borderline(v, act)
        y = (act64(act, v) + P["X"] @ P["Wr"].t() + P["br"]) @ P["W2"].t() + P["b2"]
        (y * C.double()).sum().backward()
        _chain_cache[key] = (T, C, y.detach(), {k: p.grad for k, p in P.items()})
    return _chain_cache[key]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("K,N1,N2", CHAIN)
@pytest.mark.parametrize("M", [3, 16, 17, 32])
def test_backward_forms(M, K, N1, N2, form):
    f = dict(dy_ld=0, dy_off=0, z_ld=0, x_off=0, x_ld=0, xadd_off=0, xadd_ld=0, dw=True, dx=True, act=RELU)
    f.update(FORMS[form])
    act = f["act"]
    T, C, y64, grads = chain_case(M, K, N1, N2, act)
    D = {k: g(v) for k, v in T.items()}
    # forward
    z1, part, r = out(M, N1), out(N1 // 16, M, 2), out(M, N1)
    ok(fwd(M, dict(X=D["X"], W=D["W1"], bias=D["b1"], Y=z1.t, stat_part=part.t), dict(X=D["X"], W=D["Wr"], bias=D["br"], Y=r.t)))
    y, mu, rs = out(M, N2), out(M), out(M)
    ok(fwd(M, dict(X=z1.t, W=D["W2"], bias=D["b2"], Y=y.t, gamma=D["g"], beta=D["be"], act=act, in_part=part.t,
                   mu_out=mu.t, rs_out=rs.t, in_addend=r.t)))
    assert H.rel_err(c64(y.t), y64.numpy()) < 1e-5
    # backward of the second Linear: dY = C, X = z1 behind the LayerNorm prologue, plus r
    zp = place(z1.t, ld=N1 + f["z_ld"])
    wg = lambda **kw: kw if f["dw"] else {}                                    # noqa: E731
    nc2 = pick_nc(N2)
    dW2, db2, sl2 = out(N2, N1), out(N2), out(cdiv(N2, nc2), M, N1)
    ok(bwd(M, dict(dY=place(C, ld=(up4(N2) if f["dy_off"] else N2) + f["dy_ld"], off=f["dy_off"]), W=D["W2"], slabs=sl2.t, nc=nc2,
                   **wg(X=place(z1.t, ld=N1 + f["x_ld"], off=f["x_off"]), xmu=mu.t, xrs=rs.t, xgamma=D["g"], xbeta=D["be"], xact=act,
                        xadd=place(r.t, ld=N1 + f["xadd_ld"], off=f["xadd_off"]), dW=dW2.t, db=db2.t))))
    dh, G = out(M, N1, ld=N1 + f["dy_ld"], off=f["dy_off"]), out(M, N1, ld=N1 + f["dy_ld"], off=f["dy_off"])
    dg, dbe, rowpart = out(N1), out(N1), out(cdiv(N1, 64), M, 2)
    ok(red(M, [sl2.t], K=N1, dh=dh.t, z=zp, mu=mu.t, rs=rs.t, gamma=D["g"], beta=D["be"], act=act, G=G.t, dgamma=dg.t,
           dbeta=dbe.t, rowpart=rowpart.t))
    # backward of the two Linears that read X, one launch: LayerNorm form (dY = G) and plain form (dY = dh)
    Xp = place(T["X"], ld=K + f["x_ld"], off=f["x_off"])
    nc1 = pick_nc(N1)
    ns1 = cdiv(N1, nc1)
    dW1, db1, dWr, dbr, sl1, slr, dX = out(N1, K), out(N1), out(N1, K), out(N1), out(ns1, M, K), out(ns1, M, K), out(M, K)
    dx = lambda s: dict(slabs=s.t, nc=nc1) if f["dx"] else {}                  # noqa: E731
    ok(bwd(M, dict(dY=G.t, z=zp, mu=mu.t, rs=rs.t, rowpart=rowpart.t, W=D["W1"], **wg(X=Xp, dW=dW1.t, db=db1.t), **dx(sl1)),
              dict(dY=dh.t, W=D["Wr"], **wg(X=Xp, dW=dWr.t, db=dbr.t), **dx(slr))))
    got = dict(g=dg, be=dbe)
    if f["dw"]:
        got.update(W1=dW1, b1=db1, Wr=dWr, br=dbr, W2=dW2, b2=db2)
    if f["dx"]:
        ok(red(M, [sl1.t, slr.t], K=K, dh=dX.t))
        got.update(X=dX)
    for k, w in got.items():
        e = H.elem_err(c64(w.t), grads[k].numpy())
        assert e < 1e-4, (k, e)
    every = (z1, part, r, y, mu, rs, dW2, db2, sl2, dh, G, dg, dbe, rowpart, dW1, db1, dWr, dbr, sl1, slr, dX)
    assert all(w.untouched_outside() for w in every)
    written = set(map(id, got.values())) | set(map(id, (z1, part, r, y, mu, rs, sl2, dh, G, rowpart))) | \
        (set(map(id, (sl1, slr))) if f["dx"] else set())
    for w in every:                                   # what was not asked for was not written
        assert id(w) in written or bool(w.buf.isnan().all())


def test_backward_with_nothing_to_do_launches_nothing():
    M, N, K = 4, 8, 8
    z = lambda *s: torch.zeros(*s, device=dev())                               # noqa: E731
    db = out(N)
    ok(bwd(M, dict(dY=z(M, N), W=z(N, K), X=z(M, K), db=db.t)))
    torch.cuda.synchronize()
    assert bool(db.buf.isnan().all())


QUAD = [(17, 36), (64, 260), (130, 8), (6, 516)]


def test_four_problems_in_one_launch_equal_four_launches():
    M = 17
    gen = torch.Generator().manual_seed(4)
    ins = [dict(dY=g(randn(gen, M, N)), W=g(randn(gen, N, K, scale=K ** -0.5)), X=g(randn(gen, M, K)), bias=g(randn(gen, N)))
           for N, K in QUAD]

    def outs():
        return [dict(dW=out(N, K), db=out(N), slabs=out(cdiv(N, pick_nc(N)), M, K), Y=out(M, N)) for N, K in QUAD]

    def fprob(i, o):
        return dict(X=i["X"], W=i["W"], bias=i["bias"], Y=o["Y"].t)

    def bprob(i, o, N):
        return dict(dY=i["dY"], W=i["W"], X=i["X"], dW=o["dW"].t, db=o["db"].t, slabs=o["slabs"].t, nc=pick_nc(N))

    a, b = outs(), outs()
    ok(fwd(M, *(fprob(i, o) for i, o in zip(ins, a))))
    ok(bwd(M, *(bprob(i, o, N) for i, o, (N, K) in zip(ins, a, QUAD))))
    for i, o, (N, K) in zip(ins, b, QUAD):
        ok(fwd(M, fprob(i, o)))
        ok(bwd(M, bprob(i, o, N)))
    for i, oa, ob in zip(ins, a, b):
        assert H.rel_err(c64(oa["Y"].t), c64(i["X"]) @ c64(i["W"]).T + c64(i["bias"])) < 1e-5
        assert H.elem_err(c64(oa["dW"].t), c64(i["dY"]).T @ c64(i["X"])) < 1e-4
        assert H.elem_err(c64(oa["db"].t), c64(i["dY"]).sum(0)) < 1e-4
        assert H.elem_err(c64(oa["slabs"].t).sum(0), c64(i["dY"]) @ c64(i["W"])) < 1e-4
        for k in oa:
            assert torch.equal(oa[k].t, ob[k].t), k
            assert oa[k].untouched_outside() and ob[k].untouched_outside()


NC = [(4, 2), (8, 6), (12, 10), (12, 12), (64, 64), (130, 64), (256, 128)]


@pytest.mark.parametrize("K", [8, 516])
@pytest.mark.parametrize("N,nc", NC)
@pytest.mark.parametrize("M", [5, 32])
def test_dgrad_chunk_heights(M, N, nc, K):
    """Every even nc in 2..128 is a valid chunk height, also where N % 4 == 0 and the chunk is not whole float4's
    (nc = 2, 6, 10): each slab against fp64 dz[:, chunk]·W[chunk, :], and their sum through the reduce kernel."""
    gen = torch.Generator().manual_seed(N + nc + K + M)
    dY, W = randn(gen, M, N), randn(gen, N, K, scale=N ** -0.5)
    ns = cdiv(N, nc)
    sl, dX = out(ns, M, K), out(M, K)
    ok(bwd(M, dict(dY=g(dY), W=g(W), slabs=sl.t, nc=nc)))
    ok(red(M, [sl.t], K=K, dh=dX.t))
    want = torch.stack([dY.double()[:, s * nc:(s + 1) * nc] @ W.double()[s * nc:(s + 1) * nc] for s in range(ns)])
    assert H.elem_err(c64(sl.t), want.numpy()) < 1e-4
    assert H.elem_err(c64(dX.t), want.sum(0).numpy()) < 1e-4
    assert sl.untouched_outside() and dX.untouched_outside()


# ------------------------------------------------------------------------------------------------------------------
# 4. reduce
# ------------------------------------------------------------------------------------------------------------------
LAYOUTS = [(1,), (16,), (17,), (33,), (17, 1), (16, 33, 1), ()]       # (): `extra` alone


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "+".join(map(str, l)) or "extra")
@pytest.mark.parametrize("K", [4, 64, 65, 200])
@pytest.mark.parametrize("M", [1, 8, 9, 32])
def test_reduce_forms(M, K, layout):
    c = reduce_case(M, K, layout)
    sets, extra = [g(s) for s in c["sets"]], g(c["extra"])
    dh = out(M, K)
    ok(red(M, sets, K=K, extra=extra, dh=dh.t))
    assert H.rel_err(c64(dh.t), c["v"].numpy()) < 1e-5
    assert dh.untouched_outside()
    ln = dict(z=g(c["z"]), mu=g(c["mu"]), rs=g(c["rs"]), gamma=g(c["gam"]), beta=g(c["bet"]))
    for act in (RELU, GELU, NONE):
        runs = []
        for want_dh in (True, True, False):
            w = dict(G=out(M, K), dgamma=out(K), dbeta=out(K), rowpart=out(cdiv(K, 64), M, 2))
            if want_dh:
                w["dh"] = out(M, K)
            ok(red(M, sets, K=K, extra=extra, act=act, **ln, **{k: v.t for k, v in w.items()}))
            assert all(v.untouched_outside() for v in w.values())
            runs.append(w)
        for k in runs[0]:                                 # deterministic, and dh == NULL changes nothing else
            assert torch.equal(runs[0][k].t, runs[1][k].t), k
            assert k == "dh" or torch.equal(runs[0][k].t, runs[2][k].t), k
        assert torch.equal(runs[0]["dh"].t, dh.t)
        G, dg, db, rowpart = reduce_ref(c, act)
        for k, want in (("G", G), ("dgamma", dg), ("dbeta", db), ("rowpart", rowpart)):
            e = H.elem_err(c64(runs[0][k].t), want.numpy())
            assert e < 1e-4, (act, k, e)


# ------------------------------------------------------------------------------------------------------------------
# 5. one ReLU decision at three sites
# ------------------------------------------------------------------------------------------------------------------
def borderline_case(M, K=64):
    """z, gamma, beta, mu, rs (fp32) with a few hundred elements whose LayerNorm value is the cancellation residue of
    xhat*gamma + beta (|value| of the order of 1e-8, either sign: z is moved 0..3 ulp to either side of the fp64 root)
    and 4 columns where it is exactly 0 (beta = 0, z = mu)."""
    rng = np.random.default_rng(100 + M)
    f32 = np.float32
    mu, rs = rng.normal(size=M).astype(f32), (0.5 + rng.random(M)).astype(f32)
    gam = (rng.choice([-1.0, 1.0], K) * (0.5 + rng.random(K))).astype(f32)
    bet = (0.3 * rng.normal(size=K)).astype(f32)
    bet[:4] = 0
    z = (mu[:, None] + rng.normal(size=(M, K)) / rs[:, None]).astype(f32)
    root = (mu.astype(np.float64)[:, None] - bet.astype(np.float64) / (gam.astype(np.float64) * rs.astype(np.float64)[:, None])).astype(f32)
    steps = rng.integers(-3, 4, size=(M, K))
    for s in (1, 2, 3):
        root = np.where(steps >= s, np.nextafter(root, f32(np.inf)), np.where(steps <= -s, np.nextafter(root, f32(-np.inf)), root))
    near = rng.random((M, K)) < min(0.7, 400 / (M * K))
    z = np.where(near, root, z).astype(f32)
    z[:, :4] = mu[:, None]
    d = lambda a: torch.from_numpy(a.astype(np.float64))                      # noqa: E731
    v64 = (d(z) - d(mu)[:, None]) * d(rs)[:, None] * d(gam) + d(bet)
    assert int((v64 == 0).sum()) >= 4 * M
    assert int(((v64 > 0) & (v64 < 1e-6)).sum()) >= 40 and int(((v64 < 0) & (v64 > -1e-6)).sum()) >= 40
    assert int((v64.abs() < 1e-6).sum()) >= 150 and int((v64.abs() > 1e-5).sum()) >= 64
    return tuple(torch.from_numpy(a) for a in (z, gam, bet, mu, rs)) + (v64,)


@pytest.mark.parametrize("M", [5, 32])
def test_one_relu_decision_at_three_sites(M):
    """skinny.hip computes the LayerNorm value in one fixed operation order so that the forward prologue, the
    weight-gradient prologue and the reduce kernel's mask decide alike, borderline elements included."""
    K = 64
    z, gam, bet, mu, rs, v64 = borderline_case(M, K)
    z, gam, bet, mu, rs = g(z), g(gam), g(bet), g(mu), g(rs)
    # (a) forward through the identity: Y = relu(LN(z)), every MFMA product is with 1 or 0
    Y = out(M, K)
    ok(fwd(M, dict(X=z, W=torch.eye(K, device=dev()), Y=Y.t, gamma=gam, beta=bet, act=RELU, mu=mu, rs=rs)))
    # (b) weight gradient under dY = identity: dW[n, :] = the prologue's row n; both staging branches
    dWs = []
    for off in (0, 1):
        dW = out(M, K)
        ok(bwd(M, dict(dY=torch.eye(M, device=dev()), W=torch.zeros(M, K, device=dev()), X=place(z, off=off), xmu=mu, xrs=rs,
                       xgamma=gam, xbeta=bet, xact=RELU, dW=dW.t)))
        dWs.append(dW.t)
    # (c) reduce over one slab of ones: G = mask * gamma, gamma != 0
    G, dg, db, rowpart = out(M, K), out(K), out(K), out(1, M, 2)
    ok(red(M, [torch.ones(1, M, K, device=dev())], K=K, z=z, mu=mu, rs=rs, gamma=gam, beta=bet, act=RELU, G=G.t, dgamma=dg.t,
           dbeta=db.t, rowpart=rowpart.t))
    assert torch.equal(Y.t, dWs[0]) and torch.equal(Y.t, dWs[1])
    pos = (Y.t > 0).cpu()
    assert torch.equal((G.t != 0).cpu(), pos)
    clear = v64.abs() > 1e-5
    assert torch.equal(pos[clear], (v64 > 0)[clear])
    assert not bool(pos[v64 == 0].any())
    assert H.rel_err(c64(Y.t), torch.relu(v64).numpy()) < 1e-5


# ------------------------------------------------------------------------------------------------------------------
# 6. rows do not see each other
# ------------------------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_row_count():
    """Row m of the forward output and of the summed dgrad, computed among 32 rows and alone (M = 1), bit for bit: no
    step of either kernel mixes rows, and the two forward tile heights (16 and 32 rows) run the same chain per row."""
    M, K, N, nc = 32, 516, 65, 64
    c = ln_case(M, K, N, RELU, 1, given=True)
    D = {k: g(c[k]) for k in ("X", "W", "b", "gam", "bet", "A", "R")}
    mu, rs = g(c["mu"].float()), g(c["rs"].float())
    dY = g(randn(torch.Generator().manual_seed(6), M, N))
    ns = cdiv(N, nc)

    def run(m, rows):
        Y, sl, dX = out(m, N), out(ns, m, K), out(m, K)
        ok(fwd(m, dict(X=D["X"][rows].contiguous(), W=D["W"], bias=D["b"], Y=Y.t, gamma=D["gam"], beta=D["bet"], act=RELU,
                       mu=mu[rows].contiguous(), rs=rs[rows].contiguous(), in_addend=D["A"][rows].contiguous(),
                       out_addend=D["R"][rows].contiguous())))
        ok(bwd(m, dict(dY=dY[rows].contiguous(), W=D["W"], slabs=sl.t, nc=nc)))
        ok(red(m, [sl.t], K=K, dh=dX.t))
        return Y.t, dX.t

    Y, dX = run(M, slice(0, M))
    assert H.rel_err(c64(Y), c["want"].numpy()) < 1e-5
    assert H.elem_err(c64(dX), c64(dY) @ c64(D["W"])) < 1e-4
    for m in range(M):
        y1, dx1 = run(1, slice(m, m + 1))
        assert torch.equal(y1[0], Y[m]) and torch.equal(dx1[0], dX[m]), m


# ------------------------------------------------------------------------------------------------------------------
# 7. refusals: decided on the host, nothing is launched
# ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    M, K, N = 4, 16, 32
    z = lambda *s: torch.zeros(*s, device=dev())                               # noqa: E731
    X, W, Y, vec = z(M, K), z(N, K), z(M, N), z(K)
    base = dict(X=X, W=W, Y=Y)
    refused(fwd(M, dict(X=z(M, 6), W=z(N, 6), Y=Y)), ERR_ARG, "bad problem")
    refused(fwd(0, base), ERR_UNSUPPORTED, "M=0")
    refused(fwd(33, dict(X=z(33, K), W=W, Y=z(33, N))), ERR_UNSUPPORTED, "M=33")
    refused(fwd(M, dict(X=X, W=z(24, K), Y=z(M, 24), stat_part=z(2, M, 2))), ERR_UNSUPPORTED, "N % 16")
    refused(fwd(M, dict(base, gamma=vec, beta=vec, act=RELU, in_part=z(2, M, 2))), ERR_ARG, "statistics partials covering K")
    refused(fwd(M, dict(base, gamma=vec, beta=vec, act=RELU)), ERR_ARG, "statistics partials covering K")
    refused(fwd(M, dict(base, X=z(M, K + 1), ldx=K + 1)), ERR_UNSUPPORTED, "16-byte aligned")
    refused(fwd(M, dict(base, in_addend=z(M * K + 4)[1:1 + M * K].view(M, K))), ERR_UNSUPPORTED, "in_addend alignment")
    refused(fwd(M, dict(base, in_addend=z(M, K + 1)[:, :K])), ERR_UNSUPPORTED, "in_addend alignment")
    refused(fwd(M, *([base] * 5)), ERR_ARG, "problems per launch")
    refused(fwd(M), ERR_ARG, "problems per launch")

    dY, sl = z(M, N), z(N, M, K)                                               # slabs sized for any chunk height
    b = dict(dY=dY, W=W, X=X, dW=z(N, K), db=z(N), slabs=sl, nc=32)
    refused(bwd(M, *([b] * 5)), ERR_ARG, "problems per launch")
    refused(bwd(M), ERR_ARG, "problems per launch")
    refused(bwd(0, b), ERR_UNSUPPORTED, "M=0")
    refused(bwd(33, b), ERR_UNSUPPORTED, "M=33")
    refused(bwd(M, dict(dY=dY, W=z(N, 6), slabs=sl, nc=32)), ERR_ARG, "bad problem")
    refused(bwd(M, dict(b, z=Y, mu=z(M), rs=z(M))), ERR_ARG, "needs mu, rs, rowpart")
    for nc in (1, 3, 130):
        refused(bwd(M, dict(b, nc=nc)), ERR_ARG, "nc must be even")

    refused(red(0, [sl], K=K, dh=X), ERR_ARG, "bad arguments")
    refused(red(33, [sl], K=K, dh=X), ERR_ARG, "bad arguments")
    refused(red(M, [sl], K=K, dh=X, z=X, mu=z(M), rs=z(M), gamma=vec, beta=vec, G=z(M, K), dgamma=z(K), dbeta=z(K)), ERR_ARG, "rowpart")
    torch.cuda.synchronize()
