"""The per-point encoder's backward under every subset of its three cotangents, on every route, against fp64.

EncoderFn / EncoderFnPacked / EncoderFnPackedSkip return (pooled, point_features, upooled) and call
ctx.set_materialize_grads(False), so each of the three cotangents (dpooled, dpf, dupooled) may arrive as None; the
backward then takes one of several routes per Linear (functional.Route).  The full-model tests only ever give it
(dpooled, None, dupooled) at the model's widths.  Here PointNetEncoder.encode / encode_packed are driven directly:

  - every row of CONFIGS selects one combination of routes and ASSERTS it on the autograd node, so no case can pass on
    another path than the one it names;
  - every non-empty subset of (g, point_features, upooled) receives a seeded Gaussian cotangent (point_features' scaled
    by 0.01), and EVERY element of EVERY parameter gradient is compared with the fp64 oracle run under the kernels' own
    decisions (tests/enc_cases.py; the method of tests/test_frozen_grad_gpu.py, whose bounds these are): forward outputs
    1e-4, gradients 1e-4 in fp32 and 4e-4 in bf16x3 with every GEMM forced onto the split path (TOL_X3_FORCED);
  - inputs are redrawn (up to 32 seeds) until no recomputed LayerNorm output lies within 5e-7 of 0; the masks of layers
    whose activated output exists as an sx8 operand are the forward kernel's own (kernel_masks);
  - the same through the packed layouts (host counts, pad rows, capacity tables from host and device counts with a cloud
    of no rows, tail="skip" with a NaN cotangent tail), through the input gradient, and through three properties that
    need no reference: None == explicit zeros, bit for bit; the first-max rule on duplicated points, near and a pool
    chunk apart.

Each test prints its worst tensor and error (pytest -s)."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import enc_cases as E  # noqa: E402
import helpers as H  # noqa: E402,F401

TOL = 1e-4                  # forward outputs, and gradients in fp32 mode
TOL_X3_FORCED = 4e-4        # bf16x3 gradients with SPLIT_MIN_ROWS = 1 (tests/test_frozen_grad_gpu.py)
DRAWS = 32
NAN = float("nan")


def dev():
    return torch.device("cuda:0")


def R(fwd, wgrad, dgrad):
    from wf3d.functional import Route
    return Route(fwd, wgrad, dgrad)


FIRST = ("first", "first", None)
FP32_0 = ("fp32", "fp32", None)         # layer 0 where the fused first-layer pass does not apply (fp32 mode, no hidden layer)
MODEL = [512, 1024, 2048, 1024]

# id -> hidden widths, output width, (B, N), precision, and the routes (fwd, wgrad, dgrad) of Linear 0 .. output it must show.
# TN wgrad: out % 256 == 0, in % 128 == 0, rows % 32 == 0; "transposes": both widths split (multiples of 8, >= 32), rows % 8
# == 0; split forward / dgrad: the reduction width a multiple of 8, >= 32 (functional._encoder_routes).
CONFIGS = {
    "tn-small":   dict(hidden=[128], out=256, B=2, N=48, precision="bf16x3", routes=[FIRST, ("split", "tn", "split")]),
    "tn-model":   dict(hidden=MODEL, out=512, B=2, N=48, precision="bf16x3", routes=[FIRST] + [("split", "tn", "split")] * 4),
    "transposes": dict(hidden=[64], out=40, B=2, N=48, precision="bf16x3", routes=[FIRST, ("split", "transposes", "split")]),
    "fp32-wgrad": dict(hidden=[64], out=40, B=3, N=11, precision="bf16x3", routes=[FIRST, ("split", "fp32", "split")]),
    "mixed":      dict(hidden=[64, 36], out=20, B=2, N=48, precision="bf16x3",
                       routes=[FIRST, ("split", "fp32", "fp32"), ("fp32", "fp32", "fp32")]),
    "no-hidden-x3": dict(hidden=[], out=32, B=2, N=48, precision="bf16x3", routes=[FP32_0]),
    "no-hidden-fp32": dict(hidden=[], out=32, B=2, N=48, precision="fp32", routes=[FP32_0]),
    "fp32-small": dict(hidden=[128], out=256, B=2, N=48, precision="fp32", routes=[FP32_0, ("fp32", "fp32", "fp32")]),
    "fp32-mixed": dict(hidden=[64, 36], out=20, B=2, N=48, precision="fp32", routes=[FP32_0] + [("fp32", "fp32", "fp32")] * 2),
    # the first-max rule a pool split apart: C = 64 takes the 16-byte pool kernel, N = 600 three splits of 200 rows
    "tie-far":    dict(hidden=[64], out=64, B=1, N=600, precision="bf16x3", routes=[FIRST, ("split", "transposes", "split")]),
}
# a packed batch runs over ops.ROW_PAD = 256-row multiples: there fp32-wgrad's rows % 8 == 0 again
PACKED_ROUTES = {"fp32-wgrad": [FIRST, ("split", "transposes", "split")]}

# layout -> (point counts, capacity, counts on the device, tail).  Host counts need every cloud to have a point
# (ops.point_counts_list), so the cloud of no rows comes with the device counts.
LAYOUTS = {
    "dense": None,
    "packed96": ([33, 1, 62], None, False, "compute"),
    "packed95": ([33, 7, 55], None, False, "compute"),          # M = 95: pad rows 95 .. 255 exist
    "cap-host": ([40, 1, 55], 256, False, "compute"),
    "cap-dev": ([40, 0, 56], 256, True, "compute"),
    "skip": ([40, 0, 56], 256, True, "skip"),
    "packed-far": ([420, 30, 100], None, False, "compute"),     # cloud 0 spans the 256-row chunk boundary
}


@contextlib.contextmanager
def mode(precision):
    """Precision and SPLIT_MIN_ROWS = 1 for the body, as the `precision` fixture of tests/test_degenerate_values_gpu.py."""
    from wf3d import config
    old = (config.precision(), config.SPLIT_MIN_ROWS)
    config.set_precision(precision)
    config.SPLIT_MIN_ROWS = 1
    try:
        yield
    finally:
        config.set_precision(old[0])
        config.SPLIT_MIN_ROWS = old[1]


_ENCODERS = {}


def encoder(cfg):
    """One PointNetEncoder per width set for the whole file (its values never change: only .grad does)."""
    from models.PointNetEncoder import PointNetEncoder
    key = (tuple(cfg["hidden"]), cfg["out"])
    if key not in _ENCODERS:
        torch.manual_seed(20)
        enc = PointNetEncoder(8, cfg["hidden"], cfg["out"]).to(dev())
        E.perturb_1d(enc)
        _ENCODERS[key] = enc
    enc = _ENCODERS[key]
    enc.zero_grad(set_to_none=True)
    return enc.set_packed_tail("compute")


class Batch:
    """One input in one layout: the points as encode / encode_packed take them, and how a row of a cloud is addressed."""

    def __init__(self, cfg, layout, seed):
        self.layout, self.spec = layout, LAYOUTS[layout]
        if self.spec is None:
            self.x = E.dense_input(seed, cfg["B"], cfg["N"])
            self.counts = [cfg["N"]] * cfg["B"]
        else:
            self.counts = self.spec[0]
            self.x = E.packed_input(seed, self.counts)
        self.M = sum(self.counts)
        self.offsets = [sum(self.counts[:b]) for b in range(len(self.counts))]

    def copy_row(self, cloud, i, j):
        if self.spec is None:
            self.x[cloud, j] = self.x[cloud, i]
        else:
            o = self.offsets[cloud]
            self.x[o + j] = self.x[o + i]

    def rows(self):
        """Rows the per-point MLP runs over."""
        if self.spec is None:
            return self.M
        return self.spec[1] or -(-self.M // 256) * 256

    def run(self, enc, tail=None, requires_grad=False):
        """(outs {g, pf, up} with pf cut to the clouds' rows, pf as returned, the input leaf)."""
        if self.spec is None:
            xd = self.x.to(dev()).requires_grad_(requires_grad)
            g, pf, up = enc.encode(xd)
            return {"g": g, "pf": pf, "up": up}, pf, xd
        counts, cap, on_dev, tail0 = self.spec
        pts = self.x
        if cap is not None:
            pts = torch.zeros(cap, self.x.shape[1])
            pts[:self.M] = self.x
        enc.set_packed_tail(tail or tail0)
        arg = torch.tensor(counts, device=dev()) if on_dev else counts
        g, pf, up = enc.encode_packed(pts.to(dev()), arg, capacity=cap)
        enc.set_packed_tail("compute")
        return {"g": g, "pf": pf[:self.M], "up": up}, pf, None


def pick_tie(node, batch, cloud, lo, hi):
    """The row i of `cloud` in [lo, hi) that most channels name as BOTH pools' arg-max (None if there is none)."""
    arg_m, arg_u = node.saved[5][cloud].long().cpu(), node.saved[6][cloud].long().cpu()
    n = batch.counts[cloud]
    cm = torch.bincount(arg_m[arg_m >= 0], minlength=n)[lo:hi]
    cu = torch.bincount(arg_u[arg_u >= 0], minlength=n)[lo:hi]
    score = torch.minimum(cm, cu)
    return lo + int(score.argmax()) if int(score.max()) > 0 else None


class Result:
    pass


def drive(cid, subset, layout="dense", want_dx=False, tie=None, tail=None, poison=False):
    """Runs config `cid` in `layout` on the first borderline-free input, backpropagates the cotangents of `subset`, and
    compares with the fp64 oracle under the captured decisions.  tie = (cloud, lo, hi, delta): the cloud's row i in
    [lo, hi) that most channels pool from is copied to row i + delta first.  poison: the point_features cotangent is NaN
    in the rows behind the clouds (a capacity layout)."""
    from oracle.frozen import capture_encoder_decisions
    cfg = CONFIGS[cid]
    x3 = cfg["precision"] != "fp32"
    res = Result()
    with mode(cfg["precision"]):
        enc = encoder(cfg)
        for seed in range(100, 100 + DRAWS):
            batch = Batch(cfg, layout, seed)
            if tie is not None:
                cloud, lo, hi, delta = tie
                outs, _, _ = batch.run(enc, tail)
                i = pick_tie(outs["g"].grad_fn.next_functions[0][0], batch, cloud, lo, hi)
                if i is None:
                    continue
                batch.copy_row(cloud, i, i + delta)
                res.tie = (cloud, i, i + delta)
            outs, pf_full, xd = batch.run(enc, tail, requires_grad=want_dx)
            frozen, n_border, node = capture_encoder_decisions(outs["g"], enc, kernel_masks=x3,
                                                               rows=None if batch.spec is None else batch.M)
            if n_border == 0:
                break
        else:
            pytest.fail(f"no borderline-free input found in {DRAWS} draws")
        res.seed, res.routes, res.live = seed, list(node.routes), node.live
        res.arg_m, res.arg_u = frozen["argmax"]["enc_masked"], frozen["argmax"]["vert_unmasked"]
        want = PACKED_ROUTES.get(cid, cfg["routes"]) if batch.spec is not None else cfg["routes"]
        want = [R(*r) for r in want]
        if want_dx:
            want[0] = R(want[0][0], "fp32", "fp32")
        assert res.routes == want, (cid, layout, res.routes)
        assert node.saved[0].shape[0] == batch.rows()

        cot = E.cotangents(seed + 1000, {k: tuple(outs[k].shape) for k in E.OUTS})
        keys = [k for k in E.OUTS if k in subset]
        heads = {"g": outs["g"], "pf": pf_full, "up": outs["up"]}
        cots = {k: cot[k].to(dev()) for k in keys}
        if "pf" in keys and pf_full.shape[0] != outs["pf"].shape[0]:
            full = torch.full(tuple(pf_full.shape), NAN if poison else 0.0)
            full[:batch.M] = cot["pf"]
            cots["pf"] = full.to(dev())
        torch.autograd.backward([heads[k] for k in keys], [cots[k] for k in keys])
        res.got = E.np_grads(enc)

        P = E.params64(enc)
        x64 = batch.x.double().requires_grad_(want_dx)
        ref = E.ref_dense(P, x64, frozen) if batch.spec is None else E.ref_packed(P, x64, batch.counts, frozen)
        ref = dict(zip(E.OUTS, ref))
        sum((ref[k] * cot[k].double()).sum() for k in keys).backward()
        res.fwd = E.out_errors(outs, ref)
        res.errs = E.grad_errors(res.got, P)
        if want_dx:
            res.errs["x"] = H.elem_err(xd.grad.cpu().numpy(), x64.grad.numpy())
        res.tol = TOL_X3_FORCED if x3 else TOL
    return res


def check(res, tag):
    worst = sorted(((e, n) for n, e in res.errs.items()), reverse=True)[:3]
    print(f"{tag} (seed {res.seed}): worst gradient errors {[(f'{e:.1e}', n) for e, n in worst]}; forward "
          f"{ {k: (f'{a:.1e}', f'{b:.1e}') for k, (a, b) in res.fwd.items()} }")
    for k, (a, b) in res.fwd.items():
        assert a < TOL and b < TOL, (tag, k, a, b)
    assert res.errs, tag
    bad = [(n, e) for n, e in res.errs.items() if not e <= res.tol]
    assert not bad, (tag, res.seed, bad)


def subset_id(s):
    return "+".join(s)


# ----------------------------------------------------------------------------------------------------------------------
# the route table x every cotangent subset, dense
# ----------------------------------------------------------------------------------------------------------------------
TABLE = ["tn-small", "tn-model", "transposes", "fp32-wgrad", "mixed", "no-hidden-x3", "no-hidden-fp32", "fp32-small", "fp32-mixed"]


@pytest.mark.parametrize("subset", E.SUBSETS, ids=subset_id)
@pytest.mark.parametrize("cid", TABLE)
def test_every_cotangent_subset_on_every_route(cid, subset):
    res = drive(cid, subset)
    check(res, f"{cid} {subset_id(subset)}")
    n_mlp = 4 * len(CONFIGS[cid]["hidden"]) + 2
    # the fusion MLP is reached through g alone
    assert len(res.errs) == n_mlp + (10 if "g" in subset else 0)


# ----------------------------------------------------------------------------------------------------------------------
# layouts
# ----------------------------------------------------------------------------------------------------------------------
LAYOUT_SUBSETS = [("g",), ("pf",), ("g", "pf", "up")]


@pytest.mark.parametrize("subset", LAYOUT_SUBSETS, ids=subset_id)
@pytest.mark.parametrize("layout", ["packed96", "packed95", "cap-host", "cap-dev"])
@pytest.mark.parametrize("cid", ["tn-small", "transposes", "tn-model"])
def test_packed_layouts(cid, layout, subset):
    res = drive(cid, subset, layout)
    check(res, f"{cid} {layout} {subset_id(subset)}")
    assert res.live is None
    if layout == "cap-dev":                 # the cloud of no rows: no arg-max row, and none of its zeros reached a gradient
        assert bool((res.arg_m[1] == -1).all()) and bool((res.arg_u[1] == -1).all())


@pytest.mark.parametrize("subset", LAYOUT_SUBSETS, ids=subset_id)
@pytest.mark.parametrize("cid", ["tn-small", "transposes", "tn-model"])
def test_packed_tail_skip(cid, subset):
    """Capacity 256 under set_packed_tail("skip"): the live total is 96, so the 256-row extent above it is the capacity
    itself and no row at or past it exists; the point_features cotangent is NaN from the live total to that boundary,
    rows no cloud owns, which the pool backward never reads (include/wf3d.h: dpf_direct needs only the clouds' rows, the
    pad rows are written as zeros).  Same values against the oracle, and bit-equal to the "compute" run."""
    res = drive(cid, subset, "skip", poison=True)
    check(res, f"{cid} skip {subset_id(subset)}")
    assert res.live is not None, "the skip run fell back to computing the tail"
    ref = drive(cid, subset, "skip", tail="compute")
    assert ref.live is None and ref.seed == res.seed
    for n, a in ref.got.items():
        b = res.got[n]
        assert (a is None and b is None) or torch.equal(a, b), n


# ----------------------------------------------------------------------------------------------------------------------
# the input gradient
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subset", [("g",), ("pf", "up")], ids=subset_id)
@pytest.mark.parametrize("cid", ["tn-small", "mixed"])
def test_input_gradient(cid, subset):
    """x.requires_grad: layer 0 leaves the fused backward (dx = dz·W needs dz) for the fp32 wgrad and dgrad, which drive()
    asserts on the node; x.grad is compared element-wise like the parameters' ("x" in the errors)."""
    res = drive(cid, subset, want_dx=True)
    assert res.routes[0][1:3] == ("fp32", "fp32") and "x" in res.errs
    check(res, f"{cid} dx {subset_id(subset)}")


# ----------------------------------------------------------------------------------------------------------------------
# properties that need no reference
# ----------------------------------------------------------------------------------------------------------------------
PROPERTY_CONFIGS = ["tn-small", "transposes", "fp32-wgrad"]


def _grads(cid, layout, present, zeros):
    """Parameter gradients with the cotangents of `present` given, those of `zeros` passed as explicit zeros tensors."""
    cfg = CONFIGS[cid]
    with mode(cfg["precision"]):
        enc = encoder(cfg)
        batch = Batch(cfg, layout, 100)
        outs, _, _ = batch.run(enc)
        cot = E.cotangents(77, {k: tuple(outs[k].shape) for k in E.OUTS})
        keys = [k for k in E.OUTS if k in present or k in zeros]
        cots = [torch.zeros_like(outs[k]) if k in zeros else cot[k].to(dev()) for k in keys]
        torch.autograd.backward([outs[k] for k in keys], cots)
        return E.np_grads(enc)


@pytest.mark.parametrize("absent", E.OUTS)
@pytest.mark.parametrize("layout", ["dense", "packed95"])
@pytest.mark.parametrize("cid", PROPERTY_CONFIGS)
def test_none_cotangent_equals_zeros(cid, layout, absent):
    """A cotangent that is absent (None reaches the backward: set_materialize_grads(False)) against the same cotangent
    passed as zeros of the output's shape, the other two present: adding exact zeros changes no bit, so every parameter
    gradient is torch.equal; a difference means the None branch computes something else.  (Without a cotangent for g the
    fusion MLP is not reached and has no gradient; with a zero one its gradients are exact zeros.)"""
    present = tuple(k for k in E.OUTS if k != absent)
    a, b = _grads(cid, layout, present, ()), _grads(cid, layout, present, (absent,))
    for n in a:
        assert b[n] is not None, n
        if a[n] is None:
            assert absent == "g" and not bool(b[n].any()), n
        else:
            assert torch.equal(a[n], b[n]), (n, float((a[n] - b[n]).abs().max()))
    assert any(v is not None and bool(v.any()) for v in a.values())


def _tie(cid, layout, tie):
    res = drive(cid, ("g", "pf", "up"), layout, tie=tie)
    cloud, i, j = res.tie
    for arg in (res.arg_m, res.arg_u):
        assert not bool((arg[cloud] == j).any()), (cid, layout, "the later of two equal rows was recorded", i, j)
        assert bool((arg[cloud] == i).any()), (cid, layout, "the duplicated row is no channel's arg-max", i, j)
    check(res, f"{cid} {layout} tie rows {i}, {j}")


@pytest.mark.parametrize("layout", ["dense", "packed96"])
@pytest.mark.parametrize("cid", PROPERTY_CONFIGS)
def test_first_max_rule_on_a_duplicated_point(cid, layout):
    """Point row i of cloud 0 copied to the next row, both valid: every channel ties between them, neither arg_m nor
    arg_u may name the copy, some channel names i (the tie is live), and the gradients pass the oracle comparison."""
    n = CONFIGS[cid]["N"] if layout == "dense" else LAYOUTS[layout][0][0]
    _tie(cid, layout, (0, 0, n - n // 4 - 1, 1))


def test_first_max_rule_across_pool_splits_dense():
    """B = 1, N = 600, C = 64: three pool splits of 200 rows; i in the first one, its copy 250 rows on (valid rows end at
    450)."""
    _tie("tie-far", "dense", (0, 0, 200, 250))


def test_first_max_rule_across_chunks_packed():
    """A 420-row cloud of a packed batch is two chunks (256 rows each at most): i in rows 0 .. 49 of the first, its copy
    260 rows on in the second (valid rows end at 315)."""
    _tie("tie-far", "packed-far", (0, 0, 50, 260))
