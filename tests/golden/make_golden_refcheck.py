#!/usr/bin/env python3
"""Golden fixtures for the checks of the project against the REFERENCE itself (build container only): run the reference's
models, losses.WireframeLoss and eval.ap_calculator on the inputs the tests regenerate, and store what they return
(tests/refsummary.py: whole up to 1024 elements, else max |.|, a seeded sample and row / column sums; parameters and
regenerated inputs as sha256 digests).

    refcheck_init.npz   seeded initialisation of PointCloudToWireframe(8, 12)      tests/test_dropin_surface.py
    refcheck_model.npz  PointCloudToWireframe(8, 9) forward + parameter gradients   tests/test_oracle_vs_reference.py
    refcheck_sizes.npz  the three sub-modules at the size-sweep constructor sizes   tests/test_oracle_vs_reference.py
    refcheck_loss.npz   WireframeLoss at the device-loss sweep shapes               tests/test_loss_vs_reference.py
    refcheck_eval.npz   APCalculator on random and degenerate batches               tests/test_eval_vs_reference.py

    WF3D_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_refcheck.py
"""
import contextlib
import copy
import importlib.util
import io
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REF = os.environ.get("WF3D_REFERENCE") or sys.exit("set WF3D_REFERENCE to a checkout of the reference project")
sys.path.insert(0, REF)
sys.path.append(TESTS)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from models.PointCloudToWireframe import PointCloudToWireframe      # noqa: E402  (the reference)
from models.PointNetEncoder import PointNetEncoder                  # noqa: E402
from models.EdgePredictor import EdgePredictor                      # noqa: E402
from models.VertexPredictor import VertexPredictor                  # noqa: E402
from refsummary import digest, summarize                            # noqa: E402
import refcases                                                     # noqa: E402


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def save(tag, res):
    path = os.path.join(HERE, f"refcheck_{tag}.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")


def quiet(m):
    for s in m.modules():
        if isinstance(s, torch.nn.Dropout):
            s.p = 0.0
        if isinstance(s, torch.nn.MultiheadAttention):
            s.dropout = 0.0
    return m.train()


def params(m, res, key):
    names = [n for n, _ in m.named_parameters()]
    res[key + ".names"] = np.array(names)
    res[key + ".digests"] = np.array([digest(p) for _, p in m.named_parameters()])


def grads(m, res, key):
    none = []
    for n, p in m.named_parameters():
        if p.grad is None:
            none.append(n)
        else:
            summarize(f"{key}.grad.{n}", p.grad, res)
    res[key + ".none_grads"] = np.array(none, dtype=str)


def init():
    torch.manual_seed(1234)
    m = PointCloudToWireframe(8, 12)
    sd = m.state_dict()
    res = {"state_dict.keys": np.array(list(sd)), "state_dict.digests": np.array([digest(v) for v in sd.values()])}
    params(m, res, "params")
    save("init", res)


def model():
    """Recorded in float64 (the seeded float32 parameters, converted exactly): the oracle is compared in float64 too, so
    the comparison does not depend on the float32 summation order of the CPU it runs on."""
    torch.manual_seed(5)
    m = quiet(PointCloudToWireframe(8, 9))
    x = torch.randn(2, 150, 8)
    x[0, 100:] = 0
    cnt = torch.tensor([9, 3])
    with torch.no_grad():
        m(x, cnt)                                    # default torch init, the lazy layer is created here (no draws after it)
    res = {"x": x.numpy(), "counts": cnt.numpy()}
    params(m, res, "params")
    m.double()
    torch.set_default_dtype(torch.float64)
    try:
        out = m(x.double(), cnt)
    finally:
        torch.set_default_dtype(torch.float32)
    res["edge_indices"] = np.array([len(e) for e in out["edge_indices"]], dtype=np.int64)
    res["edge_indices.flat"] = np.array([p for e in out["edge_indices"] for p in e], dtype=np.int64).reshape(-1, 2)
    for k in refcases.MODEL_OUTPUTS:
        summarize("out." + k, out[k], res)
    c = {k: torch.randn(out[k].shape) for k in refcases.MODEL_COTANGENTS}
    for k in c:
        res["cot." + k] = c[k].numpy()
    sum((out[k] * c[k].double()).sum() for k in c).backward()
    grads(m, res, "params")
    save("model", res)


def sizes():
    res = {}
    torch.manual_seed(1)
    for i, (hidden, out_dim) in enumerate(refcases.ENCODER_SIZES):
        key = f"enc{i}"
        m = quiet(PointNetEncoder(8, hidden, out_dim))
        params(m, res, key)
        x = torch.randn(3, 70, 8)
        x[:, ::9] = 0
        res[key + ".x"] = np.array(digest(x))
        g, pf = m(x)
        summarize(key + ".g", g, res)
        summarize(key + ".pf", pf, res)
        cg, cp = torch.randn_like(g), torch.randn_like(pf)
        res[key + ".cot"] = np.array([digest(cg), digest(cp)])
        ((g * cg).sum() + (pf * cp).sum()).backward()
        grads(m, res, key)
    for i, (vd, hidden, heads, cnt) in enumerate(refcases.EDGE_SIZES):
        key = f"edge{i}"
        m = quiet(EdgePredictor(vd, hidden, heads))
        params(m, res, key)
        v = torch.randn(1, cnt, vd, requires_grad=True)
        res[key + ".v"] = np.array(digest(v))
        probs, idx = m(v)
        res[key + ".idx"] = np.array(idx, dtype=np.int64).reshape(-1, 2)
        summarize(key + ".probs", probs, res)
        c = torch.randn_like(probs)
        res[key + ".cot"] = np.array([digest(c)])
        (probs * c).sum().backward()
        summarize(key + ".dv", v.grad, res)
        grads(m, res, key)
    for i, (gdim, V) in enumerate(refcases.VERTEX_SIZES):
        key = f"vert{i}"
        m = quiet(VertexPredictor(gdim, V, 4))
        g = torch.randn(3, gdim, requires_grad=True)
        pf = torch.randn(3, 9, gdim, requires_grad=True)
        res[key + ".inputs"] = np.array([digest(g), digest(pf)])
        o = m(g, pf)                                  # creates the lazy point_pool_proj
        params(m, res, key)
        summarize(key + ".vertices", o["vertices"], res)
        summarize(key + ".existence_probabilities", o["existence_probabilities"], res)
        res[key + ".actual_vertex_counts"] = o["actual_vertex_counts"].numpy()
        cv, ce = torch.randn_like(o["vertices"]), torch.randn_like(o["existence_probabilities"])
        res[key + ".cot"] = np.array([digest(cv), digest(ce)])
        ((o["vertices"] * cv).sum() + (o["existence_probabilities"] * ce).sum()).backward()
        summarize(key + ".dg", g.grad, res)
        summarize(key + ".dpf", pf.grad, res)
        grads(m, res, key)
    save("sizes", res)


def loss():
    ref = load("ref_loss", os.path.join(REF, "losses", "WireframeLoss.py"))
    res = {}
    for i, shape in enumerate(refcases.LOSS_SHAPES):
        key = f"case{i}"
        p, tg = refcases.loss_inputs(*shape)
        res[key + ".inputs"] = np.array([digest(t) for t in list(p.values()) + list(tg.values())])
        p = {k: v.clone().requires_grad_() for k, v in p.items()}
        with contextlib.redirect_stdout(io.StringIO()):
            out = ref.WireframeLoss(3.0, 1.5, 1.0)(p, tg)
        out["total_loss"].backward()
        for k in refcases.LOSS_KEYS:
            res[f"{key}.{k}"] = np.array(float(out[k]))
        for k, v in p.items():
            summarize(f"{key}.grad.{k}", v.grad if v.grad is not None else torch.zeros_like(v), res)
    save("loss", res)


def evaluation():
    ref = load("ref_ap", os.path.join(REF, "eval", "ap_calculator.py"))
    res = {}
    rng = np.random.RandomState(3)
    for t, thr in enumerate(refcases.EVAL_THRESHOLDS):
        calc = ref.APCalculator(distance_thresh=thr)
        for c, case in enumerate(refcases.EVAL_CASES):
            batch = refcases.eval_sample(rng, *case)
            res[f"t{t}.c{c}.batch"] = np.array(refcases.eval_batch_digest(batch))
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    calc.compute_metrics(copy.deepcopy(batch))          # it overwrites matched predicted edges in place
                err = ""
            except Exception as e:                                      # no edge within the radius: numpy refuses min() of nothing
                err = type(e).__name__
            res[f"t{t}.c{c}.error"] = np.array(err)
            res[f"t{t}.c{c}.ap"] = np.array([float(calc.ap_dict[k]) for k in refcases.EVAL_KEYS])
        with contextlib.redirect_stdout(io.StringIO()):
            calc.output_accuracy()
        res[f"t{t}.accuracy"] = np.array([float(calc.ap_dict[k]) for k in refcases.EVAL_ACCURACY_KEYS])
    p, t = rng.normal(0, 3, (40, 2, 3)), rng.normal(0, 3, (9, 2, 3))
    res["hausdorff.inputs"] = np.array([digest(p), digest(t)])
    res["hausdorff"] = np.asarray(ref.hausdorff_distance_line(p, t), dtype=np.float64)
    save("eval", res)


if __name__ == "__main__":
    init()
    model()
    sizes()
    loss()
    evaluation()
