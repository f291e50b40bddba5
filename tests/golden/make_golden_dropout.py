#!/usr/bin/env python3
"""Golden fixture for the train-mode (dropout) check of the CPU oracle against the REFERENCE itself (build container
only): run the reference's EdgePredictor and PointCloudToWireframe in train mode with dropout on, record every mask torch
draws (torch.nn.functional.dropout is wrapped; nn.Dropout and MultiheadAttention both call it), and store the masks with
the outputs and parameter gradients they produced (tests/refsummary.py records; parameters and regenerated inputs as
sha256 digests).

    dropout.npz   edge.*   EdgePredictor(3, 512, 8), one batched forward of 2 samples (V = 9)
                  model.*  PointCloudToWireframe(8, 12), a ragged batch (vertex counts 12, 5, 2): one edge-head call per
                           sample, four masks each

Each of the four sites gets its own p (SITES_P), so that a permutation of sites cannot pass.  Masks are stored as packed
keep bits; the scale 1/(1-p) is the test's to apply.  tests/test_dropout_oracle.py feeds them to
oracle.reference_cpu (drop=) and holds its outputs and gradients to the recorded ones.

    WF3D_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dropout.py
"""
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
import torch.nn.functional as F  # noqa: E402

from models.PointCloudToWireframe import PointCloudToWireframe      # noqa: E402  (the reference)
from models.EdgePredictor import EdgePredictor                      # noqa: E402
from refsummary import digest, summarize                            # noqa: E402
import refcases                                                     # noqa: E402

# vertex_proj.5, attention, edge_mlp.3, edge_mlp.7 (the order of oracle/dropout.py SITES)
SITES_P = (0.05, 0.1, 0.2, 0.3)
EDGE_SEED, EDGE_SHAPE = 21, (2, 9, 3)
MODEL_SEED, MODEL_V, MODEL_X, MODEL_COUNTS = 22, 12, (3, 64, 8), (12, 5, 2)


def set_ps(ep):
    ep.vertex_proj[5].p, ep.attention.dropout, ep.edge_mlp[3].p, ep.edge_mlp[7].p = SITES_P
    return ep.train()


class Recorder:
    """Wraps F.dropout: every call with p > 0 in training is passed through and its keep-mask recorded."""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        self.orig = F.dropout

        def rec(input, p=0.5, training=True, inplace=False):
            out = self.orig(input, p, training, inplace)
            if training and p > 0:
                # the mask is read off the output; an input element that is exactly 0 would make it ambiguous
                assert not inplace and bool((input != 0).all()), "ambiguous dropout mask"
                self.calls.append((float(p), (out != 0).numpy().copy()))
            return out
        F.dropout = rec
        return self

    def __exit__(self, *a):
        F.dropout = self.orig


def store_masks(res, key, calls):
    for n, (p, m) in enumerate(calls):
        res[f"{key}.mask{n}.p"] = np.array(p)
        res[f"{key}.mask{n}.shape"] = np.array(m.shape, dtype=np.int64)
        res[f"{key}.mask{n}.bits"] = np.packbits(m.reshape(-1))
    res[key + ".nmasks"] = np.array(len(calls))


def params(m, res, key):
    res[key + ".names"] = np.array([n for n, _ in m.named_parameters()])
    res[key + ".digests"] = np.array([digest(p) for _, p in m.named_parameters()])


def grads(m, res, key):
    none = []
    for n, p in m.named_parameters():
        if p.grad is None:
            none.append(n)
        else:
            summarize(f"{key}.grad.{n}", p.grad, res)
    res[key + ".none_grads"] = np.array(none, dtype=str)


def edge(res):
    """One batched forward: the masks span both samples ([2, V, H], [2*heads, V, V], [2E, H], [2E, H/2])."""
    torch.manual_seed(EDGE_SEED)
    m = set_ps(EdgePredictor(3, 512, 8))
    v = torch.randn(*EDGE_SHAPE)
    params(m, res, "edge")
    res["edge.v"] = np.array(digest(v))
    m.double()
    v64 = v.double().requires_grad_()
    with Recorder() as r:
        probs, idx = m(v64)
    assert [p for p, _ in r.calls] == list(SITES_P), [p for p, _ in r.calls]
    store_masks(res, "edge", r.calls)
    summarize("edge.probs", probs, res)
    c = torch.randn(probs.shape)
    res["edge.cot"] = c.numpy()
    (probs * c.double()).sum().backward()
    summarize("edge.dv", v64.grad, res)
    grads(m, res, "edge")


def model(res):
    """Float64 throughout (the seeded float32 parameters, converted exactly), as refcheck_model.npz."""
    torch.manual_seed(MODEL_SEED)
    m = PointCloudToWireframe(8, MODEL_V)
    for s in m.modules():
        if isinstance(s, EdgePredictor):
            set_ps(s)
    m.train()
    x = torch.randn(*MODEL_X)
    x[0, 40:] = 0
    cnt = torch.tensor(MODEL_COUNTS)
    with torch.no_grad():
        m(x, cnt)                                    # the lazy layer is created here (no parameter draws after it)
    res["model.x"] = x.numpy()
    res["model.counts"] = cnt.numpy()
    params(m, res, "model")
    m.double()
    torch.set_default_dtype(torch.float64)
    try:
        with Recorder() as r:
            out = m(x.double(), cnt)
    finally:
        torch.set_default_dtype(torch.float32)
    assert len(r.calls) == 4 * len(MODEL_COUNTS), len(r.calls)
    assert [p for p, _ in r.calls] == list(SITES_P) * len(MODEL_COUNTS)
    store_masks(res, "model", r.calls)
    for k in refcases.MODEL_OUTPUTS:
        summarize("model.out." + k, out[k], res)
    c = {k: torch.randn(out[k].shape) for k in refcases.MODEL_COTANGENTS}
    for k in c:
        res["model.cot." + k] = c[k].numpy()
    sum((out[k] * c[k].double()).sum() for k in c).backward()
    grads(m, res, "model")


if __name__ == "__main__":
    res = {"sites_p": np.array(SITES_P)}
    edge(res)
    model(res)
    path = os.path.join(HERE, "dropout.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")
