#!/usr/bin/env python3
"""Golden fixture for the dropout sites of the encoder and the vertex head (build container only): run the REFERENCE's
PointNetEncoder and VertexPredictor in train mode with a different p at every nn.Dropout, record every mask, and store
the masks with the outputs and parameter gradients they produced (tests/refsummary.py records; parameters and
regenerated inputs as sha256 digests).

    dropout_sites.npz   enc.*    PointNetEncoder(8, [32, 64], 16) on [2, 16, 8]: sites mlp.3, mlp.7
                        vert.*   VertexPredictor(512, 8) on B = 2 with point_features [2, 6, 16]: vertex_mlp1..4[3]

These sites follow a ReLU, so half of their input is exact zeros and a mask cannot be read off the output (the method
of make_golden_dropout.py).  torch.nn.functional.dropout is therefore replaced by a function that draws the keep mask
itself (torch.rand_like(x) >= p), records it and returns x * keep / (1 - p): the reference's modules, its placement of
every site, torch's scale — only the random stream is ours, and the test replays the recorded masks, not the stream.
Masks are stored as packed keep bits.  tests/test_dropout_sites_model.py feeds them to tests/dropout_sites_model.py and
holds its outputs and gradients to the recorded ones.

    WF3D_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dropout_sites.py
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
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from models.PointNetEncoder import PointNetEncoder                  # noqa: E402  (the reference)
from models.VertexPredictor import VertexPredictor                  # noqa: E402
from refsummary import digest, summarize                            # noqa: E402
from make_golden_dropout import grads, params, store_masks          # noqa: E402

ENC_SEED, ENC_ARGS, ENC_X, ENC_P = 31, (8, [32, 64], 16), (2, 16, 8), (0.15, 0.35)
VERT_SEED, VERT_ARGS, VERT_B, VERT_PF, VERT_P = 32, (512, 8), 2, (2, 6, 16), (0.05, 0.1, 0.2, 0.3)


class Recorder:
    """Replaces F.dropout: a call with p > 0 in training draws its own keep mask, records it and applies it."""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        self.orig = F.dropout

        def rec(input, p=0.5, training=True, inplace=False):
            if not training or p == 0:
                return self.orig(input, p, training, inplace)
            keep = torch.rand_like(input) >= p
            self.calls.append((float(p), keep.numpy().copy()))
            return input * keep.to(input.dtype) / (1.0 - p)
        F.dropout = rec
        return self

    def __exit__(self, *a):
        F.dropout = self.orig


def set_ps(m, ps):
    drops = [s for s in m.modules() if isinstance(s, nn.Dropout)]
    assert len(drops) == len(ps)
    for s, p in zip(drops, ps):
        s.p = p
    return m.train()


def enc(res):
    torch.manual_seed(ENC_SEED)
    m = set_ps(PointNetEncoder(*ENC_ARGS), ENC_P)
    x = torch.randn(*ENC_X)
    x[0, 12:] = 0
    params(m, res, "enc")
    res["enc.x"] = np.array(digest(x))
    m.double()
    with Recorder() as r:
        g, pf = m(x.double())
    assert [p for p, _ in r.calls] == list(ENC_P), [p for p, _ in r.calls]
    store_masks(res, "enc", r.calls)
    summarize("enc.g", g, res)
    summarize("enc.pf", pf, res)
    cg, cpf = torch.randn(g.shape), torch.randn(pf.shape)
    res["enc.cot.g"], res["enc.cot.pf"] = cg.numpy(), cpf.numpy()
    ((g * cg.double()).sum() + (pf * cpf.double()).sum()).backward()
    grads(m, res, "enc")


def vert(res):
    torch.manual_seed(VERT_SEED)
    m = set_ps(VertexPredictor(*VERT_ARGS), VERT_P)
    g = torch.randn(VERT_B, VERT_ARGS[0])
    pf = torch.randn(*VERT_PF)
    with torch.no_grad():
        m(g, pf)                                     # the lazy layer is created here (no parameter draws after it)
    params(m, res, "vert")
    res["vert.g"], res["vert.pf"] = np.array(digest(g)), np.array(digest(pf))
    m.double()
    g64, pf64 = g.double().requires_grad_(), pf.double().requires_grad_()
    with Recorder() as r:
        out = m(g64, pf64)
    assert [p for p, _ in r.calls] == list(VERT_P), [p for p, _ in r.calls]
    store_masks(res, "vert", r.calls)
    cot = {}
    for k in ("vertices", "existence_probabilities"):
        summarize("vert.out." + k, out[k], res)
        cot[k] = torch.randn(out[k].shape)
        res["vert.cot." + k] = cot[k].numpy()
    res["vert.out.actual_vertex_counts"] = out["actual_vertex_counts"].numpy()
    sum((out[k] * cot[k].double()).sum() for k in cot).backward()
    summarize("vert.dg", g64.grad, res)
    summarize("vert.dpf", pf64.grad, res)
    grads(m, res, "vert")


if __name__ == "__main__":
    res = {"enc.sites_p": np.array(ENC_P), "vert.sites_p": np.array(VERT_P)}
    enc(res)
    vert(res)
    path = os.path.join(HERE, "dropout_sites.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")
