#!/usr/bin/env python3
"""Generate tests/golden/packed.npz by running the REFERENCE's own model on each cloud alone (B = 1).

Run in the build container only (needs the reference, read-only), like make_golden.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_packed.py

A packed batch (PointCloudToWireframe.forward_packed) is defined cloud by cloud: outputs and gradients of cloud b are those
of the reference model on x_b[None], parameter gradients the sum over the clouds.  Four clouds of different lengths — one
with a zero-row tail, one shorter than 64 points — run through one model (one seed) at B = 1; the outputs are stored
in batch form (row b = cloud b, edge_probs zero-padded to the widest sample), the gradients as the summaries
helpers.grad_summary_of produces, of the gradients summed over the four clouds.  Only names / seeds of the detgen
recipes and numeric results are stored; no weights.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np   # noqa: E402
import torch         # noqa: E402

import make_golden as MG   # noqa: E402  (puts the reference and the repository root on sys.path, imports its classes)
from oracle import detgen  # noqa: E402

TAG, SEED, V = "packed", 31, 12
POINT_COUNTS = [300, 37, 1100, 517]
ZERO_TAIL = (0, 60)                   # cloud 0: its last 60 rows are zero
VERTEX_COUNTS = [12, 4, 9, 2]
KEYS = ("vertices", "existence_probabilities", "edge_probs")


def cloud(b):
    x = detgen.normalish(f"{TAG}.x{b}", (1, POINT_COUNTS[b], 8), SEED)
    if b == ZERO_TAIL[0]:
        x[0, POINT_COUNTS[b] - ZERO_TAIL[1]:] = 0.0
    return x


def main():
    torch.manual_seed(0)
    model = MG.PointCloudToWireframe(input_dim=8, max_vertices=V)
    MG.zero_dropout(model)
    model.train()
    with torch.no_grad():                       # creates the lazy point_pool_proj
        model(torch.from_numpy(cloud(1)), torch.tensor([2]))
    MG.load_detgen(model, SEED)
    B = len(POINT_COUNTS)
    max_e = max(c * (c - 1) // 2 for c in VERTEX_COUNTS)
    res = {"meta.seed": np.array(SEED), "meta.V": np.array(V), "meta.point_counts": np.array(POINT_COUNTS, dtype=np.int64),
           "meta.zero_tail": np.array(ZERO_TAIL, dtype=np.int64), "meta.counts": np.array(VERTEX_COUNTS, dtype=np.int64)}
    outs = {"vertices": np.zeros((B, V, 3), np.float32), "existence_probabilities": np.zeros((B, V), np.float32),
            "edge_probs": np.zeros((B, max_e), np.float32), "global_features": np.zeros((B, 512), np.float32)}
    avc, lens, flat, loss_sum = [], [], [], 0.0
    for b in range(B):
        out = model(torch.from_numpy(cloud(b)), torch.tensor(VERTEX_COUNTS[b:b + 1]))
        for k in ("vertices", "existence_probabilities", "global_features"):
            outs[k][b] = out[k].detach().numpy()[0]
        e = out["edge_probs"].shape[1]
        outs["edge_probs"][b, :e] = out["edge_probs"].detach().numpy()[0]
        avc.append(int(out["actual_vertex_counts"][0]))
        lens.append(len(out["edge_indices"][0]))
        flat += list(out["edge_indices"][0])
        cot = {k: torch.from_numpy(detgen.uniform(f"{TAG}.cot{b}.{k}", tuple(out[k].shape), -1, 1, SEED)) for k in KEYS}
        loss = sum((out[k] * cot[k]).sum() for k in cot)
        loss.backward()                          # .grad accumulates: the sum over the clouds
        loss_sum += loss.item()
    for k, v in outs.items():
        res["out." + k] = v
    res["out.actual_vertex_counts"] = np.array(avc, dtype=np.int64)
    res["out.edge_index_lens"] = np.array(lens, dtype=np.int64)
    res["out.edge_indices_flat"] = np.array(flat, dtype=np.int64).reshape(-1, 2)
    res["out.loss"] = np.array(loss_sum)
    MG.grad_summary(model.named_parameters(), res)
    np.savez_compressed(os.path.join(HERE, TAG + ".npz"), **res)
    print(TAG, "loss", loss_sum, "counts", avc)


if __name__ == "__main__":
    main()
