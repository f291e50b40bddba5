"""Times ops.attn_fwd + ops.attn_bwd (--E 512 --heads 8 by default, B = 32) per kernel family.  Head width 64: the key-tiled
MFMA kernels against the parent dispatch (wf3d_set_option "attn_tiled" = 0: chunked VALU kernels beyond 256 vertices) and
against the resident MFMA kernels where both apply.  Other widths (--E 1024 --heads 8, --E 768 --heads 8): the key-tiled
kernels against the VALU kernels (option 0) at 64 and 128 vertices, where the VALU kernels' operands fit the LDS, and
alone at 256 and 512.  Device events, median over --iters calls after --warmup; the arms alternate per repeat, so the
spread between two runs of the same arm is in the output.  One JSON line per (shape, arm, repeat).

    python scripts/bench_attn.py [--E 512] [--heads 8] [--iters 50] [--warmup 10] [--repeats 2] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wireframe-3d-prediction_amd"))

B = 32
PEAK_TF = 157.3                       # fp32 MFMA


def flops(counts, E, HEADS):
    """MFMA work of the algorithm: forward 2 contractions, backward 5 + the recomputed S in both sweeps = 7; 2*n*n*head_dim
    each (the live head_dim E / heads: the zero columns a padded width adds are not counted)."""
    per = sum(2.0 * n * n * (E // HEADS) for n in counts) * HEADS
    return 2 * per, 7 * per


def time_arm(ops, lib, option, counts, iters, warmup, E, HEADS):
    assert lib.wf3d_set_option(b"attn_tiled", option) == 0
    try:
        dev = torch.device("cuda:0")
        meta = ops.EdgeMeta.get(counts, dev)
        g = torch.Generator().manual_seed(0)
        qkv = torch.randn(meta.Rv, 3 * E, generator=g).to(dev)
        dctx = torch.randn(meta.Rv, E, generator=g).to(dev)
        family = ops.attn_kernel(E, HEADS, max(counts))
        tf, tb = [], []
        for it in range(warmup + iters):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            ctx, lse = ops.attn_fwd(qkv, meta, E, HEADS, 0.1, 7)
            e[1].record()
            ops.attn_bwd(qkv, dctx, ctx, lse, meta, E, HEADS, 0.1, 7)
            e[2].record()
            torch.cuda.synchronize()
            if it >= warmup:
                tf.append(e[0].elapsed_time(e[1]))
                tb.append(e[1].elapsed_time(e[2]))
        return family, statistics.median(tf), statistics.median(tb)
    finally:
        lib.wf3d_set_option(b"attn_tiled", 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, default=512)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn: needs a GPU")
    from wf3d import _lib, ops
    lib = _lib.load()
    ragged = [4 + (i * 508) // (B - 1) for i in range(B)]
    E, HEADS = a.E, a.heads
    if E % HEADS:
        raise SystemExit("bench_attn: --E must be a multiple of --heads")
    if E // HEADS == 64:
        shapes = [("all512", [512] * B, (0, 1)), ("all1024", [1024] * B, (0, 1)), ("ragged4..512", ragged, (0, 1)),
                  ("all256", [256] * B, (1, 2))]
    else:
        shapes = [("all64", [64] * B, (0, 1)), ("all128", [128] * B, (0, 1)), ("all256", [256] * B, (1,)),
                  ("all512", [512] * B, (1,))]
    lines = []
    for name, counts, arms in shapes:
        ff, fb = flops(counts, E, HEADS)
        for rep in range(a.repeats):
            for option in arms:
                fam, mf, mb = time_arm(ops, lib, option, counts, a.iters, a.warmup, E, HEADS)
                rec = {"E": E, "heads": HEADS, "shape": name, "attn_tiled": option, "family": fam, "repeat": rep, "fwd_ms": round(mf, 4),
                       "bwd_ms": round(mb, 4), "fwd_bwd_ms": round(mf + mb, 4), "fwd_tflops": round(ff / mf / 1e9, 2),
                       "bwd_tflops": round(fb / mb / 1e9, 2), "peak_tflops": PEAK_TF, "iters": a.iters}
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
