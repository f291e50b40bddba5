#!/usr/bin/env python3
"""The three arithmetic modes side by side (fp32 / bf16x3 / bf16) on one training configuration:

    python scripts/bench_precision.py --config cfg2 --steps 20 --warmup 5 [--out profiles/r04_precision_cfg2.json]

Each mode runs in a fresh child process under its own time limit; the parent stops at the first non-zero exit.  Per mode
one JSON line: clouds/s and ms/step (a plain timed region, the board power and shader clock sampled read-only during it),
then the split-GEMM time per step from HIP events around every ops.gemm_split / ops.gemm_split_tn call of a second timed
region, and the executed MFMA rate of those GEMMs: 2*M*N*K FLOP per product, times the MFMAs issued per product (1 in
bf16, 3 in bf16x3).  fp32 has no split GEMMs (its GEMMs run on the fp32 MFMA).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wireframe-3d-prediction_amd")
CONFIGS = {"cfg1": (8, 4096, 64), "cfg2": (32, 4096, 64), "cfg5": (32, 4096, 256)}
MODES = ("fp32", "bf16x3", "bf16")


def child(mode, cfg, steps, warmup):
    sys.path.insert(0, PKG)
    import torch
    from wf3d import config, ops, telemetry
    import wf3d.functional as F
    from models.PointCloudToWireframe import PointCloudToWireframe
    config.set_precision(mode)
    dev = torch.device("cuda:0")
    B, N, V = CONFIGS[cfg]
    torch.manual_seed(0)
    model = PointCloudToWireframe(input_dim=8, max_vertices=V).to(dev)
    model.vertex_predictor.ensure_point_pool_proj(1024, dev)
    model.set_dropout(0.1)
    model.train()
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, N, 8, generator=g, device=dev)
    counts = torch.full((B,), V, dtype=torch.long, device=dev)

    def step():
        model.zero_grad(set_to_none=True)
        out = model(x, counts)
        (out["vertices"].sum() + out["existence_probabilities"].sum() + out["edge_probs"].sum()).backward()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    hw = telemetry.hwmon_dir(0)
    with telemetry.Sampler(hw) as smp:
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    res = {"config": cfg, "precision": mode, "B": B, "N": N, "V": V, "steps": steps,
           "value": B * steps / dt, "unit": "clouds/s", "ms_per_step": 1e3 * dt / steps,
           "board_w": smp.watts, "shader_ghz": smp.ghz, "cap_w": telemetry.power_cap_watts(hw)}

    # second region: every split GEMM between HIP events (the events add no synchronisation)
    rec = []

    def wrap(name, tn):
        f = getattr(ops, name)

        def g_(a_s, b_s, *a, products=3, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = f(a_s, b_s, *a, products=products, **k)
            e1.record()
            if tn:
                K, Mo = a_s.shape
                n_out = b_s.shape[1]
                flop = 2.0 * K * Mo * n_out
            else:
                flop = 2.0 * a_s.shape[0] * b_s.shape[0] * a_s.shape[1]
            rec.append((e0, e1, flop, products))
            return r
        setattr(ops, name, g_)
        setattr(F.ops, name, g_)
    wrap("gemm_split", False)
    wrap("gemm_split_tn", True)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = sum(a.elapsed_time(b) for a, b, _, _ in rec)
    prods = {p for _, _, _, p in rec}
    res["split_gemm_calls_per_step"] = len(rec) / steps
    res["split_gemm_ms_per_step"] = ms / steps
    res["products_per_mfma_product"] = sorted(prods)
    flop = sum(f for _, _, f, _ in rec)
    mfma_flop = sum(f * p for _, _, f, p in rec)
    res["split_gemm_tflops_math"] = flop / (ms * 1e-3) / 1e12 if ms > 0 else None
    res["split_gemm_tflops_mfma_executed"] = mfma_flop / (ms * 1e-3) / 1e12 if ms > 0 else None
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2", choices=sorted(CONFIGS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--timeout", type=int, default=600, help="seconds per mode")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.config, a.steps, a.warmup)
        return 0
    lines = []
    for mode in a.modes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--config", a.config,
               "--steps", str(a.steps), "--warmup", str(a.warmup)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"{mode}: timed out after {a.timeout} s", file=sys.stderr)
            return 124
        if r.returncode != 0:
            print(f"{mode}: exit {r.returncode}\n{r.stderr[-3000:]}", file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):]
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
