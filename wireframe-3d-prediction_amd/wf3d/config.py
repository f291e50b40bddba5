"""Run-time configuration of the HIP path.

precision
    "bf16x3" (default): the large per-point Linear layers (rows >= SPLIT_MIN_ROWS) run as
             split-precision GEMMs — fp32 operands split into bf16 high + low parts, three
             bf16 MFMAs per product, fp32 accumulation: results agree with the fp32 path to
             ~1e-5 (inside the 1e-4 parity gate) at ~3x the fp32-MFMA throughput.
    "fp32":  every GEMM on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32).
    "bf16":  opt-in.  Exactly the GEMMs "bf16x3" runs split, on the same sx8 operands, with ONE bf16 MFMA per
             product (hi*hi: bf16 round-to-nearest operands, fp32 accumulation; wf3d_gemm_bf16 / _tn).
             Everything else stays as in "bf16x3".  Narrower than fp32: its error is measured and gated
             (tests/test_precision_bf16_gpu.py).
Environment override: WF3D_PRECISION.

dropout_rng
    "host" (default): each train-mode edge-head forward draws its dropout seed from torch's CPU generator and hands it
             to the mask kernels by value.  A captured graph replays that one seed: the same masks on every replay.
    "device": the seed words are drawn on the device (wf3d.random: one draw kernel per forward, state in device
             memory) and the mask kernels load them at run time, so every replay of a captured training step draws
             fresh masks.
Environment override: WF3D_DROPOUT_RNG.

inference
    "train" (default): a forward under torch.no_grad() is the training forward, which keeps every layer's activations
             until it returns.
    "stream": with grad mode off, the encoder stage of PointNetEncoder.forward and PointCloudToWireframe.forward /
             forward_packed takes the forward-only path (wf3d.infer): the per-point MLP walks the rows in blocks of
             INFER_ROWS, keeps nothing for a backward and pools the blocks as they pass.  With grad mode on nothing
             changes; the module's train() / eval() mode does not enter the decision.
Environment override: WF3D_INFERENCE.

edge_inference
    "train" (default): the edge head's forward under torch.no_grad() is EdgeFn's, which holds every edge-row tensor
             (4,608 B per edge row at hidden_dim = 512) until it returns.
    "stream": with grad mode off and no dropout probability active (eval(), or set_dropout(0)), EdgePredictor.forward /
             forward_ragged / forward_padded take the forward-only path (wf3d.infer.edge_stream): the edge rows are walked
             in blocks of INFER_EDGE_ROWS and nothing per edge row outlives its block.  With grad mode on, or with dropout
             active, nothing changes.  A setting of its own: "inference" above keeps meaning the encoder stage alone.
Environment override: WF3D_EDGE_INFERENCE.
"""
import os

SPLIT_MIN_ROWS = 1024
PRECISIONS = ("fp32", "bf16x3", "bf16")
_precision = os.environ.get("WF3D_PRECISION", "bf16x3")
if _precision not in PRECISIONS:
    raise RuntimeError(f"WF3D_PRECISION={_precision!r}: expected 'fp32', 'bf16x3' or 'bf16'")


DROPOUT_RNGS = ("host", "device")
_dropout_rng = os.environ.get("WF3D_DROPOUT_RNG", "host")
if _dropout_rng not in DROPOUT_RNGS:
    raise RuntimeError(f"WF3D_DROPOUT_RNG={_dropout_rng!r}: expected 'host' or 'device'")


def dropout_rng():
    return _dropout_rng


def set_dropout_rng(src):
    global _dropout_rng
    if src not in DROPOUT_RNGS:
        raise ValueError("dropout_rng must be 'host' or 'device'")
    _dropout_rng = src


INFERENCES = ("train", "stream")
_inference = os.environ.get("WF3D_INFERENCE", "train")
if _inference not in INFERENCES:
    raise RuntimeError(f"WF3D_INFERENCE={_inference!r}: expected 'train' or 'stream'")

# Rows per block of the forward-only encoder (a positive multiple of 8; wf3d.infer.block_plan).  Chosen by measurement
# ("Forward only"): the fastest fixed height of the sweep 4096 .. 32768 at cfg2 and at cfg4, 6 - 7 %
# behind the training forward at 1/7 of its peak memory.  8192 rows (z plus h of the 2048-wide layer = 128 MiB, half of
# the Infinity Cache) measured 42 % behind: per block, the GEMMs have too few tiles and the host too many launches.
INFER_ROWS = 32768


EDGE_INFERENCES = ("train", "stream")
_edge_inference = os.environ.get("WF3D_EDGE_INFERENCE", "train")
if _edge_inference not in EDGE_INFERENCES:
    raise RuntimeError(f"WF3D_EDGE_INFERENCE={_edge_inference!r}: expected 'train' or 'stream'")

# Edge rows per block of the forward-only edge head (a positive multiple of 256, the extent of a live-row count;
# wf3d.infer.edge_stream).  Chosen by measurement ("Forward only, edge head";
# profiles/r12_edge_inference.jsonl): the fastest fixed height of the sweep 8192 .. 131072 at the edge shapes of cfg2
# (64,512 rows: one block, 4 % ahead of the training forward) and of cfg5 (1,044,480 rows: 3.25 ms against 3.05 / 3.13 ms).
# At cfg5 NO height matches the training forward within its run-to-run spread (2.7 %): this one is 4 - 7 % behind it at
# 1/7.7 of its peak memory (648 MB against 5.0 GB), so the path ships on footprint.  Smaller blocks cost host time, not
# GPU time: five launches per block at ~16 us each (65536: +8 %, 1/14.5; 32768: +40 %, 1/26; 8192: 3.4 x the time).
INFER_EDGE_ROWS = 131072


def edge_inference():
    return _edge_inference


def set_edge_inference(mode):
    global _edge_inference
    if mode not in EDGE_INFERENCES:
        raise ValueError("edge_inference must be 'train' or 'stream'")
    _edge_inference = mode


def inference():
    return _inference


def set_inference(mode):
    global _inference
    if mode not in INFERENCES:
        raise ValueError("inference must be 'train' or 'stream'")
    _inference = mode


def precision():
    return _precision


def set_precision(p):
    global _precision
    if p not in PRECISIONS:
        raise ValueError("precision must be 'fp32', 'bf16x3' or 'bf16'")
    _precision = p


# Edge head, bf16x3 mode: the per-vertex Linears (embed, in_proj, out_proj, Pa / Pb: sum-of-counts rows, 14 GFLOP per
# cfg2 step) stay on the exact-fp32 MFMA.  Round 2 ran them on bf16x3 through the general GEMM's x3 staging (0.4 % of
# the step faster); the production-selection frozen-gradient test (tests/test_frozen_grad_gpu.py) then measured 3.2e-4
# on attention.in_proj_weight against 1.7e-4 with fp32 here — the 2e-4 bound on every gradient element is worth more.
# WF3D_EDGE_X3=1 restores the x3 path (kept and tested: tests/test_kernels_gpu.py::test_gemm_x3_layouts).
EDGE_X3 = os.environ.get("WF3D_EDGE_X3", "0") != "0"

# The stages release their saved activations (2.7 GB at cfg2) at the end of their backward, so a second backward through
# the same graph (retain_graph=True, which the reference's autograd serves) raises.  RETAIN_SAVED = True keeps them
# until the graph itself is freed.
RETAIN_SAVED = os.environ.get("WF3D_RETAIN_SAVED", "0") != "0"
