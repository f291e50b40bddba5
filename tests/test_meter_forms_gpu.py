"""wf3d.meter.TrainMeter (meter_update_kernel, csrc/loss.hip) against optim_model.meter64 at the inputs the one test in
tests/test_loss.py leaves out: counts[0] of 0, 1, 7, 86 (3 c = 258: the 256-thread loop takes a second pass) and 300,
a count above min(Vp, Vt) (the clamp), counts=None, predicted and target vertex numbers that differ, predictions as the
[:, :, :3] view of a [B, V, 4] tensor, a ring of 0, 1 and 4 entries over 9 steps, a NaN total loss at step 0 and at
step 3, and loss keys that are missing.

Bounds: the four losses, the best loss and the ring are copies and must be bit-equal (NaN where the model has NaN); both
RMSE fields within 1e-6 relative, and exactly 0 at count 0."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402,F401
import optim_model as OM  # noqa: E402

STEPS = 9


def dev():
    return torch.device("cuda:0")


def _check(meter, s64, capacity, label):
    got = meter.state.cpu().numpy()
    assert got.shape == (8 + capacity,)
    copies = [0, 1, 3, 4, 5, 6] + list(range(8, 8 + capacity))
    assert np.array_equal(got[copies], s64[copies].astype(np.float32), equal_nan=True), (label, got, s64)
    worst = 0.0
    for k in (2, 7):
        if s64[k] == 0.0:
            assert got[k] == 0.0, (label, k)
        else:
            worst = max(worst, abs(float(got[k]) - s64[k]) / s64[k])
    assert worst <= 1e-6, (label, worst)
    return worst


def _run(count0, capacity, *, vp=300, vt=300, nan_steps=(), keys=("vertex_loss", "existence_loss", "edge_loss"), seed=0):
    from wf3d.meter import TrainMeter
    rng = np.random.RandomState(seed)
    B = 2
    meter = TrainMeter(dev(), history=capacity)
    tgt = rng.standard_normal((B, vt, 3)).astype(np.float32)
    tgt_d = torch.from_numpy(tgt).to(dev())
    counts = None if count0 is None else torch.tensor([count0, 5], dtype=torch.int64, device=dev())
    s64 = np.zeros(8 + capacity)
    worst, hist = 0.0, []
    for step in range(STEPS):
        out4 = rng.standard_normal((B, vp, 4)).astype(np.float32)       # `vertices` is a strided view of [B, V, 4] in the model
        vals = {k: np.float32(3.0 - 0.3 * step + rng.random_sample()) for k in ("total_loss",) + tuple(keys)}
        if step in nan_steps:
            vals["total_loss"] = np.float32("nan")
        losses = {k: torch.tensor(v, dtype=torch.float32, device=dev()) for k, v in vals.items()}
        pv = torch.from_numpy(out4).to(dev())[:, :, :3]
        assert pv.stride(1) == 4 and not pv.is_contiguous()
        meter.update(losses, pv, tgt_d, counts)
        s64 = OM.meter64(s64, capacity, vals["total_loss"], vals.get("vertex_loss"), vals.get("existence_loss"),
                         vals.get("edge_loss"), out4[0, :, :3], tgt[0], count0)
        worst = max(worst, _check(meter, s64, capacity, (count0, capacity, step)))
        hist.append(float(vals["total_loss"]))
        m = meter.read()                                                  # read() on the same record, every step
        assert m["steps"] == step + 1
        want = hist[-capacity:] if capacity else []
        assert np.array_equal(np.array(m["loss_history"]), np.array(want), equal_nan=True)
        assert np.array_equal(np.float32([m["total_loss"], m["vertex_loss"], m["existence_loss"], m["edge_loss"]]),
                              s64[3:7].astype(np.float32), equal_nan=True)
    print(f"[meter forms] count0={count0} capacity={capacity} Vp={vp} Vt={vt} nan={nan_steps}: worst RMSE rel err {worst:.2e}")
    return meter, s64


@pytest.mark.parametrize("capacity", [0, 1, 4])
@pytest.mark.parametrize("count0", [0, 1, 7, 86, 300, None])
def test_meter_counts_and_ring_sizes(count0, capacity):
    meter, s64 = _run(count0, capacity, seed=11)
    if count0 == 0:
        assert meter.read()["vertex_rmse"] == 0.0 and meter.read()["best_vertex_rmse"] == 0.0


@pytest.mark.parametrize("vp,vt,count0", [(300, 120, 300), (120, 300, 300), (300, 120, 121), (90, 300, None), (300, 86, None),
                                          (300, 300, 100000), (300, 300, -4)])
def test_meter_clamps_the_count_to_both_vertex_numbers(vp, vt, count0):
    """counts[0] above min(Vp, Vt) (the padded target of another batch, or a corrupt count) reads no vertex past either
    tensor: the RMSE is the one over min(Vp, Vt) vertices; a negative count is 0 vertices."""
    _, s64 = _run(count0, 4, vp=vp, vt=vt, seed=12)
    if count0 is not None and count0 < 0:
        assert s64[7] == 0.0


@pytest.mark.parametrize("nan_steps", [(0,), (3,), (0, 3)])
def test_meter_nan_loss_follows_fminf(nan_steps):
    """A NaN total loss is recorded as the last loss and in the ring; the best loss follows fminf: a NaN first step is
    replaced by the first number, a later NaN never replaces a number."""
    meter, s64 = _run(7, 4, nan_steps=nan_steps, seed=13)
    m = meter.read()
    assert m["best_loss"] == m["best_loss"] and m["best_loss"] == float(np.float32(s64[1]))


@pytest.mark.parametrize("keys", [(), ("edge_loss",), ("vertex_loss", "existence_loss")])
def test_meter_missing_loss_keys_leave_zeros(keys):
    meter, _ = _run(7, 4, keys=keys, seed=14)
    m = meter.read()
    for k in ("vertex_loss", "existence_loss", "edge_loss"):
        assert (m[k] != 0.0) == (k in keys)
