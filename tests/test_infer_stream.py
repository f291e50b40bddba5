"""The forward-only encoder's host side without a GPU: the block plan, the settings, and the numpy model of the
streaming pool (tests/infer_model.py) that tests/test_infer_stream_gpu.py holds the kernel to."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H  # noqa: F401  (puts the package on sys.path)
import infer_model as IM


# ----------------------------------------------------------------------------------------------------------------------
# block_plan
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total, rows", [(5, 64), (63, 64), (64, 64), (65, 64), (200, 64), (1000, 256), (33, 8), (8, 8),
                                         (7, 8), (376, 1000), (376, 24)])
def test_block_plan_covers_every_row_once_in_order(total, rows):
    from wf3d.infer import block_plan
    plan = block_plan(total, rows)
    assert plan[0][0] == 0
    assert all(0 < n <= rows for _, n in plan)
    assert all(n == rows for _, n in plan[:-1])                          # only the last block is short
    assert all(a + n == b for (a, n), (b, _) in zip(plan, plan[1:]))     # in order, no gap, no overlap
    assert plan[-1][0] + plan[-1][1] == total
    assert len(plan) == -(-total // rows)
    assert all(r0 % 8 == 0 for r0, _ in plan)


def test_block_plan_of_no_rows_is_empty():
    from wf3d.infer import block_plan
    assert block_plan(0, 64) == []


def test_block_plan_default_height_is_the_setting():
    from wf3d import config
    from wf3d.infer import block_plan
    assert config.INFER_ROWS > 0 and config.INFER_ROWS % 256 == 0
    assert block_plan(config.INFER_ROWS + 8) == [(0, config.INFER_ROWS), (config.INFER_ROWS, 8)]
    old = config.INFER_ROWS
    try:
        config.INFER_ROWS = 16
        assert block_plan(40) == [(0, 16), (16, 16), (32, 8)]
    finally:
        config.INFER_ROWS = old


@pytest.mark.parametrize("rows", [0, -8, 4, 12, 257, 8.0, "8", True])
def test_block_plan_refuses_a_height_that_is_no_positive_multiple_of_8(rows):
    from wf3d.infer import block_plan
    with pytest.raises(ValueError, match="multiple of 8"):
        block_plan(100, rows)


@pytest.mark.parametrize("total", [-1, 2.5, None])
def test_block_plan_refuses_a_bad_total(total):
    from wf3d.infer import block_plan
    with pytest.raises(ValueError, match="total_rows"):
        block_plan(total, 8)


# ----------------------------------------------------------------------------------------------------------------------
# settings
# ----------------------------------------------------------------------------------------------------------------------
def test_set_inference_validates_and_defaults_to_train():
    from wf3d import config
    old = config.inference()
    try:
        config.set_inference("stream")
        assert config.inference() == "stream"
        config.set_inference("train")
        assert config.inference() == "train"
        for bad in ("eval", "", None, "Stream"):
            with pytest.raises(ValueError, match="'train' or 'stream'"):
                config.set_inference(bad)
        assert config.inference() == "train"
    finally:
        config.set_inference(old)


def _config_in_child(value):
    env = {k: v for k, v in os.environ.items() if k != "WF3D_INFERENCE"}
    if value is not None:
        env["WF3D_INFERENCE"] = value
    code = f"import sys; sys.path.insert(0, {H.PKG!r}); from wf3d import config; print(config.inference())"
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)


def test_environment_override_is_validated():
    """WF3D_INFERENCE is read when wf3d.config is imported, as WF3D_PRECISION is: one child process per value."""
    assert _config_in_child(None).stdout.strip() == "train"
    assert _config_in_child("stream").stdout.strip() == "stream"
    bad = _config_in_child("fast")
    assert bad.returncode != 0 and "WF3D_INFERENCE='fast'" in bad.stderr


def test_cpu_tensors_are_refused():
    import torch
    from models.PointNetEncoder import PointNetEncoder
    enc = PointNetEncoder(8, [64], 40)
    with pytest.raises(RuntimeError, match="needs CUDA"):
        enc.encode_stream(torch.zeros(2, 16, 8))
    with pytest.raises(RuntimeError, match="needs CUDA"):
        enc.encode_packed_stream(torch.zeros(24, 8), [16, 8])


# ----------------------------------------------------------------------------------------------------------------------
# the numpy model of the streaming fold
# ----------------------------------------------------------------------------------------------------------------------
# offsets, and the clouds whose rows are all invalid.  Every set has a cloud of no rows and a cloud with no valid row.
MODEL_CASES = {
    "issue": ([0, 37, 37, 100, 356], [2]),
    "empty-first-and-last": ([0, 0, 50, 51, 51], [2]),
    "one-row-clouds": ([0, 1, 2, 2, 3, 40], [1, 3]),
}


def model_inputs(offsets, dead, C, seed, pad=20):
    rng = np.random.default_rng(seed)
    R = offsets[-1] + pad
    pf = rng.standard_normal((R, C))
    pf[:, 0] = -1.0 - np.abs(pf[:, 0])          # negative everywhere: a maximum that starts from 0 would be wrong
    pf[:, 1] = 0.75                             # constant
    valid = np.ones(R)
    valid[rng.random(R) < 0.3] = 0.0
    for b in dead:
        valid[offsets[b]:offsets[b + 1]] = 0.0
    pf[offsets[-1]:] = 1e6                      # the rows behind the clouds must reach no pool
    return pf, valid


@pytest.mark.parametrize("case", sorted(MODEL_CASES))
def test_model_equals_the_direct_pools_for_random_cuts(case):
    offsets, dead = MODEL_CASES[case]
    pf, valid = model_inputs(offsets, dead, 6, seed=len(case))
    want = IM.direct(offsets, pf, valid)
    R = pf.shape[0]
    rng = np.random.default_rng(3)
    cut_sets = [[0, R], list(range(0, R, 8)) + [R], list(range(R + 1))]
    cut_sets += [[0] + sorted(rng.choice(np.arange(1, R), size=k, replace=False).tolist()) + [R] for k in (1, 3, 9, 17)]
    for cuts in cut_sets:
        got = IM.stream(offsets, pf, valid, cuts)
        for k in ("cnt", "nvalid"):
            assert np.array_equal(got[k], want[k]), (case, k)
        C = pf.shape[1]
        assert np.array_equal(got["masked"][:, :C], want["masked"][:, :C]), (case, "masked max")
        assert np.array_equal(got["unmasked"][:, C:], want["unmasked"][:, C:]), (case, "unmasked max")
        assert np.allclose(got["masked"][:, C:], want["masked"][:, C:], rtol=1e-13, atol=1e-13), (case, "masked mean")
        assert np.allclose(got["unmasked"][:, :C], want["unmasked"][:, :C], rtol=1e-13, atol=1e-13), (case, "unmasked mean")


def test_model_degenerate_clouds():
    offsets, dead = MODEL_CASES["issue"]
    pf, valid = model_inputs(offsets, dead, 4, seed=1)
    got = IM.stream(offsets, pf, valid, [0, 100, pf.shape[0]])
    assert not got["masked"][1].any() and not got["unmasked"][1].any()          # the cloud of no rows: zeros
    assert got["cnt"][1] == 1 and got["nvalid"][1] == 0
    assert not got["masked"][2].any() and got["unmasked"][2].any()              # no valid row: masked pools 0, unmasked live
    assert got["cnt"][2] == 1 and got["nvalid"][2] == 0
    assert (got["masked"][0, 0] < 0) and (got["unmasked"][0, 4] < 0)            # the negative channel's maxima
    assert np.abs(got["masked"]).max() < 1e3 and np.abs(got["unmasked"]).max() < 1e3   # no pad row was pooled
