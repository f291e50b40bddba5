"""The forward-only edge head's host side without a GPU: the settings, the refusals, and the numpy statement of the block
walk (tests/infer_edge_model.py) that tests/test_infer_edge_stream_gpu.py holds the kernels to."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H  # noqa: F401  (puts the package on sys.path)
import infer_edge_model as EM


# ----------------------------------------------------------------------------------------------------------------------
# settings
# ----------------------------------------------------------------------------------------------------------------------
def test_set_edge_inference_validates_and_defaults_to_train():
    from wf3d import config
    assert config.EDGE_INFERENCES == ("train", "stream")
    old = config.edge_inference()
    try:
        config.set_edge_inference("stream")
        assert config.edge_inference() == "stream"
        config.set_edge_inference("train")
        assert config.edge_inference() == "train"
        for bad in ("eval", "", None, "Stream"):
            with pytest.raises(ValueError, match="'train' or 'stream'"):
                config.set_edge_inference(bad)
        assert config.edge_inference() == "train"
    finally:
        config.set_edge_inference(old)


def test_the_encoder_setting_does_not_move_the_edge_setting():
    from wf3d import config
    old = (config.inference(), config.edge_inference())
    try:
        config.set_edge_inference("train")
        config.set_inference("stream")
        assert config.edge_inference() == "train"
        config.set_inference("train")
        config.set_edge_inference("stream")
        assert config.inference() == "train"
    finally:
        config.set_inference(old[0])
        config.set_edge_inference(old[1])


def _config_in_child(value):
    env = {k: v for k, v in os.environ.items() if k not in ("WF3D_EDGE_INFERENCE", "WF3D_INFERENCE")}
    if value is not None:
        env["WF3D_EDGE_INFERENCE"] = value
    code = (f"import sys; sys.path.insert(0, {H.PKG!r}); from wf3d import config; "
            "print(config.edge_inference(), config.inference())")
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)


def test_environment_override_is_validated():
    """WF3D_EDGE_INFERENCE is read when wf3d.config is imported, as WF3D_INFERENCE is: one child process per value."""
    assert _config_in_child(None).stdout.split() == ["train", "train"]
    assert _config_in_child("stream").stdout.split() == ["stream", "train"]
    bad = _config_in_child("fast")
    assert bad.returncode != 0 and "WF3D_EDGE_INFERENCE='fast'" in bad.stderr


def test_default_block_height_is_a_positive_multiple_of_256():
    from wf3d import config
    assert isinstance(config.INFER_EDGE_ROWS, int) and config.INFER_EDGE_ROWS > 0 and config.INFER_EDGE_ROWS % 256 == 0


# ----------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    import torch
    from models.EdgePredictor import EdgePredictor
    from wf3d import infer
    ep = EdgePredictor(3, 64, 2).eval()
    with pytest.raises(RuntimeError, match="needs CUDA"):
        infer.edge_stream(torch.zeros(2, 5, 3), None, 2, "bf16x3", ep._param_list(), rows=8)
    with pytest.raises(RuntimeError, match="needs CUDA"):
        ep.forward_stream(torch.zeros(2, 5, 3), [5, 3])
    with pytest.raises(RuntimeError, match="needs CUDA"):
        ep.forward_stream(torch.zeros(2, 5, 3), torch.tensor([5, 3]))


def test_forward_stream_refuses_active_dropout_and_bad_arguments():
    import torch
    from models.EdgePredictor import EdgePredictor
    ep = EdgePredictor(3, 64, 2)
    v = torch.zeros(2, 5, 3)
    ep.train()
    with pytest.raises(ValueError, match="no dropout"):
        ep.forward_stream(v, [5, 3])
    with pytest.raises(ValueError, match="no dropout"):
        ep.forward_stream(v, torch.tensor([5, 3]))
    ep.eval()
    with pytest.raises(ValueError, match="3 counts for a batch of 2"):
        ep.forward_stream(v, [5, 3, 2])
    with pytest.raises(IndexError, match="too many indices"):            # the ragged layout's check stays
        ep.forward_stream(v, [5, 1])
    with pytest.raises(ValueError, match="tail must be"):
        ep.forward_stream(v, torch.tensor([5, 3]), tail="drop")
    with pytest.raises(ValueError, match="must be integers"):
        ep.forward_stream(v, torch.tensor([5.0, 3.0]))
    with pytest.raises(ValueError, match="1-D tensor of 2 counts"):
        ep.forward_stream(v, torch.tensor([5, 3, 2]))


@pytest.mark.parametrize("rows", [0, -8, 12, 8.0, True])
def test_a_height_that_is_no_positive_multiple_of_8_is_refused(rows):
    import torch
    from wf3d import infer

    class OnDevice:                     # is_cuda is all the check before the height reads
        is_cuda = True
    with pytest.raises(ValueError, match="multiple of 8"):
        infer.edge_stream(OnDevice(), None, 2, "bf16x3", [torch.zeros(1)] * 24, rows=rows)


# ----------------------------------------------------------------------------------------------------------------------
# the numpy model: block_live and "global edge row -> (sample, i, j)"
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows, Re", [(8, 50), (16, 144), (24, 144), (256, 1000), (64, 64), (4096, 144)])
def test_block_live_model(rows, Re):
    from wf3d.infer import block_plan
    plan = block_plan(Re, rows)
    for total in (0, 1, rows - 1, rows, rows + 1, Re - 1, Re, Re + 5, -3):
        bl = EM.block_live(total, rows, Re, len(plan))
        assert bl.dtype == np.int32 and bl.shape == (len(plan),)
        live = min(max(total, 0), Re)
        assert int(bl.sum()) == live                                       # the blocks' counts add up to the live total
        for k, (e0, n) in enumerate(plan):
            assert bl[k] == len([e for e in range(e0, e0 + n) if e < live])
        assert np.all(np.diff(bl) <= 0)                                    # full blocks, one partial block, empty blocks
    assert EM.block_live(5, rows, Re, len(plan) + 2)[-2:].tolist() == [0, 0]     # blocks past Re are empty, never negative


COUNTS = [[5, 2, 9, 3], [5, 0, 1, 9], [2], [0, 0], [1, 3, 1], [7, 4], [12, 2, 7]]


@pytest.mark.parametrize("counts", COUNTS)
def test_edge_row_model_equals_edge_index_lists(counts):
    """Row e of the compact layout is pair e - eoff[s] of sample s's list, for ragged counts including 0 and 1."""
    from wf3d.functional import edge_index_lists
    lists = edge_index_lists(counts)
    want = [(s, i, j) for s, lst in enumerate(lists) for i, j in lst]
    eoff = EM.edge_offsets(counts)
    assert eoff[-1] == len(want) and eoff.tolist() == np.cumsum([0] + [len(l) for l in lists]).tolist()
    assert [EM.edge_row(counts, e) for e in range(len(want))] == want
    assert EM.edge_row(counts, len(want)) is None and EM.edge_row(counts, -1) is None


def test_block_rows_cut_samples_anywhere():
    """The rows of the blocks of a walk, concatenated, are the rows of the layout: a block that starts inside a sample
    continues the sample's pairs where the last one stopped; rows past the live total are None."""
    from wf3d.infer import block_plan
    counts = [5, 2, 9, 3]
    total = int(EM.edge_offsets(counts)[-1])
    assert total == 50
    whole = EM.block_rows(counts, 0, total + 6)
    assert whole[total:] == [None] * 6
    for rows in (8, 16, 24, 56):
        got = [r for e0, n in block_plan(total + 6, rows) for r in EM.block_rows(counts, e0, n)]
        assert got == whole
    assert EM.block_rows(counts, 8, 4) == [(0, 2, 4), (0, 3, 4), (1, 0, 1), (2, 0, 1)]     # sample 0 ends, 1 passes, 2 starts
