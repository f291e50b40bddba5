"""CPU-side checks of the capturable training step: the WF3D_DROPOUT_RNG switch, ClipAdam's `capturable` argument, and
the C ABI of the device dropout seeds and the capturable optimizer step (tests/test_graph_step_gpu.py runs them)."""
import os
import subprocess
import sys

import pytest
import torch

import helpers as H


def _config_in_child(value):
    env = dict(os.environ)
    env.pop("WF3D_DROPOUT_RNG", None)
    if value is not None:
        env["WF3D_DROPOUT_RNG"] = value
    code = "from wf3d import config; print(config.dropout_rng())"
    return subprocess.run([sys.executable, "-c", code], cwd=H.PKG, env=env, capture_output=True, text=True)


@pytest.mark.parametrize("value,want", [(None, "host"), ("host", "host"), ("device", "device")])
def test_dropout_rng_environment(value, want):
    r = _config_in_child(value)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == want


@pytest.mark.parametrize("value", ["Device", "cuda", "", "1"])
def test_dropout_rng_environment_rejects(value):
    r = _config_in_child(value)
    assert r.returncode != 0
    assert "WF3D_DROPOUT_RNG" in r.stderr


def test_set_dropout_rng_validates():
    from wf3d import config
    old = config.dropout_rng()
    try:
        config.set_dropout_rng("device")
        assert config.dropout_rng() == "device"
        config.set_dropout_rng("host")
        assert config.dropout_rng() == "host"
        with pytest.raises(ValueError, match="dropout_rng"):
            config.set_dropout_rng("gpu")
        assert config.dropout_rng() == "host"
    finally:
        config.set_dropout_rng(old)


def test_clip_adam_capturable_argument():
    from wf3d.optim import ClipAdam
    ps = [torch.nn.Parameter(torch.zeros(3))]
    assert ClipAdam(ps).capturable is False
    opt = ClipAdam(ps, capturable=True)
    assert opt.capturable is True and opt.param_groups[0]["capturable"] is True
    assert ClipAdam(ps, lr=torch.tensor(1e-3), capturable=True).param_groups[0]["lr"].dim() == 0
    with pytest.raises(TypeError, match="capturable"):
        ClipAdam(ps, capturable="yes")
    with pytest.raises(ValueError, match="capturable=True"):
        ClipAdam(ps, lr=torch.tensor(1e-3))
    with pytest.raises(ValueError, match="0-d fp32"):
        ClipAdam(ps, lr=torch.tensor([1e-3]), capturable=True)
    with pytest.raises(ValueError, match="hyper-parameters"):
        ClipAdam(ps, lr=torch.tensor(-1.0), capturable=True)


def test_clip_adam_state_dict_keeps_its_own_capturable():
    """A state_dict saved by torch.optim.Adam carries its own "capturable": loading it does not switch the mode."""
    from wf3d.optim import ClipAdam
    ps = [torch.nn.Parameter(torch.zeros(3))]
    ref = torch.optim.Adam(ps, capturable=False)
    opt = ClipAdam(ps, capturable=True)
    opt.load_state_dict(ref.state_dict())
    assert opt.param_groups[0]["capturable"] is True


def test_new_symbols_declared_and_bound():
    import re
    from wf3d import _lib
    hdr = open(os.path.join(H.ROOT, "include", "wf3d.h")).read()
    lib = _lib.load()
    for name in ("wf3d_dropout_draw", "wf3d_set_dropout_seed_words", "wf3d_clip_adam_step_dev"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.wf3d_version() == 105


def test_new_entry_points_check_their_arguments():
    """Argument checks only: nothing is launched."""
    from wf3d import _lib
    lib = _lib.load()
    assert lib.wf3d_dropout_draw(None, None, None) == -1 and b"wf3d_dropout_draw" in lib.wf3d_last_error()
    assert lib.wf3d_set_dropout_seed_words(None) == 0
    assert lib.wf3d_clip_adam_step_dev(None, None, None, None, None, None, 1, 1.0, 1e-3, None, 0.9, 0.999, 1e-8, 0.0,
                                       None, 0, None, None) == -1
    assert b"null table" in lib.wf3d_last_error()
