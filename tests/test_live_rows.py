"""The live-row count of the padded edge head, without a GPU: the C ABI carries the new symbol in the header and in the
library, and the models take tail="compute" | "skip" on the padded layout only."""
import re
import subprocess

import pytest

import helpers as H  # noqa: F401  (sys.path)


def test_symbol_in_header_and_library():
    import os
    from wf3d import _lib
    txt = open(os.path.join(H.ROOT, "include", "wf3d.h")).read()
    assert re.search(r"^int wf3d_set_live_rows\(const int32_t\* rows\);", txt, flags=re.M)
    assert "LIVE ROW COUNT" in txt
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "wf3d_set_live_rows" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    lib = _lib.load()
    assert "wf3d_set_live_rows" in _lib.SIGNATURES
    assert lib.wf3d_set_live_rows(None) == 0                 # clearing needs no device


def test_live_rows_context_rejects_host_tensors():
    import torch
    from wf3d import ops
    with ops.live_rows(None):                                 # no count: nothing to set
        pass
    with pytest.raises(RuntimeError):
        with ops.live_rows(torch.zeros(1, dtype=torch.int32)):
            pass


def test_set_edge_layout_tail_values():
    from models.PointCloudToWireframe import PointCloudToWireframe
    m = PointCloudToWireframe(8, 8)
    assert m._edge_tail == "compute"
    assert m.set_edge_layout("padded") is m and m._edge_tail == "compute"          # the default
    assert m.set_edge_layout("padded", tail="skip")._edge_tail == "skip"
    assert m.set_edge_layout("padded", tail="compute")._edge_tail == "compute"
    m.set_edge_layout("padded", tail="skip")
    assert m.set_edge_layout("padded")._edge_tail == "compute"                     # not sticky: today's path unless asked
    for bad in ("zero", "", "SKIP", 1, True):
        with pytest.raises(ValueError):
            m.set_edge_layout("padded", tail=bad)
    assert m._edge_layout == "padded" and m._edge_tail == "compute"                # a rejected call changes nothing


def test_tail_with_ragged_layout_raises():
    from models.PointCloudToWireframe import PointCloudToWireframe
    m = PointCloudToWireframe(8, 8)
    for t in ("skip", "compute"):
        with pytest.raises(ValueError):
            m.set_edge_layout("ragged", tail=t)
    assert m.set_edge_layout("ragged")._edge_layout == "ragged"


def test_forward_padded_rejects_unknown_tail():
    import inspect

    import torch
    from models.EdgePredictor import EdgePredictor
    assert inspect.signature(EdgePredictor.forward_padded).parameters["tail"].default == "compute"
    ep = EdgePredictor(3, 64, 4)
    with pytest.raises(ValueError):
        ep.forward_padded(torch.zeros(2, 5, 3), torch.tensor([3, 4]), tail="drop")


def test_skip_mode_needs_every_launch_to_honour_the_count():
    """_edge_live: the count is used only when the whole edge-row section runs on kernels that honour it."""
    from types import SimpleNamespace as NS
    from wf3d.functional import Route, _edge_live
    split = (Route("split", "tn", "split"), Route("split", "tn_t", "split"))
    live = object()
    meta = NS(padded=True, tail="skip", live=live)
    assert _edge_live(meta, split, True) is live
    assert _edge_live(meta, split, False) is None
    assert _edge_live(NS(padded=True, tail="compute", live=live), split, True) is None
    assert _edge_live(NS(padded=False, tail="compute", live=None), split, True) is None
    fp32 = (Route("fp32", "fp32", "fp32"),) * 2
    assert _edge_live(meta, fp32, True) is None
    assert _edge_live(meta, (split[0], Route("split", "transposes", "split")), True) is live      # sx8 operands too
    assert _edge_live(meta, (split[0], Route("split", "fp32", "split")), True) is None             # an fp32 route: no count
