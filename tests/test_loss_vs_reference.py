"""The CPU loss oracle (oracle/loss_cpu.py) against the reference's own losses/WireframeLoss.py at the shapes the device-loss
sweep uses (tests/test_loss.py::test_device_loss_matches_the_cpu_oracle_at_other_shapes) — values and input gradients,
against results recorded from the reference (tests/golden/refcheck_loss.npz, tests/golden/make_golden_refcheck.py)."""
import contextlib
import io

import helpers as H
import refcases
from oracle import loss_cpu
from refsummary import digest, violations


def test_loss_oracle_equals_the_reference_at_the_sweep_shapes():
    gold = H.load_golden("refcheck_loss")
    for i, shape in enumerate(refcases.LOSS_SHAPES):
        key = f"case{i}"
        p, tg = refcases.loss_inputs(*shape)
        assert [digest(t) for t in list(p.values()) + list(tg.values())] == list(gold[key + ".inputs"]), shape
        p = {k: v.clone().requires_grad_() for k, v in p.items()}
        with contextlib.redirect_stdout(io.StringIO()):
            out = loss_cpu.wireframe_loss(p, tg, 3.0, 1.5, 1.0)[0]
        out["total_loss"].backward()
        for k in refcases.LOSS_KEYS:
            a = float(gold[f"{key}.{k}"])
            assert abs(a - float(out[k])) <= 1e-6 * max(1.0, abs(a)), (shape[:2], k, a, float(out[k]))
        for k, v in p.items():
            name = f"{key}.grad.{k}"
            if float(gold[name + ".maxabs"]) == 0.0:           # the reference sends no (or an all-zero) gradient here
                assert v.grad is None or float(v.grad.abs().max()) == 0.0, (shape[:2], k)
            else:
                assert v.grad is not None, (shape[:2], k)
                assert violations(gold, name, v.grad, 1e-6, floor=1e-12) == [], (shape[:2], k)
