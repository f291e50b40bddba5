"""The drop-in eval.ap_calculator against the reference's own file on random and degenerate batches, against results
recorded from the reference (tests/golden/refcheck_eval.npz, tests/golden/make_golden_refcheck.py)."""
import contextlib
import copy
import importlib.util
import io
import os

import numpy as np

import helpers as H
import refcases


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_ap_calculator_equals_the_reference_on_random_and_degenerate_batches():
    gold = H.load_golden("refcheck_eval")
    mine = load("my_ap", os.path.join(H.PKG, "eval", "ap_calculator.py"))
    rng = np.random.RandomState(3)
    computed = 0
    for t, thr in enumerate(refcases.EVAL_THRESHOLDS):
        calc = mine.APCalculator(distance_thresh=thr)
        for c, case in enumerate(refcases.EVAL_CASES):
            batch = refcases.eval_sample(rng, *case)
            assert refcases.eval_batch_digest(batch) == gold[f"t{t}.c{c}.batch"], (thr, case)
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    calc.compute_metrics(copy.deepcopy(batch))          # it overwrites matched predicted edges in place
                err = ""
            except Exception as e:                                      # no edge within the radius: numpy refuses min() of nothing
                err = type(e).__name__
            assert err == str(gold[f"t{t}.c{c}.error"]), (thr, case, err)
            computed += err == ""
            for k, want in zip(refcases.EVAL_KEYS, gold[f"t{t}.c{c}.ap"]):
                assert np.isclose(want, float(calc.ap_dict[k]), rtol=1e-9, atol=1e-9), (thr, case, k, want, calc.ap_dict[k])
        with contextlib.redirect_stdout(io.StringIO()):
            calc.output_accuracy()
        for k, want in zip(refcases.EVAL_ACCURACY_KEYS, gold[f"t{t}.accuracy"]):
            assert np.isclose(want, float(calc.ap_dict[k]), rtol=1e-9, atol=1e-12), (thr, k)
    p, t = rng.normal(0, 3, (40, 2, 3)), rng.normal(0, 3, (9, 2, 3))
    assert [refcases.digest(p), refcases.digest(t)] == list(gold["hausdorff.inputs"])
    assert np.allclose(gold["hausdorff"], mine.hausdorff_distance_line(p, t), rtol=1e-12, atol=1e-12)
    assert computed >= 8, computed            # most cases go all the way through
