"""tests/lsa_model.py, the numpy model of the device assignment solver (csrc/lsa_solve.h, csrc/loss.hip), held to scipy on the CPU: on
every cost generator of the device tests it returns a permutation of scipy's optimal total.  test_loss_assign_forms_gpu.py
then asks the kernels for the model's assignment element for element, which pins their tie rule as well.

Also the written record of why the kernels sanitise their cost loads: on a matrix with a whole row or column of NaN or
+inf the unsanitised algorithm walks an augmenting path through an entry that no scan wrote (on the device: an endless
walk); after sanitise() it returns a permutation."""
import numpy as np
import pytest
import lsa_cases as K
import lsa_model as M

SIZES = (1, 2, 3, 7, 33, 64, 65, 130)
B = 2


assert_optimal_permutation = K.assert_optimal_permutation


@pytest.mark.parametrize("V", SIZES)
@pytest.mark.parametrize("name", K.SQUARE)
def test_square_model_is_optimal(name, V):
    for C in K.square_costs(name, V, B):
        c4r = M.square(C)
        assert_optimal_permutation(C, c4r, name in K.EXACT)
        if name == "product":
            assert C.astype(np.float64)[np.arange(V), c4r].sum() == K.product_optimum(V)


@pytest.mark.parametrize("V", SIZES)
@pytest.mark.parametrize("name", K.WIREFRAME + ("wf_gauss",))
def test_both_models_are_optimal_on_wireframe_costs(name, V):
    counts = np.array([0, 1, V - 1, V, V + 5, -3], dtype=np.int64)
    cost = K.wireframe_cost(*K.wireframe_inputs(name, V, counts))
    for C, n in zip(cost, counts):
        assert_optimal_permutation(C, M.square(C), name in K.EXACT)
        assert_optimal_permutation(C, M.rect(C, n), name in K.EXACT)
    assert np.array_equal(M.rect(cost[4], V + 5), M.rect(cost[4], V))           # a count above V is V
    assert np.array_equal(M.rect(cost[5], -3), np.arange(V))                    # a negative count is 0: nothing matched


def test_product_matrix_walks_through_every_row():
    """Why the product matrix is in the set: V (V + 1) / 2 path steps, against a few per row on Gaussian costs."""
    V = 65
    C = np.outer(np.arange(V) + 1.0, np.arange(V) + 1.0).astype(np.float32)
    c4r, steps = M.square(C, return_steps=True)
    assert steps == V * (V + 1) // 2
    assert np.array_equal(c4r, np.arange(V)[::-1])
    assert M.square(K.square_costs("gauss", V, 1)[0], return_steps=True)[1] < V * (V + 1) // 8


def test_sanitise():
    f = np.finfo(np.float32)
    x = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.5, -f.max, f.max, f.tiny], dtype=np.float32)
    want = np.array([f.max, f.max, -f.max, 0.0, -0.0, 1.5, -f.max, f.max, f.tiny], dtype=np.float32)
    got = M.sanitise(x)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()


def _with_line(C, value, axis, k):
    C = C.copy()
    if axis == 0:
        C[k, :] = value
    else:
        C[:, k] = value
    return C


@pytest.mark.parametrize("V", (1, 2, 5, 64, 70))
@pytest.mark.parametrize("axis", (0, 1))
@pytest.mark.parametrize("value", (np.nan, np.inf, -np.inf))
def test_whole_non_finite_lines_need_the_sanitised_load(value, axis, V):
    """A whole row or column of NaN / +inf: the unsanitised walk reads an unset path entry (the model reports it; the
    kernels before the sanitising load never returned).  Sanitised, every such matrix — whole lines of -inf too — gives
    an optimal permutation of the sanitised costs.  These inputs are for the model only, never for the device."""
    base = K.square_costs("gauss", V, 1)[0]
    for k in sorted({0, V // 2, V - 1}):
        C = _with_line(base, np.float32(value), axis, k)
        S = M.sanitise(C)
        assert np.isfinite(S).all()
        assert_optimal_permutation(S, M.square(S), exact=False)
        if value != -np.inf:
            with pytest.raises(M.UnsetPath):
                M.square(C)


@pytest.mark.parametrize("V", (4, 33, 64, 65, 130))
def test_partial_permutation_holes_leave_the_unsanitised_walk_finite(V):
    """The device tests' non-finite inputs (NaN / +inf on a partial permutation) keep a finite perfect matching: the
    algorithm ends on them with or without the sanitising load, and sanitised it finds scipy's optimum."""
    C = K.partial_permutation_holes(K.square_costs("gauss", V, 4), salt=V)
    for Cb in C:
        assert sorted(int(c) for c in M.square(Cb)) == list(range(V))           # no UnsetPath
        S = M.sanitise(Cb)
        c4r = M.square(S)
        assert_optimal_permutation(S, c4r, exact=False)
        assert np.isfinite(Cb[np.arange(V), c4r]).all()                         # no hole is used
