"""The device assignment solver (csrc/loss.hip) in all three forms, through ops.loss_assign:

  lsa64_kernel<false>   square problem, V <= 64, state in registers
  lsa64_kernel<true>    rectangular shortcut over `counts`, V <= 64
  lsa_kernel            64 < V <= 1024, state in LDS: lsa_rect_solve of csrc/lsa_solve.h on the square problem

Each result must be a permutation, carry scipy's optimal total (equal where the costs are integers or dyadic, within
1e-12 relative otherwise) and equal tests/lsa_model.py, the numpy statement of the kernels' algorithm and tie rule
("unassigned column first, then lowest index"), ELEMENT FOR ELEMENT — an optimum reached by another tie rule fails.
Sizes sit on both sides of the wave width, of the 64-column trips of lsa_rect_solve and of the switch between kernels;
inputs go beyond Gaussian costs: negative, badly scaled, tied (small integers, constant, rank one, lattice wireframes)
and the product matrix (i+1)(j+1), whose augmenting paths run through every assigned row.

Non-finite costs: only inputs whose finite entries still hold a perfect matching (NaN / +inf on a partial permutation;
predictions with NaN coordinates and enough dummy columns for them).  A matrix with a whole non-finite row or column
is never given to the device; tests/test_loss_assign_model.py covers it on the model."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lsa_cases as K  # noqa: E402
import lsa_model as M  # noqa: E402

LSA64_SIZES = (1, 2, 3, 31, 32, 33, 63, 64)
LSA_SIZES = (65, 127, 128, 129, 257, 320)
B = 5


def dev():
    return torch.device("cuda:0")


def assign(cost, counts=None):
    from wf3d import ops
    c = torch.from_numpy(np.ascontiguousarray(cost)).to(dev())
    n = None if counts is None else torch.from_numpy(np.asarray(counts, dtype=np.int64)).to(dev())
    return ops.loss_assign(c, n).cpu().numpy()


def device_cost(pv, pe, tv, counts):
    """ops.loss_cost_matrix on the generator's data; it must be the numpy statement of the cost kernel bit for bit."""
    from wf3d import ops
    t = [torch.from_numpy(a).to(dev()) for a in (pv, pe, tv, counts)]
    cost = ops.loss_cost_matrix(*t).cpu().numpy()
    assert np.array_equal(cost, K.wireframe_cost(pv, pe, tv, counts), equal_nan=True)
    return cost


def assert_equals_model(got, want, what):
    if not np.array_equal(got, want):
        p = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: device and model differ at {np.count_nonzero(got != want)} of {got.size} rows, "
                             f"first at prediction {p}: device {got[p]}, model {want[p]}")


def check_square(cost, got, exact, what):
    for b, (C, g) in enumerate(zip(cost, got)):
        K.assert_optimal_permutation(C, g, exact)
        assert_equals_model(g, M.square(C), f"{what}, sample {b}")


@pytest.mark.parametrize("V", LSA64_SIZES + LSA_SIZES)
@pytest.mark.parametrize("name", K.SQUARE)
def test_square_solver_equals_the_model(name, V):
    cost = K.square_costs(name, V, B)
    got = assign(cost)
    check_square(cost, got, name in K.EXACT, f"{name} V={V}")
    if name == "product":
        for C, g in zip(cost, got):
            assert C.astype(np.float64)[np.arange(V), g].sum() == K.product_optimum(V)


@pytest.mark.parametrize("V", LSA64_SIZES + LSA_SIZES)
@pytest.mark.parametrize("name", K.WIREFRAME)
def test_square_solver_equals_the_model_on_wireframe_costs(name, V):
    cost = device_cost(*K.wireframe_inputs(name, V, K.random_counts(name, V, B)))
    check_square(cost, assign(cost), name in K.EXACT, f"{name} V={V}")


@pytest.mark.parametrize("name", ("gauss", "perm_matrix"))
def test_square_solver_at_the_largest_size(name):
    V = 1024
    cost = K.square_costs(name, V, 2)
    check_square(cost, assign(cost), name in K.EXACT, f"{name} V={V}")


@pytest.mark.parametrize("V", LSA64_SIZES)
@pytest.mark.parametrize("name", ("wf_gauss", "wf_lattice"))
def test_rectangular_solver_equals_the_model(name, V):
    """Every count of {0, 1, V-1, V, V+5, -3}: V+5 behaves as V, -3 as 0."""
    counts = np.array([0, 1, V - 1, V, V + 5, -3], dtype=np.int64)
    cost = device_cost(*K.wireframe_inputs(name, V, counts))
    got = assign(cost, counts)
    for b, (C, g, n) in enumerate(zip(cost, got, counts)):
        K.assert_optimal_permutation(C, g, name in K.EXACT)                    # the square problem's optimum
        assert_equals_model(g, M.rect(C, n), f"{name} V={V} count={n}")
    assert_equals_model(got[4], M.rect(cost[4], V), "count V+5 as V")
    assert np.array_equal(got[5], np.arange(V))                                # nothing matched: dummy columns in order
    assert np.array_equal(got[0], np.arange(V))


@pytest.mark.parametrize("V", (65, 130))
def test_counts_above_64_vertices_fall_back_to_the_square_solver(V):
    counts = K.random_counts("fallback", V, B)
    cost = device_cost(*K.wireframe_inputs("wf_lattice", V, counts))
    assert np.array_equal(assign(cost, counts), assign(cost))


@pytest.mark.parametrize("V", (33, 64, 65, 130))
def test_samples_are_independent_and_calls_repeat(V):
    """One problem at b = 0 and again at b = B-1 among others gives the same row there, and alone; a second call gives
    the same bits.  Square form on Gaussian costs, form with counts on tied lattice wireframes."""
    square = K.square_costs("gauss", V, B)
    square[B - 1] = square[0]
    counts = K.random_counts("indep", V, B)
    counts[0] = counts[B - 1] = V // 2
    pv, pe, tv, counts = K.wireframe_inputs("wf_lattice", V, counts)
    for a in (pv, pe, tv):
        a[B - 1] = a[0]
    for batch, n in ((square, None), (device_cost(pv, pe, tv, counts), counts)):
        first, second = assign(batch, n), assign(batch, n)
        assert np.array_equal(first, second)
        assert np.array_equal(first[0], first[B - 1])
        assert np.array_equal(assign(batch[:1], None if n is None else n[:1])[0], first[0])


@pytest.mark.parametrize("V", (4, 33, 64, 65, 130))
def test_square_solver_reads_non_finite_costs_as_flt_max(V):
    """NaN / +inf on a partial permutation: the result is the model's on the sanitised matrix, optimal for it, and
    uses none of those entries."""
    cost = K.partial_permutation_holes(K.square_costs("gauss", V, 4), salt=V)
    got = assign(cost)
    for b, (C, g) in enumerate(zip(cost, got)):
        S = M.sanitise(C)
        K.assert_optimal_permutation(S, g, exact=False)
        assert_equals_model(g, M.square(S), f"holes V={V}, sample {b}")
        assert np.isfinite(C[np.arange(V), g]).all()


@pytest.mark.parametrize("V", (4, 33, 64, 65, 130))
def test_predictions_with_nan_coordinates_land_on_dummy_columns(V):
    """m predictions with a NaN coordinate and a finite existence probability, counts <= V - m: their cost rows are NaN
    on the real columns and finite on the dummies.  Both forms put each of them on a dummy column and match the other
    predictions as the model does on the sanitised cost."""
    m = max(1, V // 4)
    counts = np.array([0, 1, V - m, (V - m) // 2], dtype=np.int64)
    pv, pe, tv, counts = K.wireframe_inputs("wf_gauss", V, counts, salt=1)
    rng = np.random.default_rng(V)
    bad = np.stack([rng.permutation(V)[:m] for _ in counts])
    for b in range(len(counts)):
        pv[b, bad[b], rng.integers(0, 3, m)] = np.nan
    cost = device_cost(pv, pe, tv, counts)
    for rect in (False, True):
        got = assign(cost, counts if rect else None)
        for b, (C, g, n) in enumerate(zip(cost, got, counts)):
            assert np.isnan(C[bad[b], :n]).all() and np.isfinite(C[bad[b], n:]).all()
            assert sorted(g.tolist()) == list(range(V))
            assert (g[bad[b]] >= n).all()
            S = M.sanitise(C)
            want = M.rect(S, n) if rect and V <= 64 else M.square(S)
            ok = np.setdiff1d(np.arange(V), bad[b])
            assert_equals_model(g[ok], want[ok], f"NaN predictions V={V} rect={rect}, sample {b}")
