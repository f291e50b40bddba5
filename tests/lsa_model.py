"""A numpy model, in float64, of the device assignment solvers (csrc/lsa_solve.h, csrc/loss.hip): scipy's shortest-augmenting-path
algorithm with the kernels' own choices written out, so that a test can ask for the kernels' col4row element for
element and not merely for an optimum.

  square(C)        lsa_kernel (64 < V <= 1024: lsa_rect_solve of lsa_solve.h on the square problem) and
                   lsa64_kernel<false> (V <= 64)
  rect(C, count)   lsa64_kernel<true>: the rectangular shortcut over the real targets of a wireframe cost
  sanitise(C)      what every kernel's cost load does to a value that is not finite
_augmenting_paths is also the model of lsa_rect_kernel (csrc/evalmetrics.hip), the same lsa_rect_solve on rectangular
fp64 costs (tests/evalmetrics_model.py).

The kernels' choices:
  * rows are added in order cur = 0 .. nrow-1;
  * a scan of row i forms r = ((min_val + cost[i, j]) - u[i]) - v[j] in that association, for the unscanned columns;
  * spc[j] and path[j] change only where r < spc[j] (false for a NaN, and for +inf against the initial +inf);
  * the next column is, among the unscanned columns of minimal spc, the unassigned one of lowest index, or the
    lowest index when none is unassigned;
  * u[cur] += min_val, u[r] += min_val - spc[col4row[r]] for the other scanned rows, v[j] -= min_val - spc[j] for
    the scanned columns; then the matching is augmented along `path` from the sink back to row cur.
Only additions, subtractions and comparisons: nothing contracts to an FMA, so fp64 numpy reproduces the device bit
for bit and the assignments agree exactly.

A cost that is NaN or +inf never sets path[j].  Once only such columns remain, one of them is still picked, and the
augmenting walk then reads a path entry that no scan wrote (UnsetPath).  The kernels read their costs through
sanitise(), after which the first scan of every row sets path[j] for every column."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


class UnsetPath(RuntimeError):
    """The augmenting walk met a column whose path entry no scan of this row had written."""


def sanitise(C):
    """NaN and +inf -> FLT_MAX, -inf -> -FLT_MAX, every finite value unchanged (float32 in, float32 out)."""
    C = np.asarray(C, dtype=np.float32)
    out = np.where(C < np.float32(FLT_MAX), C, np.float32(FLT_MAX))          # NaN compares false
    return np.where(out > np.float32(-FLT_MAX), out, np.float32(-FLT_MAX)).astype(np.float32)


def _augmenting_paths(A):
    """A [nrow, ncol] float64, nrow <= ncol.  Returns (col4row [nrow], row4col [ncol], path steps taken)."""
    nrow, ncol = A.shape
    u, v = np.zeros(nrow), np.zeros(ncol)
    row4col, col4row = np.full(ncol, -1), np.full(nrow, -1)
    steps = 0
    for cur in range(nrow):
        # spc of the unscanned columns lives in `open_spc`, which holds +inf at the scanned ones so that one argmin
        # finds the next column; a column's final spc moves to `spc` when it is scanned (written as a few cheap
        # whole-array calls per step: the product matrix at V = 320 takes 51,360 steps)
        open_spc = np.full(ncol, np.inf)
        spc = np.full(ncol, np.inf)
        path = np.full(ncol, -1)
        unscanned = np.ones(ncol, dtype=bool)
        scanned_rows, scanned_cols = [], []
        i, sink, min_val = cur, -1, 0.0
        while sink < 0:
            steps += 1
            scanned_rows.append(i)
            r = min_val + A[i]
            r -= u[i]
            r -= v
            better = r < open_spc
            better &= unscanned
            np.copyto(open_spc, r, where=better)
            np.copyto(path, i, where=better)
            j = int(open_spc.argmin())                              # the lowest index among equal minima
            min_val = float(open_spc[j])
            if row4col[j] >= 0 or min_val == np.inf:                # look for a tied unassigned (and unscanned) column
                tied = np.flatnonzero((open_spc == min_val) & unscanned)
                unassigned = tied[row4col[tied] < 0]
                j = int(unassigned[0] if unassigned.size else tied[0])
            spc[j] = min_val
            open_spc[j] = np.inf
            unscanned[j] = False
            scanned_cols.append(j)
            if row4col[j] < 0:
                sink = j
            else:
                i = int(row4col[j])
        u[cur] += min_val
        for r_ in scanned_rows[1:]:
            u[r_] += min_val - spc[col4row[r_]]
        with np.errstate(invalid="ignore"):                         # inf - inf: only on costs that were not sanitised
            v[scanned_cols] -= min_val - spc[scanned_cols]
        j = sink
        for _ in range(ncol + 1):                   # a walk over set entries visits each column at most once
            r_ = int(path[j])
            if r_ < 0:
                raise UnsetPath(f"row {cur}: the walk from sink {sink} reads path[{j}], which no scan wrote")
            row4col[j] = r_
            col4row[r_], j = j, col4row[r_]
            if r_ == cur:
                break
        else:
            raise UnsetPath(f"row {cur}: the walk from sink {sink} did not reach row {cur}")
    return col4row, row4col, steps


def square(C, return_steps=False):
    """col4row [V] of the square problem on C [V, V] (float32 values, as the kernel reads them)."""
    C = np.asarray(C, dtype=np.float64)
    assert C.ndim == 2 and C.shape[0] == C.shape[1]
    col4row, _, steps = _augmenting_paths(C)
    return (col4row, steps) if return_steps else col4row


def rect(C, count):
    """col4row [V] of lsa64_kernel<true> on a wireframe cost C [V, V] whose columns >= count are identical dummies:
    rows are the real targets, columns the predictions, cost float64(C[p, t]) - ep[p] with ep[p] the dummy cost
    C[p, V-1] (0 when every column is real).  A matched prediction gets its target; the unmatched ones get the dummy
    columns nrow, nrow + 1, ... in index order."""
    C = np.asarray(C, dtype=np.float64)
    V = C.shape[0]
    nrow = min(max(int(count), 0), V)
    ep = C[:, V - 1] if nrow < V else np.zeros(V)
    _, row4col, _ = _augmenting_paths(C[:, :nrow].T - ep[None, :])
    out = row4col.copy()
    unmatched = np.flatnonzero(row4col < 0)
    out[unmatched] = nrow + np.arange(unmatched.size)
    return out
