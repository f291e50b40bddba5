// The shortest-augmenting-path assignment solver whose state lies in memory (LDS or a workspace): one wave64 per problem,
// lanes = columns, duals and path costs in fp64 like scipy.  lsa_kernel (loss.hip: square problems on fp32 costs, V > 64)
// and lsa_rect_kernel (evalmetrics.hip: rectangular problems on fp64 costs) are its two callers;
// tests/lsa_model.py::_augmenting_paths states algorithm, association and tie rule in numpy, and both kernels' col4row
// equals it element for element (only additions and subtractions here: nothing contracts to an FMA).
//
// Termination on any input.  Every cost is read through lsa_cost64: NaN, +-inf and anything beyond +-FLT_MAX become
// +-FLT_MAX as doubles, a value inside is unchanged.  `r < spc` is false for a NaN and for +inf against the initial
// +inf, so a raw row without a finite entry would leave path[j] unset for a column that is still picked once only such
// columns remain, and the augmenting walk would then follow an unset entry and never meet `r == cur`.  With finite costs
// every r of a row's first scan is finite (the duals are sums and differences of finite costs, far below fp64's range)
// and less than the initial +inf, so the first scan sets path[j] for every column; later scans only overwrite it with
// rows scanned in this same search.  Every path entry the walk reads therefore names a row of this search's tree, each
// step moves one edge towards its root `cur`, and the walk ends after at most nrow steps.  Independently of that
// argument path[] is reset per search, a search scans at most nrow rows and the walk takes at most nrow steps: a wrong
// kernel would give a wrong answer and WF3D_EVAL_STEPS, never a hang.
#pragma once
#include <float.h>

#include "wf3d_common.h"

// bytes of solver state for a long side of L columns: 3 doubles, 4 ints and a flag per column
inline size_t lsa_state_bytes(long L) { return (size_t)((41 * L + 15) / 16 * 16); }

__device__ __forceinline__ double lsa_cost64(double c, bool& bad) {
    const double m = (double)FLT_MAX;
    if (!(c <= m && c >= -m)) bad = true;                                // NaN fails both
    return c < m ? (c > -m ? c : -m) : m;                                // NaN fails the first comparison
}

// cost(i, j) = C[i * rs + j * cs], nrow <= ncol.  State arrays are sized by ncol.  IN_LDS only separates the call sites'
// instantiations: in the ones whose `base` is the LDS array the compiler keeps every state access an LDS instruction.
// GUARD: the bounds and the per-search path reset of the last paragraph above.  The square call of loss.hip turns them
// off (fail_s may then be NULL): with them wf3d_loss_assign at B = 32, V = 256 took 32.4 ms against 30.0 / 30.1 ms, and it
// has no status to report a defect with.
// Returns WF3D_EVAL_STEPS | WF3D_EVAL_NONFINITE bits; out[p] = the column of row p.
template <typename CostT, bool IN_LDS, bool GUARD>
__device__ __forceinline__ int lsa_rect_solve(unsigned char* base, int* fail_s, const CostT* __restrict__ C, int nrow, int ncol,
                                              long rs, long cs, int32_t* __restrict__ out) {
    const long L = ncol;
    double* u = reinterpret_cast<double*>(base);            // [nrow] row duals
    double* v = u + L;                                      // [ncol] column duals
    double* spc = v + L;                                    // [ncol] shortest path costs
    int* path = reinterpret_cast<int*>(spc + L);            // [ncol]
    int* row4col = path + L;                                // [ncol]
    int* col4row = row4col + L;                             // [nrow]
    int* srlist = col4row + L;                              // [nrow]
    unsigned char* in_sc = reinterpret_cast<unsigned char*>(srlist + L);   // [ncol]
    const int lane = threadIdx.x;
    bool bad = false;
    for (int j = lane; j < ncol; j += 64) { v[j] = 0.0; row4col[j] = -1; }
    for (int i = lane; i < nrow; i += 64) { u[i] = 0.0; col4row[i] = -1; }
    if (GUARD && lane == 0) *fail_s = 0;
    __syncthreads();
    bool failed = false;
    for (int cur = 0; cur < nrow && !failed; ++cur) {
        for (int j = lane; j < ncol; j += 64) { spc[j] = INFINITY; in_sc[j] = 0; if (GUARD) path[j] = -1; }
        __syncthreads();
        int i = cur, sink = -1, nsr = 0;
        double min_val = 0.0;
        while (sink < 0) {
            if (GUARD && nsr >= nrow) { failed = true; break; }                  // a search scans each row at most once
            if (lane == 0) srlist[nsr] = i;
            ++nsr;
            const double ui = u[i];
            double best = INFINITY;
            int bestj = 0x7fffffff, best_free = 0;
            for (int j = lane; j < ncol; j += 64) {
                if (in_sc[j]) continue;
                const double r = min_val + lsa_cost64((double)C[(long)i * rs + (long)j * cs], bad) - ui - v[j];
                double cur_spc = spc[j];
                if (r < cur_spc) { cur_spc = r; spc[j] = r; path[j] = i; }
                const int fr = row4col[j] < 0;
                if (cur_spc < best || (cur_spc == best && (fr > best_free || (fr == best_free && j < bestj)))) {
                    best = cur_spc; bestj = j; best_free = fr;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o, 64);
                const int oj = __shfl_xor(bestj, o, 64), of = __shfl_xor(best_free, o, 64);
                if (ob < best || (ob == best && (of > best_free || (of == best_free && oj < bestj)))) {
                    best = ob; bestj = oj; best_free = of;
                }
            }
            if (GUARD && (bestj < 0 || bestj >= ncol)) { failed = true; break; }   // no unscanned column left: cannot happen before the bound
            min_val = best;
            if (lane == 0) in_sc[bestj] = 1;
            __syncthreads();
            const int r4c = row4col[bestj];
            if (r4c < 0) sink = bestj; else i = r4c;
        }
        if (failed) break;
        // dual update
        for (int k = lane; k < nsr; k += 64) {
            const int r = srlist[k];
            u[r] += (r == cur) ? min_val : min_val - spc[col4row[r]];
        }
        for (int j = lane; j < ncol; j += 64)
            if (in_sc[j]) v[j] -= min_val - spc[j];
        __syncthreads();
        // augment along the path (sequential), at most nrow steps
        if (lane == 0) {
            int j = sink, steps = 0;
            while (true) {
                const int r = (!GUARD || (j >= 0 && j < ncol)) ? path[j] : -1;
                if (GUARD && (r < 0 || r >= nrow || steps >= nrow)) { *fail_s = 1; break; }
                ++steps;
                row4col[j] = r;
                const int prev = col4row[r];
                col4row[r] = j;
                j = prev;
                if (r == cur) break;
            }
        }
        __syncthreads();
        if (GUARD) failed = *fail_s != 0;
    }
    __syncthreads();
    for (int p = lane; p < nrow; p += 64) out[p] = col4row[p];
    return (failed ? WF3D_EVAL_STEPS : 0) | (__ballot(bad) != 0ull ? WF3D_EVAL_NONFINITE : 0);
}
