// Evaluation metrics on the device: what eval/ap_calculator.py's compute_metrics derives from a sample's Hausdorff matrix
// (APCalculator._with_edges / _corners_only), for a whole batch.  tests/evalmetrics_model.py states all of it in numpy.
//
//   lsa_rect_kernel       B rectangular assignment problems on fp64 costs, one wave per sample: the solver of
//                         lsa_solve.h (shared with lsa_kernel of loss.hip; tests/lsa_model.py::_augmenting_paths) with
//                         nrow <= ncol, the matrix read through two strides so that the shorter side is the solver's rows
//                         without a transposed copy.  State in LDS while the long side is <= 1024, else in the caller's
//                         workspace.  The solver terminates on any input (lsa_solve.h); a defect shows as WF3D_EVAL_STEPS.
//   corner_sets_kernel    one workgroup per sample: the matched pairs under the threshold, the corner sets by VALUE (used
//                         flags over the V predicted and the label vertices, O(k^2) duplicate flags and counting ranks for
//                         np.unique / np.setdiff1d's lexicographic order), the free-corner distance matrix for the second
//                         assignment, and e_term.
//   finalize_kernel       one wave per sample: the second assignment's pairs in row order -> distances and the counters.
// wf3d_eval_metrics_nv gives every sample its own predicted vertex count (decoded wireframes): the first nverts[s] rows.
#include "lsa_solve.h"
#include "wf3d_common.h"

namespace {

constexpr int LSA_LDS_LONG = 1024;          // long side up to which the solver state lies in LDS (41 bytes per column)
constexpr int SETS_MAX = 1024;              // vertices per sample (predicted, label) of corner_sets_kernel
constexpr int SETS_THREADS = 256;

__global__ __launch_bounds__(64) void lsa_rect_kernel(const double* __restrict__ cost, const int64_t* __restrict__ ooff,
                                                      const int32_t* __restrict__ noff, const int32_t* __restrict__ moff,
                                                      int ostride, const int32_t* __restrict__ aoff, long max_long,
                                                      int32_t* __restrict__ col4row_out, int32_t* __restrict__ status,
                                                      unsigned char* __restrict__ ws, size_t ws_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    __shared__ int fail_s;
    const int s = blockIdx.x, lane = threadIdx.x;
    const long n = (long)noff[(long)s * ostride + 1] - noff[(long)s * ostride];
    const long m = (long)moff[(long)s * ostride + 1] - moff[(long)s * ostride];
    int st = 0;
    if (n < 0 || m < 0 || n > max_long || m > max_long) {
        st = WF3D_EVAL_RANGE;
    } else if (n > 0 && m > 0) {
        const double* C = cost + ooff[s];
        int32_t* out = col4row_out + aoff[s];
        const bool tr = n > m;                                           // the solver's rows are the shorter side
        const int nrow = (int)(tr ? m : n), ncol = (int)(tr ? n : m);
        const long rs = tr ? 1 : m, cs = tr ? m : 1;
        if (ncol <= LSA_LDS_LONG) st = lsa_rect_solve<double, true, true>(lsm, &fail_s, C, nrow, ncol, rs, cs, out);
        else st = lsa_rect_solve<double, false, true>(ws + (size_t)s * ws_stride, &fail_s, C, nrow, ncol, rs, cs, out);
    }
    if (lane == 0) status[s] = st;
}

// ---- corner sets --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool pt_eq(const float* a, const float* b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }
__device__ __forceinline__ bool pt_less(const float* a, const float* b) {
    return a[0] < b[0] || (a[0] == b[0] && (a[1] < b[1] || (a[1] == b[1] && a[2] < b[2])));
}
// scipy's cdist on the float64 copies: ((dx dx + dy dy) + dz dz), each product and sum rounded
__device__ __forceinline__ double pt_dist(const float* a, const float* b) {
#pragma clang fp contract(off)
    const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1], dz = (double)a[2] - (double)b[2];
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const double xy = xx + yy;
    return sqrt(xy + zz);
}
__device__ __forceinline__ bool pt_finite(const float* a) { return isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]); }

// rank[i] = -1 for a row equal to an earlier one; else the number of distinct rows of its own class (used or not) that
// are lexicographically below it.  cnt[0] / cnt[1] += the distinct used / unused rows.  Ends with a barrier.
__device__ __forceinline__ void rank_rows(const float* X, int N, const int* used, int* rank, int* cnt) {
    for (int i = threadIdx.x; i < N; i += SETS_THREADS) {
        int dup = 0;
        for (int k = 0; k < i; ++k) dup |= pt_eq(X + 3 * k, X + 3 * i);
        rank[i] = dup ? -1 : 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < N; i += SETS_THREADS) {
        if (rank[i] < 0) continue;
        int r = 0;
        // a rank that another thread has already written is >= 0 as well: the test below reads the same either way
        for (int k = 0; k < N; ++k) r += (rank[k] >= 0 && used[k] == used[i] && pt_less(X + 3 * k, X + 3 * i)) ? 1 : 0;
        rank[i] = r;
        atomicAdd(&cnt[used[i] ? 0 : 1], 1);
    }
    __syncthreads();
}

// The workspace of wf3d_eval_metrics, shared by its launches.
struct EvalWs {
    double* dm;          // [V * total_lverts]: sample s's free-corner matrix [nfp, nfg] row-major at dm + ooff2[s]
    int64_t* ooff2;      // [B]  = V * lvoff[s]
    double* eterm;       // [B]
    int32_t* dims;       // [2, B, 2] = (0, nfp) per sample, then (0, nfg): the second assignment's extents as (begin, end) pairs
    int32_t* aoff2;      // [B]  = s * V
    int32_t* part;       // [B, 4] = (|pr_u|, tp_edges, status, 0)
    int32_t* assign2;    // [B * V]
    int32_t* status1;    // [B]
    int32_t* status2;    // [B]
    int32_t* inv;        // [B * V]
    unsigned char* lsa;  // the solvers' own workspace
    size_t lsa_bytes, total;
};

EvalWs eval_ws(void* ws, int B, int V, long total_lverts, long max_long) {
    EvalWs w;
    unsigned char* p = (unsigned char*)ws;
    size_t o = 0;
    auto take = [&](size_t bytes) { unsigned char* q = p + o; o += (bytes + 15) / 16 * 16; return q; };
    w.dm = (double*)take((size_t)V * (size_t)total_lverts * 8);
    w.ooff2 = (int64_t*)take((size_t)B * 8);
    w.eterm = (double*)take((size_t)B * 8);
    w.dims = (int32_t*)take((size_t)B * 16);
    w.aoff2 = (int32_t*)take((size_t)B * 4);
    w.part = (int32_t*)take((size_t)B * 16);
    w.assign2 = (int32_t*)take((size_t)B * V * 4);
    w.status1 = (int32_t*)take((size_t)B * 4);
    w.status2 = (int32_t*)take((size_t)B * 4);
    w.inv = (int32_t*)take((size_t)B * V * 4);
    const long longest = max_long > SETS_MAX ? max_long : SETS_MAX;      // the second assignment's sides are <= 1024
    w.lsa_bytes = longest > LSA_LDS_LONG ? (size_t)B * lsa_state_bytes(longest) : 0;
    w.lsa = take(w.lsa_bytes);
    w.total = o;
    return w;
}

// sample s's predicted vertex count: the first clamp(nverts[s], 0, V) rows of its V (nverts null: all of them)
__device__ __forceinline__ int sample_verts(const int32_t* __restrict__ nverts, int s, int V) {
    return nverts ? min(max(nverts[s], 0), V) : V;
}

__global__ __launch_bounds__(SETS_THREADS) void corner_sets_kernel(
    const float* __restrict__ verts, long sstride, long vstride, int Vmax, const int32_t* __restrict__ nverts,
    const float* __restrict__ seg,
    const int32_t* __restrict__ koff, const float* __restrict__ lverts, const int32_t* __restrict__ lvoff,
    const float* __restrict__ lseg, const int32_t* __restrict__ loff, const double* __restrict__ hd,
    const int64_t* __restrict__ ooff, const int32_t* __restrict__ assign, const int32_t* __restrict__ aoff, double thresh,
    double* __restrict__ dm_all, int64_t* __restrict__ ooff2, double* __restrict__ eterm, int32_t* __restrict__ dims,
    int32_t* __restrict__ aoff2, int32_t* __restrict__ part) {
    __shared__ float Ps[SETS_MAX * 3], Gs[SETS_MAX * 3];
    __shared__ int used_p[SETS_MAX], used_g[SETS_MAX], rank_p[SETS_MAX], rank_g[SETS_MAX];
    __shared__ double emin[SETS_MAX];
    __shared__ int st_s, tp_s, cnt_p[2], cnt_g[2];
    const int s = blockIdx.x, tid = threadIdx.x, B = gridDim.x;
    const int V = sample_verts(nverts, s, Vmax);                 // the workspace layout keeps the stride Vmax
    const int k0 = koff[s], l0 = loff[s], g0 = lvoff[s];
    const long n = (long)koff[s + 1] - k0, m = (long)loff[s + 1] - l0;
    int Lv = lvoff[s + 1] - g0;
    int st = !(thresh == thresh) || isinf(thresh) ? WF3D_EVAL_NONFINITE : 0;
    if (Lv < 0 || Lv > SETS_MAX || n < 0 || m < 0) { st |= WF3D_EVAL_RANGE; Lv = 0; }     // the host checked max_lverts
    if (tid == 0) { st_s = 0; tp_s = 0; cnt_p[0] = cnt_p[1] = cnt_g[0] = cnt_g[1] = 0; }
    for (int i = tid; i < V; i += SETS_THREADS) {
        const float* p = verts + s * sstride + i * vstride;
        Ps[3 * i] = p[0]; Ps[3 * i + 1] = p[1]; Ps[3 * i + 2] = p[2];
        used_p[i] = 0;
        if (!pt_finite(p)) st |= WF3D_EVAL_NONFINITE;
    }
    for (int i = tid; i < Lv; i += SETS_THREADS) {
        const float* g = lverts + ((long)g0 + i) * 3;
        Gs[3 * i] = g[0]; Gs[3 * i + 1] = g[1]; Gs[3 * i + 2] = g[2];
        used_g[i] = 0;
        if (!pt_finite(g)) st |= WF3D_EVAL_NONFINITE;
    }
    const int64_t dmo = (int64_t)Vmax * g0;
    double* dm = dm_all + dmo;
    __syncthreads();
    if (n <= 0 || (st & WF3D_EVAL_RANGE)) {
        // corners only (APCalculator._corners_only): the rows as given, no de-duplication, no sorting
        for (long idx = tid; idx < (long)V * Lv; idx += SETS_THREADS) {
            const int i = (int)(idx / Lv), j = (int)(idx - (long)i * Lv);
            dm[idx] = pt_dist(Ps + 3 * i, Gs + 3 * j);
        }
        if (st) atomicOr(&st_s, st);
        __syncthreads();
        if (tid == 0) {
            ooff2[s] = dmo; aoff2[s] = s * Vmax; eterm[s] = 0.0;
            dims[2 * s] = 0; dims[2 * s + 1] = V; dims[2 * B + 2 * s] = 0; dims[2 * B + 2 * s + 1] = Lv;
            part[4 * s] = 0; part[4 * s + 1] = 0; part[4 * s + 2] = st_s; part[4 * s + 3] = 0;
        }
        return;
    }
    // matched pairs under the threshold; their end points mark the vertex rows of equal value
    const long k = n < m ? n : m;
    int tp = 0;
    for (long t = tid; t < k; t += SETS_THREADS) {
        const long a = assign[aoff[s] + t];
        const long p = n <= m ? t : a, l = n <= m ? a : t;
        if (p < 0 || p >= n || l < 0 || l >= m) { st |= WF3D_EVAL_RANGE; continue; }
        const double h = hd[ooff[s] + p * m + l];
        if (!(h == h) || isinf(h)) st |= WF3D_EVAL_NONFINITE;
        if (!(h <= thresh)) continue;
        ++tp;
        for (int e = 0; e < 2; ++e) {
            const float* q = seg + ((long)k0 + p) * 6 + 3 * e;
            bool found = false;
            for (int i = 0; i < V; ++i)
                if (pt_eq(q, Ps + 3 * i)) { used_p[i] = 1; found = true; }
            const float* r = lseg + ((long)l0 + l) * 6 + 3 * e;
            bool foundg = false;
            for (int i = 0; i < Lv; ++i)
                if (pt_eq(r, Gs + 3 * i)) { used_g[i] = 1; foundg = true; }
            if (!found || !foundg) st |= WF3D_EVAL_ENDPOINT;             // NaN end points land here too
        }
    }
    if (tp) atomicAdd(&tp_s, tp);
    if (st) atomicOr(&st_s, st);
    __syncthreads();
    rank_rows(Ps, V, used_p, rank_p, cnt_p);
    rank_rows(Gs, Lv, used_g, rank_g, cnt_g);
    const int npu = cnt_p[0], nfp = cnt_p[1], nfg = cnt_g[1];
    for (long idx = tid; idx < (long)V * Lv; idx += SETS_THREADS) {
        const int i = (int)(idx / Lv), j = (int)(idx - (long)i * Lv);
        if (rank_p[i] >= 0 && !used_p[i] && rank_g[j] >= 0 && !used_g[j])
            dm[(long)rank_p[i] * nfg + rank_g[j]] = pt_dist(Ps + 3 * i, Gs + 3 * j);
    }
    for (int i = tid; i < V; i += SETS_THREADS) {
        if (rank_p[i] < 0 || !used_p[i]) continue;
        double mn = INFINITY;
        for (int j = 0; j < Lv; ++j)
            if (rank_g[j] >= 0 && used_g[j]) mn = fmin(mn, pt_dist(Ps + 3 * i, Gs + 3 * j));
        emin[rank_p[i]] = mn;
    }
    __syncthreads();
    if (tid == 0) {
        double e = 0.0;
        for (int i = 0; i < npu; ++i) e += emin[i];                      // pr_u in lexicographic order
        int sts = st_s;
        if (npu == 0) sts |= WF3D_EVAL_NO_MATCH;
        if (!(e == e) || isinf(e)) sts |= WF3D_EVAL_NONFINITE;
        ooff2[s] = dmo; aoff2[s] = s * Vmax; eterm[s] = e;
        dims[2 * s] = 0; dims[2 * s + 1] = nfp; dims[2 * B + 2 * s] = 0; dims[2 * B + 2 * s + 1] = nfg;
        part[4 * s] = npu; part[4 * s + 1] = tp_s; part[4 * s + 2] = sts; part[4 * s + 3] = 0;
    }
}

__global__ __launch_bounds__(64) void finalize_kernel(int V, const int32_t* __restrict__ nverts, const int32_t* __restrict__ koff, const int32_t* __restrict__ lvoff,
                                                      const int32_t* __restrict__ loff, double thresh,
                                                      const double* __restrict__ dm_all, const int64_t* __restrict__ ooff2,
                                                      const double* __restrict__ eterm, const int32_t* __restrict__ dims,
                                                      const int32_t* __restrict__ part, const int32_t* __restrict__ assign2,
                                                      const int32_t* __restrict__ status1, const int32_t* __restrict__ status2,
                                                      int32_t* __restrict__ inv_all, int32_t* __restrict__ counters,
                                                      double* __restrict__ distances) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int nfp = dims[2 * s + 1], nfg = dims[2 * gridDim.x + 2 * s + 1];
    const int32_t* a2 = assign2 + (long)s * V;
    int32_t* inv = inv_all + (long)s * V;
    const double* dm = dm_all + ooff2[s];
    const bool tr = nfp > nfg;                   // entry j = the row of column j: turn it into the column of each row
    int st = 0;
    if (tr) {
        for (int i = lane; i < nfp; i += 64) inv[i] = -1;
        __syncthreads();
        for (int j = lane; j < nfg; j += 64) {
            const int r = a2[j];
            if (r >= 0 && r < nfp) inv[r] = j; else st |= WF3D_EVAL_RANGE;
        }
        __syncthreads();
    }
    const int bad = __ballot(st != 0) != 0ull ? WF3D_EVAL_RANGE : 0;
    if (lane != 0) return;
    st = bad | part[4 * s + 2] | status1[s] | status2[s];
    double sum = 0.0;
    int nok = 0;
    if (nfp > 0 && nfg > 0) {
        for (int i = 0; i < nfp; ++i) {                                  // row order, as np.sum over scipy's sorted pairs
            const int j = tr ? inv[i] : a2[i];
            if (tr && j < 0) continue;                                   // a row the assignment left free
            if (j < 0 || j >= nfg) { st |= WF3D_EVAL_RANGE; continue; }
            const double d = dm[(long)i * nfg + j];
            if (!(d == d) || isinf(d)) st |= WF3D_EVAL_NONFINITE;
            if (d <= thresh) { sum += d; ++nok; }
        }
    }
    distances[s] = sum + eterm[s];
    int32_t* c = counters + 8 * (long)s;
    c[0] = part[4 * s] + nok; c[1] = sample_verts(nverts, s, V); c[2] = lvoff[s + 1] - lvoff[s]; c[3] = part[4 * s + 1];
    c[4] = koff[s + 1] - koff[s]; c[5] = loff[s + 1] - loff[s]; c[6] = st; c[7] = 0;
}

int lsa_rect_launch(const double* cost, const int64_t* ooff, const int32_t* noff, const int32_t* moff, int off_stride,
                    const int32_t* aoff, int B, long max_long, int32_t* col4row, int32_t* status, void* ws, hipStream_t st) {
    const long lds_long = max_long < LSA_LDS_LONG ? (max_long < 1 ? 1 : max_long) : LSA_LDS_LONG;
    hipLaunchKernelGGL(lsa_rect_kernel, dim3(B), dim3(64), lsa_state_bytes(lds_long), st, cost, ooff, noff, moff, off_stride,
                       aoff, max_long, col4row, status, (unsigned char*)ws, lsa_state_bytes(max_long < 1 ? 1 : max_long));
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

}  // namespace

extern "C" size_t wf3d_lsa_rect_ws_bytes(int B, long max_long) {
    if (B <= 0 || max_long <= LSA_LDS_LONG) return 0;
    return (size_t)B * lsa_state_bytes(max_long);
}

extern "C" int wf3d_lsa_rect_batch(const double* cost, const int64_t* ooff, const int32_t* noff, const int32_t* moff,
                                   int off_stride, const int32_t* aoff, int B, long max_long, int32_t* col4row,
                                   int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    WF3D_CHECK(B >= 0 && max_long >= 0 && (off_stride == 1 || off_stride == 2), WF3D_ERR_ARG,
               "wf3d_lsa_rect_batch: bad dims (B %d, max_long %ld, off_stride %d)", B, max_long, off_stride);
    WF3D_CHECK(B <= 65535, WF3D_ERR_UNSUPPORTED, "wf3d_lsa_rect_batch: B > 65535 (got %d)", B);
    WF3D_CHECK(max_long < (1L << 31), WF3D_ERR_UNSUPPORTED, "wf3d_lsa_rect_batch: max_long %ld >= 2^31", max_long);
    if (B == 0) return WF3D_OK;
    WF3D_CHECK(cost && ooff && noff && moff && aoff && col4row && status, WF3D_ERR_ARG, "wf3d_lsa_rect_batch: null pointer");
    const size_t need = wf3d_lsa_rect_ws_bytes(B, max_long);
    WF3D_CHECK(need == 0 || (ws && ws_bytes >= need), WF3D_ERR_WS, "wf3d_lsa_rect_batch: workspace of %zu bytes, %zu needed",
               ws_bytes, need);
    return lsa_rect_launch(cost, ooff, noff, moff, off_stride, aoff, B, max_long, col4row, status, ws, (hipStream_t)stream);
}

extern "C" size_t wf3d_eval_metrics_ws_bytes(int B, int V, long total_lverts, long max_long) {
    if (B <= 0 || V < 0 || total_lverts < 0 || max_long < 0) return 0;
    return eval_ws(nullptr, B, V, total_lverts, max_long).total;
}

extern "C" int wf3d_eval_metrics_nv(const float* verts, long sample_stride, long vertex_stride, int B, int V,
                                    const int32_t* nverts, const float* seg, const int32_t* koff, const float* lverts,
                                    const int32_t* lvoff, const float* lseg, const int32_t* loff, const double* hd,
                                    const int64_t* ooff, const int32_t* aoff, int32_t* assign, double thresh, int max_lverts,
                                    long total_lverts, long max_long, int32_t* counters, double* distances, void* ws,
                                    size_t ws_bytes, void* stream) {
    WF3D_CHECK(B >= 0 && V >= 0 && max_lverts >= 0 && total_lverts >= 0 && max_long >= 0, WF3D_ERR_ARG,
               "wf3d_eval_metrics: bad dims");
    WF3D_CHECK(B <= 65535, WF3D_ERR_UNSUPPORTED, "wf3d_eval_metrics: B > 65535 (got %d)", B);
    WF3D_CHECK(V <= SETS_MAX && max_lverts <= SETS_MAX, WF3D_ERR_UNSUPPORTED,
               "wf3d_eval_metrics: at most 1024 predicted and 1024 label vertices per sample (V %d, label %d)", V, max_lverts);
    WF3D_CHECK((long)B * V < (1L << 31) && (long)V * total_lverts < (1L << 31) && max_long < (1L << 31), WF3D_ERR_UNSUPPORTED,
               "wf3d_eval_metrics: B * V, V * total_lverts or max_long >= 2^31 (B %d, V %d, total_lverts %ld, max_long %ld)", B,
               V, total_lverts, max_long);
    if (B == 0) return WF3D_OK;
    WF3D_CHECK(koff && lvoff && loff && ooff && aoff && counters && distances, WF3D_ERR_ARG, "wf3d_eval_metrics: null pointer");
    WF3D_CHECK(V == 0 || verts, WF3D_ERR_ARG, "wf3d_eval_metrics: null vertices");
    const EvalWs w = eval_ws(ws, B, V, total_lverts, max_long);
    WF3D_CHECK(ws && ws_bytes >= w.total, WF3D_ERR_WS, "wf3d_eval_metrics: workspace of %zu bytes, %zu needed", ws_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    // hd / assign / seg / lseg may be null when no sample has a pair: the kernels then read none of them
    int rc = lsa_rect_launch(hd, ooff, koff, loff, 1, aoff, B, max_long, assign, w.status1, w.lsa, st);
    if (rc != WF3D_OK) return rc;
    hipLaunchKernelGGL(corner_sets_kernel, dim3(B), dim3(SETS_THREADS), 0, st, verts, sample_stride, vertex_stride, V, nverts, seg, koff,
                       lverts, lvoff, lseg, loff, hd, ooff, assign, aoff, thresh, w.dm, w.ooff2, w.eterm, w.dims, w.aoff2, w.part);
    WF3D_LAUNCH_CHECK();
    rc = lsa_rect_launch(w.dm, w.ooff2, w.dims, w.dims + 2 * B, 2, w.aoff2, B, SETS_MAX, w.assign2, w.status2, w.lsa, st);
    if (rc != WF3D_OK) return rc;
    hipLaunchKernelGGL(finalize_kernel, dim3(B), dim3(64), 0, st, V, nverts, koff, lvoff, loff, thresh, w.dm, w.ooff2, w.eterm, w.dims,
                       w.part, w.assign2, w.status1, w.status2, w.inv, counters, distances);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" int wf3d_eval_metrics(const float* verts, long sample_stride, long vertex_stride, int B, int V, const float* seg,
                                 const int32_t* koff, const float* lverts, const int32_t* lvoff, const float* lseg,
                                 const int32_t* loff, const double* hd, const int64_t* ooff, const int32_t* aoff,
                                 int32_t* assign, double thresh, int max_lverts, long total_lverts, long max_long,
                                 int32_t* counters, double* distances, void* ws, size_t ws_bytes, void* stream) {
    return wf3d_eval_metrics_nv(verts, sample_stride, vertex_stride, B, V, nullptr, seg, koff, lverts, lvoff, lseg, loff, hd, ooff,
                                aoff, assign, thresh, max_lverts, total_lverts, max_long, counters, distances, ws, ws_bytes, stream);
}
