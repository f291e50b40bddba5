// Training metrics on the device: batch-wide quality counters from the loss's own assignment (wf3d.meter.WireframeMeter).
// tests/train_metrics_model.py states all of it in numpy float64.
//
//   train_metrics_part_kernel    grid (1 + chunks, B).  Workgroup (0, b): sample b's matched pairs (count, sum of squared
//                                distances, sum of distances, pairs within the threshold) and its existence counters;
//                                workgroup (1 + c, b): the edge counters of columns [c * 2048, (c + 1) * 2048) of sample b
//                                below the common width.  Each writes one record of partials to the workspace.
//   train_metrics_final_kernel   one workgroup folds the records in a fixed order, writes row 0 of the state (this batch)
//                                and adds it to row 1 (the running sums).
//
// No atomics: integer counters are exact in any order, and the two fp64 sums are folded in an order that depends on the
// shapes only, so the same inputs give the same bits in eager mode and in a replay.  The common edge width is read from
// the device when the kernels run: the grid covers min(Ep, Et) columns and the chunks past the width write zeros.
#include "wf3d_common.h"

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_CHUNK = 2048;           // edge columns per workgroup: two 16-byte loads per thread and tensor
constexpr int MT_SAMPLE_REC = 8;         // doubles: n_pairs, sum_sq, sum_dist, n_within, ex_tp, ex_fp, ex_fn, count_abs_err
constexpr int MT_EDGE_REC = 4;           // int32: ed_tp, ed_fp, ed_fn, 0
constexpr int MT_COLS = 13;              // columns of a state row

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sums over the workgroup's four waves, wave 0 + wave 1 first: every thread gets the total.  Ends with a barrier.
template <typename T, int N>
__device__ __forceinline__ void block_fold(T (&v)[N], T (*red)[N]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) red[wave][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    __syncthreads();
}

__device__ __forceinline__ void edge_count(float p, float t, float thr, int& tp, int& fp, int& fn) {
    const bool pr = p > thr, lb = t > 0.5f;                  // a NaN on either side compares false
    tp += pr && lb; fp += pr && !lb; fn += !pr && lb;
}

__global__ __launch_bounds__(MT_THREADS) void train_metrics_part_kernel(
    const float* __restrict__ verts, long vs_b, long vs_v, const float* __restrict__ exist, const float* __restrict__ edge,
    int Ep, const float* __restrict__ tverts, int Vt, const float* __restrict__ texist, const float* __restrict__ tlabel,
    int Et, const int32_t* __restrict__ col4row, const int64_t* __restrict__ counts, const int64_t* __restrict__ ewidth,
    int V, float edge_threshold, double thresh2, double* __restrict__ sample_part, int32_t* __restrict__ edge_part) {
    __shared__ double red_d[4][2];
    __shared__ int red_i[4][6];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (blockIdx.x == 0) {
        // ---- matched pairs and existence of sample b ----
        const int vmax = V < Vt ? V : Vt;
        const int64_t c64 = counts[b];
        const int cb = c64 < 0 ? 0 : (c64 > vmax ? vmax : (int)c64);
        double sums[2] = {0.0, 0.0};                          // sum_sq, sum_dist
        int cnt[6] = {0, 0, 0, 0, 0, 0};                      // n_pairs, n_within, ex_tp, ex_fp, ex_fn, predicted
        for (int p = tid; p < V; p += MT_THREADS) {
            const int t = col4row[(size_t)b * V + p];
            if (t >= 0 && t < cb) {
#pragma clang fp contract(off)
                const float* v = verts + (size_t)b * vs_b + (size_t)p * vs_v;
                const float* w = tverts + ((size_t)b * Vt + t) * 3;
                const double dx = (double)v[0] - (double)w[0], dy = (double)v[1] - (double)w[1], dz = (double)v[2] - (double)w[2];
                const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
                const double d2 = (xx + yy) + zz;
                sums[0] += d2;
                sums[1] += sqrt(d2);
                cnt[0] += 1;
                cnt[1] += d2 <= thresh2;                      // false for a NaN distance
            }
            const bool pr = exist[(size_t)b * V + p] > 0.5f, lb = texist[(size_t)b * V + p] > 0.5f;
            cnt[2] += pr && lb; cnt[3] += pr && !lb; cnt[4] += !pr && lb; cnt[5] += pr;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) sums[k] = wave_sum_f64(sums[k]);
#pragma unroll
        for (int k = 0; k < 6; ++k) cnt[k] = wave_sum_int(cnt[k]);
        block_fold(sums, red_d);
        block_fold(cnt, red_i);
        if (tid == 0) {
            double* r = sample_part + (size_t)b * MT_SAMPLE_REC;
            const int diff = cnt[5] - cb;
            r[0] = cnt[0]; r[1] = sums[0]; r[2] = sums[1]; r[3] = cnt[1];
            r[4] = cnt[2]; r[5] = cnt[3]; r[6] = cnt[4]; r[7] = diff < 0 ? -diff : diff;
        }
        return;
    }
    // ---- edge columns [c0, c1) of sample b, below the common width ----
    const int chunk = blockIdx.x - 1, chunks = gridDim.x - 1;
    const int w = edge_common_width(ewidth ? *ewidth : (int64_t)Ep, Ep, Et);      // the loss's edge term runs over the same columns
    const long c0 = (long)chunk * MT_CHUNK;
    const long c1 = c0 + MT_CHUNK < (long)w ? c0 + MT_CHUNK : (long)w;
    int cnt[3] = {0, 0, 0};
    if (c0 < c1) {
        const float* e = edge + (size_t)b * Ep;
        const float* l = tlabel + (size_t)b * Et;
        long i0 = c0;                                          // columns [c0, i0) go through 16-byte loads
        if ((reinterpret_cast<uintptr_t>(e + c0) & 15) == 0 && (reinterpret_cast<uintptr_t>(l + c0) & 15) == 0) {
            const long n4 = (c1 - c0) / 4;                     // whole groups of four columns below c1: none reaches the width
            for (long g = tid; g < n4; g += MT_THREADS) {
                const f32x4 pe = *reinterpret_cast<const f32x4*>(e + c0 + 4 * g);
                const f32x4 pl = *reinterpret_cast<const f32x4*>(l + c0 + 4 * g);
#pragma unroll
                for (int k = 0; k < 4; ++k) edge_count(pe[k], pl[k], edge_threshold, cnt[0], cnt[1], cnt[2]);
            }
            i0 = c0 + 4 * n4;
        }
        for (long i = i0 + tid; i < c1; i += MT_THREADS) edge_count(e[i], l[i], edge_threshold, cnt[0], cnt[1], cnt[2]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) cnt[k] = wave_sum_int(cnt[k]);
    block_fold(cnt, reinterpret_cast<int(*)[3]>(&red_i[0][0]));
    if (tid == 0) {
        int32_t* r = edge_part + ((size_t)b * chunks + chunk) * MT_EDGE_REC;
        r[0] = cnt[0]; r[1] = cnt[1]; r[2] = cnt[2]; r[3] = 0;
    }
}

// thread t takes records t, t + 256, ... in rising order; the threads' sums meet in the shuffle tree and in block_fold
__global__ __launch_bounds__(MT_THREADS) void train_metrics_final_kernel(const double* __restrict__ sample_part,
                                                                         const int32_t* __restrict__ edge_part, int B,
                                                                         long edge_recs, double* __restrict__ state) {
    __shared__ double red_d[4][2];
    __shared__ long long red_l[4][9];
    const int tid = threadIdx.x;
    double sums[2] = {0.0, 0.0};
    long long cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};           // n_pairs, n_within, ex_tp, ex_fp, ex_fn, count_abs_err, ed_*
    for (int b = tid; b < B; b += MT_THREADS) {
        const double* r = sample_part + (size_t)b * MT_SAMPLE_REC;
        sums[0] += r[1]; sums[1] += r[2];
        cnt[0] += (long long)r[0]; cnt[1] += (long long)r[3]; cnt[2] += (long long)r[4]; cnt[3] += (long long)r[5];
        cnt[4] += (long long)r[6]; cnt[5] += (long long)r[7];
    }
    for (long i = tid; i < edge_recs; i += MT_THREADS) {
        const int32_t* r = edge_part + (size_t)i * MT_EDGE_REC;
        cnt[6] += r[0]; cnt[7] += r[1]; cnt[8] += r[2];
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) sums[k] = wave_sum_f64(sums[k]);
#pragma unroll
    for (int k = 0; k < 9; ++k) cnt[k] = wave_sum_ll(cnt[k]);
    block_fold(sums, red_d);
    block_fold(cnt, red_l);
    if (tid == 0) {
        const double row[MT_COLS] = {1.0, (double)B, (double)cnt[0], sums[0], sums[1], (double)cnt[1], (double)cnt[2],
                                     (double)cnt[3], (double)cnt[4], (double)cnt[5], (double)cnt[6], (double)cnt[7],
                                     (double)cnt[8]};
#pragma unroll
        for (int k = 0; k < MT_COLS; ++k) {
            state[k] = row[k];
            state[MT_COLS + k] += row[k];
        }
    }
}

inline long metrics_chunks(int Ep, int Et) {
    const int m = Ep < Et ? Ep : Et;
    return m > 0 ? ((long)m + MT_CHUNK - 1) / MT_CHUNK : 0;
}
inline size_t metrics_sample_bytes(int B) { return (size_t)B * MT_SAMPLE_REC * sizeof(double); }

}  // namespace

extern "C" size_t wf3d_train_metrics_ws_bytes(int B, int Ep) {
    if (B <= 0 || Ep < 0) return 0;
    return metrics_sample_bytes(B) + (size_t)B * (size_t)metrics_chunks(Ep, Ep) * MT_EDGE_REC * sizeof(int32_t);
}

extern "C" int wf3d_train_metrics(const float* verts, long sample_stride, long vertex_stride, const float* exist,
                                  const float* edge, int Ep, const float* tverts, int Vt, const float* texist,
                                  const float* tlabel, int Et, const int32_t* col4row, const int64_t* counts,
                                  const int64_t* edge_width, int B, int V, float edge_threshold, float distance_thresh,
                                  double* state, void* ws, size_t ws_bytes, void* stream) {
    WF3D_CHECK(B > 0 && V > 0 && Vt > 0 && Ep >= 0 && Et >= 0, WF3D_ERR_ARG,
               "wf3d_train_metrics: bad dims (B %d, V %d, Vt %d, Ep %d, Et %d)", B, V, Vt, Ep, Et);
    WF3D_CHECK(V <= 1024, WF3D_ERR_UNSUPPORTED, "wf3d_train_metrics: V > 1024 (got %d)", V);
    WF3D_CHECK(B <= 65535, WF3D_ERR_UNSUPPORTED, "wf3d_train_metrics: B > 65535 (got %d)", B);
    WF3D_CHECK((long)B * Ep < (1L << 31) && (long)B * Et < (1L << 31), WF3D_ERR_UNSUPPORTED,
               "wf3d_train_metrics: B * Ep or B * Et >= 2^31 (B %d, Ep %d, Et %d)", B, Ep, Et);
    WF3D_CHECK(verts && exist && tverts && texist && col4row && counts && state, WF3D_ERR_ARG, "wf3d_train_metrics: null pointer");
    WF3D_CHECK(Ep == 0 || edge, WF3D_ERR_ARG, "wf3d_train_metrics: null edge probabilities");
    WF3D_CHECK(Et == 0 || tlabel, WF3D_ERR_ARG, "wf3d_train_metrics: null edge labels");
    const long chunks = metrics_chunks(Ep, Et);
    const size_t need = metrics_sample_bytes(B) + (size_t)B * (size_t)chunks * MT_EDGE_REC * sizeof(int32_t);
    WF3D_CHECK(ws && ws_bytes >= need, WF3D_ERR_WS, "wf3d_train_metrics: workspace of %zu bytes, %zu needed", ws_bytes, need);
    WF3D_CHECK((reinterpret_cast<uintptr_t>(ws) & 15) == 0 && (reinterpret_cast<uintptr_t>(state) & 7) == 0, WF3D_ERR_ARG,
               "wf3d_train_metrics: workspace must be 16-byte and state 8-byte aligned");
    double* sample_part = (double*)ws;
    int32_t* edge_part = (int32_t*)((unsigned char*)ws + metrics_sample_bytes(B));
    hipStream_t st = (hipStream_t)stream;
    const double t = (double)distance_thresh;
    hipLaunchKernelGGL(train_metrics_part_kernel, dim3((unsigned)(1 + chunks), B), dim3(MT_THREADS), 0, st, verts, sample_stride,
                       vertex_stride, exist, edge, Ep, tverts, Vt, texist, tlabel, Et, col4row, counts, edge_width, V,
                       edge_threshold, t * t, sample_part, edge_part);
    WF3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(train_metrics_final_kernel, dim3(1), dim3(MT_THREADS), 0, st, (const double*)sample_part,
                       (const int32_t*)edge_part, B, (long)B * chunks, state);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}
