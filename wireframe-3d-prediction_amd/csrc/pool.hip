// Fused 4-way pooling over point_features [B, N, C] (HBM-bound, one pass).
//
// The reference reads point_features four times (masked mean + masked max in
// PointNetEncoder.py:103-111, unmasked mean + max in VertexPredictor.py:86-88);
// here one streaming pass yields all four reductions plus the two arg-max index
// vectors the backward scatter needs.
//
// pool4_partial_v4_kernel (C % 64 == 0): a wave reads 4 point rows x 64 channels per load instruction, 16 B per lane
// (lane = row-in-group x float4 column), four loads in flight per lane; each lane folds its rows in registers, the
// 4 row groups of a wave are folded by a WAVEFRONT SHUFFLE tree (xor 16, 32), the 4 waves of the workgroup by an
// LDS tree; the N axis is split over blockIdx.y so that thousands of workgroups fill the chip, and a tiny second
// kernel folds the splits.  Every fold keeps torch.max's first-max rule (equal values: the smaller n wins).
// pool4_partial_kernel (any C): thread = channel, 4-byte loads — the fallback.
//
// Both row walks are templates on ARG, whether the arg-max rows are kept.  The training kernels (dense and segmented) are
// the ARG instantiations; the forward-only streaming pool (wf3d.infer, below the packed layout) runs the same walks
// without arg-max over the slices of a passing block of rows and folds them into a running state.
#include "wf3d_common.h"

namespace {

struct PoolPart {           // per (b, split, c)
    float msum, usum, mmax, umax;
    int arg_m, arg_u;
};

__global__ __launch_bounds__(256) void point_valid_kernel(const float* __restrict__ x, int M, int in_dim,
                                                           float* __restrict__ valid,
                                                           const int32_t* __restrict__ live_rows) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= wf3d_live_extent(live_rows, M)) return;       // rows past a live-row count's extent: neither read nor written
    float s = 0.f;
    for (int k = 0; k < in_dim; ++k) s += fabsf(x[(size_t)m * in_dim + k]);
    valid[m] = s > 1e-9f ? 1.0f : 0.0f;
}

// The partial kernels' bodies work on one range of rows of one cloud: `pf` / `valid` point at a base row, n0..n1 are rows
// from that base (the arg-max indices they record are those row numbers), `part` / `cnt_part` at the slot of this range.
// The dense kernels take the cloud and the range from the grid (base = the cloud's first row), the segmented ones (packed
// batches, below) from a chunk table, the streaming ones (further below) from a slice of the block that passes (base =
// the block's first row).
//
// ARG: keep the arg-max rows (training: the backward scatter reads them).  The two forms also differ on a NaN, and each
// keeps its rule as it was, since each is held to its own model by its own tests and a change is visible in the outputs:
//   ARG    a row is taken as the maximum when `v > max || arg < 0`: the first row of a range is always taken, so a NaN
//          there is taken and then sticks (no later `v > NaN` is true);
//   !ARG   `v > max` from -inf: a NaN is never taken.
// Making them one rule would change what one of the forms returns on such inputs; that is left to a change of its own.
//
// pool4_takes: whether a row's value v replaces the running maximum mx, whose row so far is arg (< 0: none yet; !ARG: unused).
template <bool ARG>
__device__ __forceinline__ bool pool4_takes(float v, float mx, int arg) {
    return ARG ? (v > mx || arg < 0) : v > mx;
}

struct Pool1 { float msum, usum, mmax, umax, cnt; int am, au; };       // one channel over a range of rows (am, au: ARG)

// the scalar walk: rows n0..n1 of channel c, in row order
template <bool ARG>
__device__ __forceinline__ Pool1 pool4_walk_rows(const float* __restrict__ pf, const float* __restrict__ valid, int n0, int n1,
                                                 int C, int c) {
    Pool1 a{0.f, 0.f, -INFINITY, -INFINITY, 0.f, -1, -1};
    const float* p = pf + (size_t)n0 * C + c;
    for (int n = n0; n < n1; ++n, p += C) {
        const float v = *p;
        const float ok = valid[n];
        a.usum += v;
        if (pool4_takes<ARG>(v, a.umax, a.au)) { a.umax = v; a.au = n; }
        if (ok != 0.f) {
            a.msum += v; a.cnt += 1.f;
            if (pool4_takes<ARG>(v, a.mmax, a.am)) { a.mmax = v; a.am = n; }
        }
    }
    return a;
}

// the partial record of one (range of rows, channel): with the arg-max rows for training, 16 bytes for the streaming pool
__device__ __forceinline__ void pool4_store(PoolPart* p, float msum, float usum, float mmax, float umax, int am, int au) {
    *p = PoolPart{msum, usum, mmax, umax, am, au};
}
__device__ __forceinline__ void pool4_store(f32x4* p, float msum, float usum, float mmax, float umax, int, int) {
    *p = f32x4{msum, usum, mmax, umax};
}

template <bool ARG, typename Part>
__device__ __forceinline__ void pool4_partial_rows(const float* __restrict__ pf, const float* __restrict__ valid,
                                                   int n0, int n1, int C,
                                                   Part* __restrict__ part, float* __restrict__ cnt_part) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    float cnt = 0.f;
    if (c < C) {
        const Pool1 a = pool4_walk_rows<ARG>(pf, valid, n0, n1, C, c);
        cnt = a.cnt;
        pool4_store(part + c, a.msum, a.usum, a.mmax, a.umax, a.am, a.au);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *cnt_part = cnt;          // channel 0 exists: every thread counts the same rows
}

__global__ __launch_bounds__(256) void pool4_partial_kernel(const float* __restrict__ pf, const float* __restrict__ valid,
                                                             int N, int C, int nsplit, int npb,
                                                             PoolPart* __restrict__ part, float* __restrict__ cnt_part) {
    const int b = blockIdx.z, sp = blockIdx.y;
    const int n0 = sp * npb, n1 = min(N, n0 + npb);
    const size_t slot = (size_t)b * nsplit + sp;
    pool4_partial_rows<true>(pf + (size_t)b * N * C, valid + (size_t)b * N, n0, n1, C, part + slot * C, cnt_part + slot);
}

template <bool ARG> struct Pool4;              // running state of 4 channels
template <> struct Pool4<true> {
    f32x4 msum, usum, mmax, umax;
    int am[4], au[4];
};
template <> struct Pool4<false> { f32x4 msum, usum, mmax, umax; };

// fold `o` into `a`; ARG: on equal maxima the smaller point index wins (torch.max returns the first maximum)
template <bool ARG>
__device__ __forceinline__ void pool4_merge(Pool4<ARG>& a, const Pool4<ARG>& o) {
    a.msum += o.msum;
    a.usum += o.usum;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if constexpr (ARG) {
            if (o.au[e] >= 0 && (a.au[e] < 0 || o.umax[e] > a.umax[e] || (o.umax[e] == a.umax[e] && o.au[e] < a.au[e]))) {
                a.umax[e] = o.umax[e]; a.au[e] = o.au[e];
            }
            if (o.am[e] >= 0 && (a.am[e] < 0 || o.mmax[e] > a.mmax[e] || (o.mmax[e] == a.mmax[e] && o.am[e] < a.am[e]))) {
                a.mmax[e] = o.mmax[e]; a.am[e] = o.am[e];
            }
        } else {
            if (pool4_takes<false>(o.umax[e], a.umax[e], -1)) a.umax[e] = o.umax[e];
            if (pool4_takes<false>(o.mmax[e], a.mmax[e], -1)) a.mmax[e] = o.mmax[e];
        }
    }
}

template <bool ARG>
__device__ __forceinline__ Pool4<ARG> pool4_shfl_xor(const Pool4<ARG>& a, int mask) {
    Pool4<ARG> o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        o.msum[e] = __shfl_xor(a.msum[e], mask, 64); o.usum[e] = __shfl_xor(a.usum[e], mask, 64);
        o.mmax[e] = __shfl_xor(a.mmax[e], mask, 64); o.umax[e] = __shfl_xor(a.umax[e], mask, 64);
        if constexpr (ARG) { o.am[e] = __shfl_xor(a.am[e], mask, 64); o.au[e] = __shfl_xor(a.au[e], mask, 64); }
    }
    return o;
}

// NT: read the rows with non-temporal loads (training: a pass over a tensor written long before); plain loads where the
// rows were written just before (the streaming pool's block comes from the GEMM in front of it).
template <bool ARG, bool NT, typename Part>
__device__ __forceinline__ void pool4_partial_v4_rows(const float* __restrict__ pf, const float* __restrict__ valid,
                                                      int n0, int n1, int C,
                                                      Part* __restrict__ part, float* __restrict__ cnt_part) {
    __shared__ Pool4<ARG> s_p[3][16];
    __shared__ float s_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rsub = lane >> 4, c = blockIdx.x * 64 + (lane & 15) * 4;
    Pool4<ARG> a;
    a.msum = a.usum = f32x4{0.f, 0.f, 0.f, 0.f};
    a.mmax = a.umax = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if constexpr (ARG) {
#pragma unroll
        for (int e = 0; e < 4; ++e) a.am[e] = a.au[e] = -1;
    }
    float cnt = 0.f;
    const float* base = pf + c;
    const float* vp = valid;
    constexpr int U = 4;                                   // 4 independent 16-B loads per lane in flight
    for (int n = n0 + wave * 4 + rsub; n < n1; n += 16 * U) {
        f32x4 v[U];
        float ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int nn = n + 16 * u;
            if (nn < n1) {
                const f32x4* q = reinterpret_cast<const f32x4*>(base + (size_t)nn * C);
                v[u] = NT ? __builtin_nontemporal_load(q) : *q;
                ok[u] = vp[nn];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int nn = n + 16 * u;
            if (nn < n1) {
                a.usum += v[u];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if constexpr (ARG) {
                        if (pool4_takes<true>(v[u][e], a.umax[e], a.au[e])) { a.umax[e] = v[u][e]; a.au[e] = nn; }
                    } else if (pool4_takes<false>(v[u][e], a.umax[e], -1)) a.umax[e] = v[u][e];
                }
                if (ok[u] != 0.f) {
                    a.msum += v[u];
                    cnt += 1.f;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if constexpr (ARG) {
                            if (pool4_takes<true>(v[u][e], a.mmax[e], a.am[e])) { a.mmax[e] = v[u][e]; a.am[e] = nn; }
                        } else if (pool4_takes<false>(v[u][e], a.mmax[e], -1)) a.mmax[e] = v[u][e];
                    }
                }
            }
        }
    }
    // wavefront shuffle tree over the wave's 4 row groups
    pool4_merge(a, pool4_shfl_xor(a, 16));
    pool4_merge(a, pool4_shfl_xor(a, 32));
    cnt += __shfl_xor(cnt, 16, 64);
    cnt += __shfl_xor(cnt, 32, 64);
    // LDS tree over the 4 waves
    if (wave > 0 && lane < 16) s_p[wave - 1][lane] = a;
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (wave == 0 && lane < 16) {
        pool4_merge(a, s_p[0][lane]);
        pool4_merge(a, s_p[1][lane]);
        pool4_merge(a, s_p[2][lane]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (ARG) pool4_store(part + c + e, a.msum[e], a.usum[e], a.mmax[e], a.umax[e], a.am[e], a.au[e]);
            else pool4_store(part + c + e, a.msum[e], a.usum[e], a.mmax[e], a.umax[e], -1, -1);
        }
        if (blockIdx.x == 0 && lane == 0) *cnt_part = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    }
}

__global__ __launch_bounds__(256) void pool4_partial_v4_kernel(const float* __restrict__ pf, const float* __restrict__ valid,
                                                                int N, int C, int nsplit, int npb,
                                                                PoolPart* __restrict__ part, float* __restrict__ cnt_part) {
    const int b = blockIdx.z, sp = blockIdx.y;
    const int n0 = sp * npb, n1 = min(N, n0 + npb);
    const size_t slot = (size_t)b * nsplit + sp;
    pool4_partial_v4_rows<true, true>(pf + (size_t)b * N * C, valid + (size_t)b * N, n0, n1, C, part + slot * C, cnt_part + slot);
}

// folds the `nsplit` partial results of cloud b (N points), slots s0 .. s0 + nsplit - 1, in slot order
__device__ __forceinline__ void pool4_final_cloud(const PoolPart* __restrict__ part,
                                                  const float* __restrict__ cnt_part, int b, size_t s0, int N, int C,
                                                  int nsplit, int ldo, float* __restrict__ nvalid_o,
                                                  float* __restrict__ mmax_o,
                                                  float* __restrict__ mavg_o, float* __restrict__ umean_o,
                                                  float* __restrict__ umax_o, int32_t* __restrict__ arg_m_o,
                                                  int32_t* __restrict__ arg_u_o, float* __restrict__ cnt_o) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    float cnt = 0.f;
    for (int s = 0; s < nsplit; ++s) cnt += cnt_part[s0 + s];
    const float cl = fmaxf(cnt, 1.0f);                      // clamp(min=1), PointNetEncoder.py:86
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        cnt_o[b] = cl;
        if (nvalid_o) nvalid_o[b] = cnt;
    }
    if (c >= C) return;
    float msum = 0.f, usum = 0.f, mmax = -INFINITY, umax = -INFINITY;
    int am = -1, au = -1;
    for (int s = 0; s < nsplit; ++s) {
        const PoolPart q = part[(s0 + s) * C + c];
        msum += q.msum; usum += q.usum;
        if (q.arg_u >= 0 && (q.umax > umax || au < 0)) { umax = q.umax; au = q.arg_u; }
        if (q.arg_m >= 0 && (q.mmax > mmax || am < 0)) { mmax = q.mmax; am = q.arg_m; }
    }
    const size_t o = (size_t)b * C + c, ov = (size_t)b * ldo + c;
    // where(isfinite(max), max, 0): a cloud with no valid point pools to 0 and passes no gradient
    const bool fin = am >= 0 && isfinite(mmax);
    mmax_o[ov] = fin ? mmax : 0.f;
    arg_m_o[o] = fin ? am : -1;
    mavg_o[ov] = msum / cl;
    // a cloud of no rows (a capacity table built from device counts may hold one) pools to 0 like a dead cloud
    umean_o[ov] = N > 0 ? usum / (float)N : 0.f;
    umax_o[ov] = au >= 0 ? umax : 0.f;
    arg_u_o[o] = au;
}

__global__ __launch_bounds__(256) void pool4_final_kernel(const PoolPart* __restrict__ part,
                                                           const float* __restrict__ cnt_part, int N, int C,
                                                           int nsplit, int ldo, float* __restrict__ nvalid_o,
                                                           float* __restrict__ mmax_o,
                                                           float* __restrict__ mavg_o, float* __restrict__ umean_o,
                                                           float* __restrict__ umax_o, int32_t* __restrict__ arg_m_o,
                                                           int32_t* __restrict__ arg_u_o, float* __restrict__ cnt_o) {
    const int b = blockIdx.y;
    pool4_final_cloud(part, cnt_part, b, (size_t)b * nsplit, N, C, nsplit, ldo, nvalid_o, mmax_o, mavg_o, umean_o, umax_o,
                      arg_m_o, arg_u_o, cnt_o);
}

// dpf written 16 B per lane: a thread owns 4 channels of one cloud (its 4 pooled cotangents and
// 2 arg-max indices live in registers) and walks the points of its split; 256/(C/4) points of a
// split are written per pass, each a contiguous C*4-byte row.
// SX8: dpf is written as the next GEMMs' split operand (include/wf3d.h, sx8): the two threads that own a group of 8
// channels swap halves, one stores the group's 8 high parts, the other its 8 low parts (wf3d_store_sx8_pair).
// The bodies work on rows n0..n1 of cloud b, whose first row is row `row0` of valid / dpf (N = its point count).
template <bool SX8>
__device__ __forceinline__ void pool4_bwd_rows(const float* __restrict__ valid, const float* __restrict__ cnt,
                                               const int32_t* __restrict__ arg_m, const int32_t* __restrict__ arg_u,
                                               const float* __restrict__ dmmax, const float* __restrict__ dmavg,
                                               const float* __restrict__ dumean, const float* __restrict__ dumax,
                                               const float* __restrict__ dpf_direct, int b, size_t row0, int n0, int n1,
                                               int N, int C, int ldm, int ldu, float* __restrict__ dpf) {
    const int tpr = C / 4 < 256 ? C / 4 : 256;             // threads per point row
    const int rpb = 256 / tpr;                             // point rows per pass
    const int rsub = threadIdx.x / tpr;
    const int c = (blockIdx.x * tpr + threadIdx.x % tpr) * 4;
    if (c >= C || rsub >= rpb) return;
    const size_t o = (size_t)b * C + c, om = (size_t)b * ldm + c, ou = (size_t)b * ldu + c;
    const float inv_cnt = 1.0f / cnt[b], inv_n = 1.0f / (float)N;
    f32x4 g_avg = {0.f, 0.f, 0.f, 0.f}, g_mean = g_avg, g_mm = g_avg, g_um = g_avg;
    if (dmavg) g_avg = *reinterpret_cast<const f32x4*>(dmavg + om) * inv_cnt;
    if (dumean) g_mean = *reinterpret_cast<const f32x4*>(dumean + ou) * inv_n;
    if (dmmax) g_mm = *reinterpret_cast<const f32x4*>(dmmax + om);
    if (dumax) g_um = *reinterpret_cast<const f32x4*>(dumax + ou);
    int am[4], au[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { am[j] = arg_m[o + j]; au[j] = arg_u[o + j]; }
    for (int n = n0 + rsub; n < n1; n += rpb) {
        const size_t idx = (row0 + n) * C + c;
        const float v = valid[row0 + n];
        f32x4 g = g_mean + g_avg * v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (n == am[j]) g[j] += g_mm[j];
            if (n == au[j]) g[j] += g_um[j];
        }
        if (dpf_direct) g += *reinterpret_cast<const f32x4*>(dpf_direct + idx);
        if (SX8) {
            // lanes (2m, 2m+1) hold one sx8 group: one exchange, then 16 contiguous bytes per lane (wf3d_store_sx8_pair)
            const float gv[4] = {g[0], g[1], g[2], g[3]};
            wf3d_store_sx8_pair(dpf + idx, gv, (c & 4) != 0);
        } else {
            *reinterpret_cast<f32x4*>(dpf + idx) = g;
        }
    }
}

template <bool SX8>
__global__ __launch_bounds__(256) void pool4_bwd_kernel(const float* __restrict__ valid, const float* __restrict__ cnt,
                                                         const int32_t* __restrict__ arg_m, const int32_t* __restrict__ arg_u,
                                                         const float* __restrict__ dmmax, const float* __restrict__ dmavg,
                                                         const float* __restrict__ dumean, const float* __restrict__ dumax,
                                                         const float* __restrict__ dpf_direct, int N, int C,
                                                         int npb, int ldm, int ldu, float* __restrict__ dpf) {
    const int b = blockIdx.z;
    const int n0 = blockIdx.y * npb, n1 = min(N, n0 + npb);
    pool4_bwd_rows<SX8>(valid, cnt, arg_m, arg_u, dmmax, dmavg, dumean, dumax, dpf_direct, b, (size_t)b * N, n0, n1, N, C,
                        ldm, ldu, dpf);
}

// scalar fallback for channel counts that are not a multiple of 4
__device__ __forceinline__ void pool4_bwd_scalar_rows(const float* __restrict__ valid, const float* __restrict__ cnt,
                                                      const int32_t* __restrict__ arg_m, const int32_t* __restrict__ arg_u,
                                                      const float* __restrict__ dmmax, const float* __restrict__ dmavg,
                                                      const float* __restrict__ dumean, const float* __restrict__ dumax,
                                                      const float* __restrict__ dpf_direct, int b, size_t row0, int n0,
                                                      int n1, int N, int C, int ldm, int ldu, float* __restrict__ dpf) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const size_t o = (size_t)b * C + c, om = (size_t)b * ldm + c, ou = (size_t)b * ldu + c;
    const float g_avg = dmavg ? dmavg[om] / cnt[b] : 0.f;
    const float g_mean = dumean ? dumean[ou] / (float)N : 0.f;
    const float g_mm = dmmax ? dmmax[om] : 0.f;
    const float g_um = dumax ? dumax[ou] : 0.f;
    const int am = arg_m[o], au = arg_u[o];
    for (int n = n0; n < n1; ++n) {
        const size_t idx = (row0 + n) * C + c;
        float g = g_mean + valid[row0 + n] * g_avg;
        if (n == am) g += g_mm;
        if (n == au) g += g_um;
        if (dpf_direct) g += dpf_direct[idx];
        dpf[idx] = g;
    }
}

__global__ __launch_bounds__(256) void pool4_bwd_scalar_kernel(const float* __restrict__ valid, const float* __restrict__ cnt,
                                                                const int32_t* __restrict__ arg_m, const int32_t* __restrict__ arg_u,
                                                                const float* __restrict__ dmmax, const float* __restrict__ dmavg,
                                                                const float* __restrict__ dumean, const float* __restrict__ dumax,
                                                                const float* __restrict__ dpf_direct, int N, int C,
                                                                int npb, int ldm, int ldu, float* __restrict__ dpf) {
    const int b = blockIdx.z;
    const int n0 = blockIdx.y * npb, n1 = min(N, n0 + npb);
    pool4_bwd_scalar_rows(valid, cnt, arg_m, arg_u, dmmax, dmavg, dumean, dumax, dpf_direct, b, (size_t)b * N, n0, n1, N, C,
                          ldm, ldu, dpf);
}

// Column sums over all B*N rows of what pool4_bwd writes, from the [B, C] cotangents alone (the bias gradient of the
// Linear in front of the pool):  sum_b  dmavg*nvalid/cnt + [arg_u >= 0]*(dumean + dumax) + [arg_m >= 0]*dmmax.
// arg_u < 0 only for a cloud of no rows (packed batches on device counts), whose backward writes nothing.
__global__ __launch_bounds__(256) void pool4_bwd_bias_kernel(const float* __restrict__ cnt, const float* __restrict__ nvalid,
                                                              const int32_t* __restrict__ arg_m, const int32_t* __restrict__ arg_u,
                                                              const float* __restrict__ dmmax, const float* __restrict__ dmavg,
                                                              const float* __restrict__ dumean, const float* __restrict__ dumax,
                                                              int B, int C, int ldm, int ldu, float* __restrict__ out) {
    // 32 columns x 8 cloud lanes per workgroup (the clouds' loads are independent), folded in LDS in lane order
    __shared__ float s_p[8][32];
    const int cl = threadIdx.x & 31, bg = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    float acc = 0.f;
    if (c < C)
        for (int b = bg; b < B; b += 8) {
            const size_t o = (size_t)b * C + c, om = (size_t)b * ldm + c, ou = (size_t)b * ldu + c;
            float v = 0.f;
            if (dmavg) v += dmavg[om] * (nvalid[b] / cnt[b]);
            const bool rows = arg_u[o] >= 0;
            if (dumean && rows) v += dumean[ou];
            if (dmmax && arg_m[o] >= 0) v += dmmax[om];
            if (dumax && rows) v += dumax[ou];
            acc += v;
        }
    s_p[bg][cl] = acc;
    __syncthreads();
    if (bg == 0 && c < C) {
        float a = 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) a += s_p[g][cl];
        out[c] = a;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Segmented pools: a packed batch, the clouds concatenated along the point axis (include/wf3d.h, "PACKED batches").
// chunks[k] = (cloud b, first row of cloud b, r0, r1): rows r0..r1-1 of the packed tensor, all of cloud b.  The chunks
// of a cloud are consecutive and in row order (cchunk[b] .. cchunk[b+1]-1), so pool4_seg_final_kernel folds them in
// fixed order with the first-max rule.  The table is the host's (wf3d.ops.PackedLayout builds it from validated counts) or
// packed_layout_kernel's (below, from device counts, for a fixed row capacity) and is trusted like any other offset array
// of the ABI.  A chunk of cloud -1 holds pad rows, which only the backward visits (zeros); an empty one (r0 == r1) is a
// dead entry of a capacity table and does nothing.
// ---------------------------------------------------------------------------------------------------------------------
struct SegChunk { int b, n0, n1; size_t row0; int N; };

__device__ __forceinline__ SegChunk seg_chunk(const int32_t* __restrict__ rows, const int32_t* __restrict__ chunks, int k) {
    const int4 q = *reinterpret_cast<const int4*>(chunks + 4 * (size_t)k);
    return SegChunk{q.x, q.z - q.y, q.w - q.y, (size_t)q.y, rows[q.x + 1] - q.y};
}

template <bool V4>
__global__ __launch_bounds__(256) void pool4_seg_partial_kernel(const float* __restrict__ pf, const float* __restrict__ valid,
                                                                 const int32_t* __restrict__ rows,
                                                                 const int32_t* __restrict__ chunks, int B, int M, int C,
                                                                 PoolPart* __restrict__ part, float* __restrict__ cnt_part) {
    const int k = blockIdx.y;
    if (chunks[4 * (size_t)k] < 0) return;                 // pad rows, or a dead entry of a capacity table: no cloud reads them
    const SegChunk s = seg_chunk(rows, chunks, k);
    if (V4) pool4_partial_v4_rows<true, true>(pf + s.row0 * C, valid + s.row0, s.n0, s.n1, C, part + (size_t)k * C, cnt_part + k);
    else    pool4_partial_rows<true>(pf + s.row0 * C, valid + s.row0, s.n0, s.n1, C, part + (size_t)k * C, cnt_part + k);
}

__global__ __launch_bounds__(256) void pool4_seg_final_kernel(const PoolPart* __restrict__ part,
                                                               const float* __restrict__ cnt_part,
                                                               const int32_t* __restrict__ rows,
                                                               const int32_t* __restrict__ cchunk, int nchunk, int C, int ldo,
                                                               float* __restrict__ nvalid_o, float* __restrict__ mmax_o,
                                                               float* __restrict__ mavg_o, float* __restrict__ umean_o,
                                                               float* __restrict__ umax_o, int32_t* __restrict__ arg_m_o,
                                                               int32_t* __restrict__ arg_u_o, float* __restrict__ cnt_o) {
    const int b = blockIdx.y;
    const int s0 = cchunk[b], s1 = cchunk[b + 1];
    const int N = rows[b + 1] - rows[b];
    pool4_final_cloud(part, cnt_part, b, (size_t)s0, N, C, s1 - s0, ldo, nvalid_o, mmax_o, mavg_o, umean_o, umax_o,
                      arg_m_o, arg_u_o, cnt_o);
}

// grid (column blocks, parts of a chunk, chunks); MODE 0: fp32, 16 B per lane; 1: sx8; 2: scalar (C % 4 != 0).
// The pad chunk (cloud -1: rows M .. M_pad-1) is written as exact zeros — in sx8 too, whose zero is all-zero bits.
// Under a live-row count (the packed batch's row total, rows[B]) the zero fill stops at its extent over M_pad rows: no
// pad row at or past it is written.  The clouds' chunks lie below the live total and are walked as without a count.
template <int MODE>
__global__ __launch_bounds__(256) void pool4_seg_bwd_kernel(const float* __restrict__ valid, const float* __restrict__ cnt,
                                                             const int32_t* __restrict__ arg_m, const int32_t* __restrict__ arg_u,
                                                             const float* __restrict__ dmmax, const float* __restrict__ dmavg,
                                                             const float* __restrict__ dumean, const float* __restrict__ dumax,
                                                             const float* __restrict__ dpf_direct,
                                                             const int32_t* __restrict__ rows, const int32_t* __restrict__ chunks,
                                                             int B, int M, int M_pad, int C, int ldm, int ldu,
                                                             float* __restrict__ dpf, const int32_t* __restrict__ live_rows) {
    const int k = blockIdx.z;
    const int4 q = *reinterpret_cast<const int4*>(chunks + 4 * (size_t)k);
    if (q.x < 0) {
        if (blockIdx.x != 0) return;
        const int r0 = q.z, r1 = min(q.w, wf3d_live_extent(live_rows, M_pad));
        for (size_t i = (size_t)r0 * C + blockIdx.y * 256 + threadIdx.x; i < (size_t)r1 * C; i += (size_t)gridDim.y * 256)
            dpf[i] = 0.f;
        return;
    }
    const SegChunk s = seg_chunk(rows, chunks, k);
    const int per = (s.n1 - s.n0 + (int)gridDim.y - 1) / (int)gridDim.y;
    const int n0 = s.n0 + blockIdx.y * per, n1 = min(s.n1, n0 + per);
    if (MODE == 2)
        pool4_bwd_scalar_rows(valid, cnt, arg_m, arg_u, dmmax, dmavg, dumean, dumax, dpf_direct, s.b, s.row0, n0, n1, s.N, C,
                              ldm, ldu, dpf);
    else
        pool4_bwd_rows<MODE == 1>(valid, cnt, arg_m, arg_u, dmmax, dmavg, dumean, dumax, dpf_direct, s.b, s.row0, n0, n1, s.N,
                                  C, ldm, ldu, dpf);
}

// ---------------------------------------------------------------------------------------------------------------------
// The chunk table of a packed batch built on the device, for a fixed row capacity (include/wf3d.h, "PACKED batches",
// capacity form): rows / cchunk / chunks from the counts in device memory, one workgroup, plain vector stores.  Thread t
// owns clouds t*per .. t*per+per-1; two block scans (rows, then chunks) place them.  Counts are clamped: below 0 -> 0,
// a cloud that would pass `capacity` ends there, later clouds get no rows.  status: bit 0 = clamped for capacity,
// bit 1 = some cloud has no rows.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long block_scan_excl(long long v, long long* s, long long* total) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const long long x = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    const long long incl = s[t];
    *total = s[255];
    __syncthreads();
    return incl - v;
}

template <typename CountT>
__global__ __launch_bounds__(256) void packed_layout_kernel(const CountT* __restrict__ counts, int B, int capacity,
                                                             int chunk_rows, int nchunk_cap, int32_t* __restrict__ rows,
                                                             int32_t* __restrict__ cchunk, int32_t* __restrict__ chunks,
                                                             int32_t* __restrict__ status) {
    __shared__ long long s_scan[256];
    __shared__ int s_flags;
    const int t = threadIdx.x;
    const int per = (B + 255) / 256;
    const int b0 = min(t * per, B), b1 = min(b0 + per, B);
    if (t == 0) s_flags = 0;
    const auto clamped = [&](int b) {
        const long long c = (long long)counts[b];
        return c < 0 ? 0ll : (c > capacity ? (long long)capacity : c);
    };
    long long sum = 0;
    for (int b = b0; b < b1; ++b) sum += clamped(b);
    long long total;
    const long long off = block_scan_excl(sum, s_scan, &total);
    // rows, and the number of chunks of this thread's clouds
    int flags = 0;
    long long o = off, nck = 0;
    for (int b = b0; b < b1; ++b) {
        const int start = (int)min(o, (long long)capacity);
        o += clamped(b);
        const int end = (int)min(o, (long long)capacity);
        if ((long long)counts[b] > capacity || o > capacity) flags |= 1;
        if (end == start) flags |= 2;
        rows[b + 1] = end;
        nck += (end - start + chunk_rows - 1) / chunk_rows;
    }
    if (flags) atomicOr(&s_flags, flags);
    long long ktotal;
    long long k = block_scan_excl(nck, s_scan, &ktotal);
    o = off;
    for (int b = b0; b < b1; ++b) {
        const int start = (int)min(o, (long long)capacity);
        o += clamped(b);
        const int end = (int)min(o, (long long)capacity);
        cchunk[b] = (int)k;
        for (int r0 = start; r0 < end; r0 += chunk_rows, ++k)
            if (k < nchunk_cap)
                *reinterpret_cast<int4*>(chunks + 4 * (size_t)k) = make_int4(b, start, r0, min(r0 + chunk_rows, end));
    }
    // the pad rows M .. capacity-1 in pieces of chunk_rows, then dead entries (capacity, capacity) up to nchunk_cap
    const long long M = min(total, (long long)capacity);
    for (long long kk = ktotal + t; kk < nchunk_cap; kk += 256) {
        const int r0 = (int)min(M + (kk - ktotal) * chunk_rows, (long long)capacity);
        *reinterpret_cast<int4*>(chunks + 4 * (size_t)kk) = make_int4(-1, 0, r0, min(r0 + chunk_rows, capacity));
    }
    if (t == 0) {
        rows[0] = 0;
        cchunk[B] = (int)ktotal;
        *status = s_flags;                                 // every atomicOr precedes the second scan's barriers
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Streaming pool (forward only, wf3d.infer).  The per-point MLP runs over one block of rows [r0, r0 + rows) of the flat row
// space at a time; the pools are a running state per (cloud, channel) that each block is folded into as it passes:
//     state[b * C + c] = (masked sum, unmasked sum, masked max, unmasked max)      one 16-byte piece
//     cnt[b]           = valid rows seen so far                                    behind the B * C pieces
// The cloud of a row comes from the int32 device table of B + 1 row offsets (a packed layout's `rows`; b * N for a dense
// batch), which only the kernels read.  A block may start and end anywhere.  It is cut into slices of `spr` rows:
//   - pool4_stream_partial_kernel reduces every slice that lies inside ONE cloud to one partial per channel with the
//     training kernels' row walks (!ARG: no arg-max is kept, nothing reads it without a backward);
//   - pool4_stream_fold_kernel has ONE owner thread per (cloud, channel): it walks the slices that hold rows of its
//     cloud in ascending row order and adds the slice's partial — or, for a slice that straddles a cloud boundary or the
//     end of the live rows (at most two per cloud and block, `spr` rows each), the cloud's rows of that slice read
//     directly — into the state.  No atomics: the summation order is a function of (offsets, r0, rows, C) alone.
// Rows at or past offsets[B] belong to no cloud and are never read.
// ---------------------------------------------------------------------------------------------------------------------
// the cloud of row r < offsets[B]: the largest b with offsets[b] <= r (a cloud of no rows is never the answer)
__device__ __forceinline__ int stream_cloud_of(const int32_t* __restrict__ offsets, int B, int r) {
    int lo = 0, hi = B;                                    // offsets[lo] <= r < offsets[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// Slice s of the block: rows [a, e) of the flat row space, cut at the end of the block and of the live rows.  `whole`:
// the slice has rows and they are all one cloud's, so its partial exists.
struct StreamSlice { int a, e, b; bool whole; };

__device__ __forceinline__ StreamSlice stream_slice(const int32_t* __restrict__ offsets, int B, int r0, int rows, int spr, int s) {
    StreamSlice q;
    const long end = min((long)r0 + rows, (long)offsets[B]);
    q.a = (int)min((long)r0 + (long)s * spr, (long)r0 + rows);
    q.e = (int)max((long)q.a, min((long)q.a + spr, end));
    q.b = -1;
    q.whole = false;
    if (q.e > q.a) {
        q.b = stream_cloud_of(offsets, B, q.a);
        q.whole = q.e <= offsets[q.b + 1];
    }
    return q;
}

// grid (C / 64 or ceil(C / 256), slices).  pf / valid point at row r0 (the block's first row).
template <bool V4>
__global__ __launch_bounds__(256) void pool4_stream_partial_kernel(const float* __restrict__ pf, const float* __restrict__ valid,
                                                                    const int32_t* __restrict__ offsets, int B, int r0,
                                                                    int rows, int spr, int C, f32x4* __restrict__ part,
                                                                    float* __restrict__ cnt_part) {
    const int s = blockIdx.y;
    const StreamSlice q = stream_slice(offsets, B, r0, rows, spr, s);
    if (!q.whole) return;                                  // the fold reads a straddling slice's rows itself
    const int n0 = q.a - r0, n1 = q.e - r0;                // rows of the block
    if (V4) pool4_partial_v4_rows<false, false>(pf, valid, n0, n1, C, part + (size_t)s * C, cnt_part + s);
    else    pool4_partial_rows<false>(pf, valid, n0, n1, C, part + (size_t)s * C, cnt_part + s);
}

// grid (ceil(C / 256), B): thread = the owner of (cloud b, channel c)
__global__ __launch_bounds__(256) void pool4_stream_fold_kernel(const float* __restrict__ pf, const float* __restrict__ valid,
                                                                 const int32_t* __restrict__ offsets, int B, int r0, int rows,
                                                                 int spr, int C, const f32x4* __restrict__ part,
                                                                 const float* __restrict__ cnt_part, f32x4* __restrict__ state,
                                                                 float* __restrict__ cnt_state) {
    const int b = blockIdx.y;
    const int c = blockIdx.x * 256 + threadIdx.x;
    // the cloud's rows inside this block
    const long lo = max((long)offsets[b], (long)r0), hi = min((long)offsets[b + 1], (long)r0 + rows);
    if (hi <= lo) return;
    if (c >= C) return;
    const bool counts = c == 0;                            // channel 0's owner also owns the cloud's valid-row count
    f32x4 st = state[(size_t)b * C + c];
    float cnt = counts ? cnt_state[b] : 0.f;
    const int s_first = (int)((lo - r0) / spr), s_last = (int)((hi - 1 - r0) / spr);
    for (int s = s_first; s <= s_last; ++s) {
        const long a = max(lo, (long)r0 + (long)s * spr), e = min(hi, (long)r0 + (long)(s + 1) * spr);
        // the slice's partial exists when all its live rows are this cloud's (stream_slice, whole)
        const long sa = (long)r0 + (long)s * spr, se = min(min(sa + spr, (long)r0 + rows), (long)offsets[B]);
        if (a == sa && e == se) {
            const f32x4 q = part[(size_t)s * C + c];
            st[0] += q[0]; st[1] += q[1];
            st[2] = q[2] > st[2] ? q[2] : st[2];
            st[3] = q[3] > st[3] ? q[3] : st[3];
            if (counts) cnt += cnt_part[s];
        } else {
            const Pool1 q = pool4_walk_rows<false>(pf, valid, (int)(a - r0), (int)(e - r0), C, c);
            st[0] += q.msum; st[1] += q.usum;
            st[2] = q.mmax > st[2] ? q.mmax : st[2];
            st[3] = q.umax > st[3] ? q.umax : st[3];
            cnt += q.cnt;
        }
    }
    state[(size_t)b * C + c] = st;
    if (counts) cnt_state[b] = cnt;
}

__global__ __launch_bounds__(256) void pool4_stream_init_kernel(f32x4* __restrict__ state, float* __restrict__ cnt_state,
                                                                 long n, int B) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) state[i] = f32x4{0.f, 0.f, -INFINITY, -INFINITY};
    if (i < B) cnt_state[i] = 0.f;
}

// grid (ceil(C / 256), B): what pool4_final_cloud writes, without the arg-max rows
__global__ __launch_bounds__(256) void pool4_stream_finish_kernel(const f32x4* __restrict__ state,
                                                                   const float* __restrict__ cnt_state,
                                                                   const int32_t* __restrict__ offsets, int C, int ldo,
                                                                   float* __restrict__ mmax_o, float* __restrict__ mavg_o,
                                                                   float* __restrict__ umean_o, float* __restrict__ umax_o,
                                                                   float* __restrict__ cnt_o, float* __restrict__ nvalid_o) {
    const int b = blockIdx.y;
    const int c = blockIdx.x * 256 + threadIdx.x;
    const float cnt = cnt_state[b];
    const float cl = fmaxf(cnt, 1.0f);                      // clamp(min=1), PointNetEncoder.py:86
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        cnt_o[b] = cl;
        if (nvalid_o) nvalid_o[b] = cnt;
    }
    if (c >= C) return;
    const int N = offsets[b + 1] - offsets[b];
    const f32x4 st = state[(size_t)b * C + c];
    const size_t ov = (size_t)b * ldo + c;
    // where(isfinite(max), max, 0): a cloud with no valid row pools to 0
    mmax_o[ov] = (cnt > 0.f && isfinite(st[2])) ? st[2] : 0.f;
    mavg_o[ov] = st[0] / cl;
    // a cloud of no rows pools to zeros, as pool4_seg_fwd gives
    umean_o[ov] = N > 0 ? st[1] / (float)N : 0.f;
    umax_o[ov] = N > 0 ? st[3] : 0.f;
}

// Rows per slice of a block of `rows` rows: about 512 workgroups over column blocks x slices (two per CU at rows = 8192,
// C = 512: 64 slices of 128 rows), a slice no shorter than 64 rows (32: thread-per-channel form) and a multiple of 16,
// the rows of one pass of the 16-byte form.  A function of (rows, C) alone: so is the summation order.
int stream_spr(int rows, int C) {
    const bool v4 = C % 64 == 0;
    const int cb = v4 ? C / 64 : wf3d_cdiv(C, 256);
    int ns = 512 / cb;
    const int cap = wf3d_cdiv(rows, v4 ? 64 : 32);
    ns = ns > cap ? cap : ns;
    ns = ns < 1 ? 1 : ns;
    return wf3d_cdiv(wf3d_cdiv(rows, ns), 16) * 16;
}

size_t stream_part_bytes(int ns, int C) { return ((size_t)ns * C * sizeof(f32x4) + 255) & ~(size_t)255; }

int packed_chunk_rows(int rows) {                          // wf3d.ops.PackedLayout: about 256 chunks, at least 256 rows each
    const int per = wf3d_cdiv(wf3d_cdiv(rows, 256), 64) * 64;
    return per < 256 ? 256 : per;
}

bool pool_v4(const float* pf, int C) { return C % 64 == 0 && ((uintptr_t)pf % 16) == 0; }

int pool_nsplit(int B, int N, int C) {
    // v4 kernel: C/64 workgroups per (cloud, split), >= 64 rows per wave; fallback: C/256 per (cloud, split)
    const int cb = C % 64 == 0 ? C / 64 : wf3d_cdiv(C, 256);
    // 2048 workgroups: a sweep of 1024..16384 in situ gave 64..71 us, flat
    int ns = 2048 / (B * cb > 0 ? B * cb : 1);
    const int cap = wf3d_cdiv(N, C % 64 == 0 ? 256 : 32);
    if (ns > cap) ns = cap;
    if (ns < 1) ns = 1;
    return ns;
}

}  // namespace

extern "C" int wf3d_point_valid(const float* x, int M, int in_dim, float* valid, void* stream) {
    WF3D_CHECK(M >= 0 && in_dim > 0, WF3D_ERR_ARG, "wf3d_point_valid: bad dims");
    if (M == 0) return WF3D_OK;
    WF3D_CHECK(x && valid, WF3D_ERR_ARG, "wf3d_point_valid: null pointer");
    hipLaunchKernelGGL(point_valid_kernel, dim3(wf3d_cdiv(M, 256)), dim3(256), 0, (hipStream_t)stream, x, M, in_dim, valid,
                       wf3d_live_rows());
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" size_t wf3d_pool4_ws_bytes(int B, int N, int C) {
    if (B <= 0 || N <= 0 || C <= 0) return 0;
    const int ns = pool_nsplit(B, N, C);
    size_t bytes = (size_t)B * ns * C * sizeof(PoolPart);
    bytes = (bytes + 255) & ~(size_t)255;
    return bytes + (size_t)B * ns * sizeof(float);
}

extern "C" int wf3d_pool4_fwd(const float* pf, const float* valid, int B, int N, int C, float* mmax, float* mavg,
                              float* umean, float* umax, int ldo, int32_t* arg_m, int32_t* arg_u, float* cnt,
                              float* nvalid, void* ws, size_t ws_bytes, void* stream) {
    WF3D_CHECK(ldo >= C, WF3D_ERR_ARG, "wf3d_pool4_fwd: ldo=%d < C=%d", ldo, C);
    WF3D_CHECK(B > 0 && N > 0 && C > 0, WF3D_ERR_ARG, "wf3d_pool4_fwd: bad dims B=%d N=%d C=%d", B, N, C);
    WF3D_CHECK(B <= 65535, WF3D_ERR_UNSUPPORTED, "wf3d_pool4_fwd: B > 65535");
    WF3D_CHECK(pf && valid && mmax && mavg && umean && umax && arg_m && arg_u && cnt, WF3D_ERR_ARG, "wf3d_pool4_fwd: null pointer");
    WF3D_CHECK(ws && ws_bytes >= wf3d_pool4_ws_bytes(B, N, C), WF3D_ERR_WS, "wf3d_pool4_fwd: workspace too small");
    const int ns = pool_nsplit(B, N, C);
    const int npb = wf3d_cdiv(N, ns);
    PoolPart* part = (PoolPart*)ws;
    size_t off = ((size_t)B * ns * C * sizeof(PoolPart) + 255) & ~(size_t)255;
    float* cnt_part = (float*)((char*)ws + off);
    hipStream_t st = (hipStream_t)stream;
    if (pool_v4(pf, C))
        hipLaunchKernelGGL(pool4_partial_v4_kernel, dim3(C / 64, ns, B), dim3(256), 0, st, pf, valid, N, C, ns, npb, part, cnt_part);
    else
        hipLaunchKernelGGL(pool4_partial_kernel, dim3(wf3d_cdiv(C, 256), ns, B), dim3(256), 0, st, pf, valid, N, C, ns, npb, part, cnt_part);
    WF3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(pool4_final_kernel, dim3(wf3d_cdiv(C, 256), B), dim3(256), 0, st, part, cnt_part, N, C, ns, ldo, nvalid,
                       mmax, mavg, umean, umax, arg_m, arg_u, cnt);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

static int pool4_bwd_impl(const float* valid, const float* cnt, const int32_t* arg_m, const int32_t* arg_u,
                          const float* dmmax, const float* dmavg, int ldm, const float* dumean, const float* dumax, int ldu,
                          const float* dpf_direct, int B, int N, int C, float* dpf, bool sx8, void* stream);

extern "C" int wf3d_pool4_bwd(const float* valid, const float* cnt, const int32_t* arg_m, const int32_t* arg_u,
                              const float* dmmax, const float* dmavg, int ldm, const float* dumean, const float* dumax,
                              int ldu, const float* dpf_direct, int B, int N, int C, float* dpf, void* stream) {
    return pool4_bwd_impl(valid, cnt, arg_m, arg_u, dmmax, dmavg, ldm, dumean, dumax, ldu, dpf_direct, B, N, C, dpf, false, stream);
}

extern "C" int wf3d_pool4_bwd_sx8(const float* valid, const float* cnt, const int32_t* arg_m, const int32_t* arg_u,
                                  const float* dmmax, const float* dmavg, int ldm, const float* dumean, const float* dumax,
                                  int ldu, const float* dpf_direct, int B, int N, int C, float* dpf_sx8, void* stream) {
    return pool4_bwd_impl(valid, cnt, arg_m, arg_u, dmmax, dmavg, ldm, dumean, dumax, ldu, dpf_direct, B, N, C, dpf_sx8, true, stream);
}

extern "C" int wf3d_pool4_bwd_bias(const float* cnt, const float* nvalid, const int32_t* arg_m, const int32_t* arg_u,
                                   const float* dmmax, const float* dmavg, int ldm, const float* dumean, const float* dumax,
                                   int ldu, int B, int C, float* dbias, void* stream) {
    WF3D_CHECK(B > 0 && C > 0 && cnt && nvalid && arg_m && arg_u && dbias, WF3D_ERR_ARG, "wf3d_pool4_bwd_bias: bad arguments");
    hipLaunchKernelGGL(pool4_bwd_bias_kernel, dim3(wf3d_cdiv(C, 32)), dim3(256), 0, (hipStream_t)stream, cnt, nvalid, arg_m,
                       arg_u, dmmax, dmavg, dumean, dumax, B, C, ldm, ldu, dbias);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

static int pool4_bwd_impl(const float* valid, const float* cnt, const int32_t* arg_m, const int32_t* arg_u,
                          const float* dmmax, const float* dmavg, int ldm, const float* dumean, const float* dumax, int ldu,
                          const float* dpf_direct, int B, int N, int C, float* dpf, bool sx8, void* stream) {
    WF3D_CHECK(B > 0 && N > 0 && C > 0 && B <= 65535, WF3D_ERR_ARG, "wf3d_pool4_bwd: bad dims");
    WF3D_CHECK(valid && cnt && arg_m && arg_u && dpf, WF3D_ERR_ARG, "wf3d_pool4_bwd: null pointer");
    const auto al = [](const float* p, int ld) { return !p || ((uintptr_t)p % 16 == 0 && ld % 4 == 0); };
    const bool vec = C % 4 == 0 && ((uintptr_t)dpf % 16 == 0) && (!dpf_direct || (uintptr_t)dpf_direct % 16 == 0) &&
                     al(dmmax, ldm) && al(dmavg, ldm) && al(dumean, ldu) && al(dumax, ldu);
    // (any C / 4: the kernel idles the threads beyond rows-per-pass x C / 4 of a workgroup — PointNetEncoder(output_dim=768)
    // used to be refused here, in the middle of a backward pass)
    WF3D_CHECK(!sx8 || (vec && C % 8 == 0), WF3D_ERR_UNSUPPORTED, "wf3d_pool4_bwd_sx8: needs C %% 8 == 0 and 16-B aligned tensors (C=%d)", C);
    if (vec) {
        int ns = 4096 / (B * wf3d_cdiv(C / 4, 256));
        const int cap = wf3d_cdiv(N, 16);
        ns = ns > cap ? cap : (ns < 1 ? 1 : ns);
        const int npb = wf3d_cdiv(N, ns);
        if (sx8) hipLaunchKernelGGL(pool4_bwd_kernel<true>, dim3(wf3d_cdiv(C / 4, 256), ns, B), dim3(256), 0, (hipStream_t)stream,
                                    valid, cnt, arg_m, arg_u, dmmax, dmavg, dumean, dumax, dpf_direct, N, C, npb, ldm, ldu, dpf);
        else     hipLaunchKernelGGL(pool4_bwd_kernel<false>, dim3(wf3d_cdiv(C / 4, 256), ns, B), dim3(256), 0, (hipStream_t)stream,
                                    valid, cnt, arg_m, arg_u, dmmax, dmavg, dumean, dumax, dpf_direct, N, C, npb, ldm, ldu, dpf);
    } else {
        const int ns = pool_nsplit(B, N, C);
        const int npb = wf3d_cdiv(N, ns);
        hipLaunchKernelGGL(pool4_bwd_scalar_kernel, dim3(wf3d_cdiv(C, 256), ns, B), dim3(256), 0, (hipStream_t)stream,
                           valid, cnt, arg_m, arg_u, dmmax, dmavg, dumean, dumax, dpf_direct, N, C, npb, ldm, ldu, dpf);
    }
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

// ---- segmented (packed) entry points ----
static size_t seg_part_bytes(int nchunk, int C) { return ((size_t)nchunk * C * sizeof(PoolPart) + 255) & ~(size_t)255; }

extern "C" size_t wf3d_pool4_seg_ws_bytes(int nchunk, int C) {
    if (nchunk <= 0 || C <= 0) return 0;
    return seg_part_bytes(nchunk, C) + (size_t)nchunk * sizeof(float);
}

extern "C" int wf3d_pool4_seg_fwd(const float* pf, const float* valid, const int32_t* rows, const int32_t* cchunk,
                                  const int32_t* chunks, int B, int M, int nchunk, int C, float* mmax, float* mavg,
                                  float* umean, float* umax, int ldo, int32_t* arg_m, int32_t* arg_u, float* cnt,
                                  float* nvalid, void* ws, size_t ws_bytes, void* stream) {
    WF3D_CHECK(ldo >= C, WF3D_ERR_ARG, "wf3d_pool4_seg_fwd: ldo=%d < C=%d", ldo, C);
    WF3D_CHECK(B > 0 && M >= B && C > 0 && nchunk >= B, WF3D_ERR_ARG, "wf3d_pool4_seg_fwd: bad dims B=%d M=%d C=%d nchunk=%d", B, M, C, nchunk);
    WF3D_CHECK(B <= 65535 && nchunk <= 65535, WF3D_ERR_UNSUPPORTED, "wf3d_pool4_seg_fwd: more than 65535 clouds or chunks");
    WF3D_CHECK(pf && valid && rows && cchunk && chunks && mmax && mavg && umean && umax && arg_m && arg_u && cnt, WF3D_ERR_ARG,
               "wf3d_pool4_seg_fwd: null pointer");
    WF3D_CHECK((uintptr_t)chunks % 16 == 0, WF3D_ERR_ARG, "wf3d_pool4_seg_fwd: the chunk table must be 16-byte aligned");
    WF3D_CHECK(ws && ws_bytes >= wf3d_pool4_seg_ws_bytes(nchunk, C), WF3D_ERR_WS, "wf3d_pool4_seg_fwd: workspace too small");
    PoolPart* part = (PoolPart*)ws;
    float* cnt_part = (float*)((char*)ws + seg_part_bytes(nchunk, C));
    hipStream_t st = (hipStream_t)stream;
    if (pool_v4(pf, C))
        hipLaunchKernelGGL(pool4_seg_partial_kernel<true>, dim3(C / 64, nchunk), dim3(256), 0, st, pf, valid, rows, chunks, B, M, C, part, cnt_part);
    else
        hipLaunchKernelGGL(pool4_seg_partial_kernel<false>, dim3(wf3d_cdiv(C, 256), nchunk), dim3(256), 0, st, pf, valid, rows, chunks, B, M, C, part, cnt_part);
    WF3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(pool4_seg_final_kernel, dim3(wf3d_cdiv(C, 256), B), dim3(256), 0, st, part, cnt_part, rows, cchunk, nchunk, C, ldo,
                       nvalid, mmax, mavg, umean, umax, arg_m, arg_u, cnt);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

static int pool4_seg_bwd_impl(const float* valid, const float* cnt, const int32_t* arg_m, const int32_t* arg_u,
                              const float* dmmax, const float* dmavg, int ldm, const float* dumean, const float* dumax, int ldu,
                              const float* dpf_direct, const int32_t* rows, const int32_t* chunks, int B, int M, int M_pad,
                              int nchunk, int chunk_rows, int C, float* dpf, bool sx8, void* stream) {
    WF3D_CHECK(B > 0 && M >= B && M_pad >= M && C > 0 && nchunk >= B && chunk_rows > 0 && B <= 65535 && nchunk <= 65535, WF3D_ERR_ARG,
               "wf3d_pool4_seg_bwd: bad dims B=%d M=%d M_pad=%d C=%d nchunk=%d chunk_rows=%d", B, M, M_pad, C, nchunk, chunk_rows);
    WF3D_CHECK(valid && cnt && arg_m && arg_u && rows && chunks && dpf, WF3D_ERR_ARG, "wf3d_pool4_seg_bwd: null pointer");
    WF3D_CHECK((uintptr_t)chunks % 16 == 0, WF3D_ERR_ARG, "wf3d_pool4_seg_bwd: the chunk table must be 16-byte aligned");
    const auto al = [](const float* p, int ld) { return !p || ((uintptr_t)p % 16 == 0 && ld % 4 == 0); };
    const bool vec = C % 4 == 0 && ((uintptr_t)dpf % 16 == 0) && (!dpf_direct || (uintptr_t)dpf_direct % 16 == 0) &&
                     al(dmmax, ldm) && al(dmavg, ldm) && al(dumean, ldu) && al(dumax, ldu);
    WF3D_CHECK(!sx8 || (vec && C % 8 == 0), WF3D_ERR_UNSUPPORTED, "wf3d_pool4_seg_bwd_sx8: needs C %% 8 == 0 and 16-B aligned tensors (C=%d)", C);
    // as the dense launch: about 4096 workgroups, at least 16 rows each
    const int cb = vec ? wf3d_cdiv(C / 4, 256) : wf3d_cdiv(C, 256);
    int ns = 4096 / (nchunk * cb);
    const int cap = wf3d_cdiv(chunk_rows, 16);
    ns = ns > cap ? cap : (ns < 1 ? 1 : ns);
    const dim3 grid(cb, ns, nchunk);
    hipStream_t st = (hipStream_t)stream;
#define WF3D_SEG_BWD(MODE) hipLaunchKernelGGL(pool4_seg_bwd_kernel<MODE>, grid, dim3(256), 0, st, valid, cnt, arg_m, arg_u, dmmax, dmavg, \
                                              dumean, dumax, dpf_direct, rows, chunks, B, M, M_pad, C, ldm, ldu, dpf, \
                                              wf3d_live_rows())
    if (!vec) WF3D_SEG_BWD(2);
    else if (sx8) WF3D_SEG_BWD(1);
    else WF3D_SEG_BWD(0);
#undef WF3D_SEG_BWD
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" int wf3d_pool4_seg_bwd(const float* valid, const float* cnt, const int32_t* arg_m, const int32_t* arg_u,
                                  const float* dmmax, const float* dmavg, int ldm, const float* dumean, const float* dumax,
                                  int ldu, const float* dpf_direct, const int32_t* rows, const int32_t* chunks, int B, int M,
                                  int M_pad, int nchunk, int chunk_rows, int C, float* dpf, void* stream) {
    return pool4_seg_bwd_impl(valid, cnt, arg_m, arg_u, dmmax, dmavg, ldm, dumean, dumax, ldu, dpf_direct, rows, chunks, B, M,
                              M_pad, nchunk, chunk_rows, C, dpf, false, stream);
}

extern "C" int wf3d_pool4_seg_bwd_sx8(const float* valid, const float* cnt, const int32_t* arg_m, const int32_t* arg_u,
                                      const float* dmmax, const float* dmavg, int ldm, const float* dumean, const float* dumax,
                                      int ldu, const float* dpf_direct, const int32_t* rows, const int32_t* chunks, int B, int M,
                                      int M_pad, int nchunk, int chunk_rows, int C, float* dpf_sx8, void* stream) {
    return pool4_seg_bwd_impl(valid, cnt, arg_m, arg_u, dmmax, dmavg, ldm, dumean, dumax, ldu, dpf_direct, rows, chunks, B, M,
                              M_pad, nchunk, chunk_rows, C, dpf_sx8, true, stream);
}

// ---- the chunk table of a row capacity, built on the device ----
extern "C" int wf3d_packed_layout_dims(int B, int capacity, int* chunk_rows, int* nchunk_cap) {
    WF3D_CHECK(B > 0 && B <= 65535, WF3D_ERR_ARG, "wf3d_packed_layout_dims: B=%d not in 1..65535", B);
    WF3D_CHECK(capacity > 0 && capacity % 256 == 0, WF3D_ERR_ARG, "wf3d_packed_layout_dims: capacity=%d is not a positive multiple of 256", capacity);
    WF3D_CHECK(chunk_rows && nchunk_cap, WF3D_ERR_ARG, "wf3d_packed_layout_dims: null pointer");
    *chunk_rows = packed_chunk_rows(capacity);
    *nchunk_cap = wf3d_cdiv(capacity, *chunk_rows) + B + 1;
    return WF3D_OK;
}

template <typename CountT>
static int packed_layout_build_impl(const CountT* counts, int B, int capacity, int32_t* rows, int32_t* cchunk,
                                    int32_t* chunks, int32_t* status, void* stream) {
    int chunk_rows = 0, nchunk_cap = 0;
    const int rc = wf3d_packed_layout_dims(B, capacity, &chunk_rows, &nchunk_cap);
    if (rc != WF3D_OK) return rc;
    WF3D_CHECK(counts && rows && cchunk && chunks && status, WF3D_ERR_ARG, "wf3d_packed_layout_build: null pointer");
    WF3D_CHECK((uintptr_t)chunks % 16 == 0, WF3D_ERR_ARG, "wf3d_packed_layout_build: the chunk table must be 16-byte aligned");
    hipLaunchKernelGGL(packed_layout_kernel<CountT>, dim3(1), dim3(256), 0, (hipStream_t)stream, counts, B, capacity,
                       chunk_rows, nchunk_cap, rows, cchunk, chunks, status);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" int wf3d_packed_layout_build(const int64_t* counts, int B, int capacity, int32_t* rows, int32_t* cchunk,
                                        int32_t* chunks, int32_t* status, void* stream) {
    return packed_layout_build_impl(counts, B, capacity, rows, cchunk, chunks, status, stream);
}

extern "C" int wf3d_packed_layout_build_i32(const int32_t* counts, int B, int capacity, int32_t* rows, int32_t* cchunk,
                                            int32_t* chunks, int32_t* status, void* stream) {
    return packed_layout_build_impl(counts, B, capacity, rows, cchunk, chunks, status, stream);
}

// ---- streaming pool ----
extern "C" size_t wf3d_pool4_stream_state_bytes(int B, int C) {
    if (B <= 0 || C <= 0) return 0;
    return (size_t)B * C * sizeof(f32x4) + (size_t)B * sizeof(float);
}

extern "C" int wf3d_pool4_stream_init(void* state, int B, int C, void* stream) {
    WF3D_CHECK(B > 0 && C > 0 && B <= 65535, WF3D_ERR_ARG, "wf3d_pool4_stream_init: bad dims B=%d C=%d", B, C);
    WF3D_CHECK(state && (uintptr_t)state % 16 == 0, WF3D_ERR_ARG, "wf3d_pool4_stream_init: null or misaligned state");
    const long n = (long)B * C;
    hipLaunchKernelGGL(pool4_stream_init_kernel, dim3(wf3d_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (f32x4*)state,
                       (float*)((f32x4*)state + n), n, B);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" size_t wf3d_pool4_stream_ws_bytes(int rows, int C) {
    if (rows <= 0 || C <= 0) return 0;
    const int ns = wf3d_cdiv(rows, stream_spr(rows, C));
    return stream_part_bytes(ns, C) + (size_t)ns * sizeof(float);
}

extern "C" int wf3d_pool4_stream(const float* pf, const float* valid, const int32_t* offsets, int B, int r0, int rows, int C,
                                 void* state, void* ws, size_t ws_bytes, void* stream) {
    WF3D_CHECK(B > 0 && C > 0 && B <= 65535 && r0 >= 0 && rows >= 0 && (long)r0 + rows <= 0x7FFFFFFFL, WF3D_ERR_ARG,
               "wf3d_pool4_stream: bad dims B=%d C=%d r0=%d rows=%d", B, C, r0, rows);
    if (rows == 0) return WF3D_OK;
    WF3D_CHECK(pf && valid && offsets && state && (uintptr_t)state % 16 == 0, WF3D_ERR_ARG,
               "wf3d_pool4_stream: null pointer or misaligned state");
    WF3D_CHECK(ws && (uintptr_t)ws % 16 == 0 && ws_bytes >= wf3d_pool4_stream_ws_bytes(rows, C), WF3D_ERR_WS,
               "wf3d_pool4_stream: workspace too small or misaligned");
    const int spr = stream_spr(rows, C);
    const int ns = wf3d_cdiv(rows, spr);
    WF3D_CHECK(ns <= 65535, WF3D_ERR_UNSUPPORTED, "wf3d_pool4_stream: more than 65535 slices (rows=%d)", rows);
    f32x4* part = (f32x4*)ws;
    float* cnt_part = (float*)((char*)ws + stream_part_bytes(ns, C));
    f32x4* st = (f32x4*)state;
    float* cnt_state = (float*)(st + (size_t)B * C);
    hipStream_t s = (hipStream_t)stream;
    if (pool_v4(pf, C))
        hipLaunchKernelGGL(pool4_stream_partial_kernel<true>, dim3(C / 64, ns), dim3(256), 0, s, pf, valid, offsets, B, r0, rows,
                           spr, C, part, cnt_part);
    else
        hipLaunchKernelGGL(pool4_stream_partial_kernel<false>, dim3(wf3d_cdiv(C, 256), ns), dim3(256), 0, s, pf, valid, offsets,
                           B, r0, rows, spr, C, part, cnt_part);
    WF3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(pool4_stream_fold_kernel, dim3(wf3d_cdiv(C, 256), B), dim3(256), 0, s, pf, valid, offsets, B, r0, rows,
                       spr, C, part, cnt_part, st, cnt_state);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" int wf3d_pool4_stream_finish(const void* state, const int32_t* offsets, int B, int C, float* mmax, float* mavg,
                                        float* umean, float* umax, int ldo, float* cnt, float* nvalid, void* stream) {
    WF3D_CHECK(ldo >= C, WF3D_ERR_ARG, "wf3d_pool4_stream_finish: ldo=%d < C=%d", ldo, C);
    WF3D_CHECK(B > 0 && C > 0 && B <= 65535, WF3D_ERR_ARG, "wf3d_pool4_stream_finish: bad dims B=%d C=%d", B, C);
    WF3D_CHECK(state && (uintptr_t)state % 16 == 0 && offsets && mmax && mavg && umean && umax && cnt, WF3D_ERR_ARG,
               "wf3d_pool4_stream_finish: null pointer or misaligned state");
    const f32x4* st = (const f32x4*)state;
    hipLaunchKernelGGL(pool4_stream_finish_kernel, dim3(wf3d_cdiv(C, 256), B), dim3(256), 0, (hipStream_t)stream, st,
                       (const float*)(st + (size_t)B * C), offsets, C, ldo, mmax, mavg, umean, umax, cnt, nvalid);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}
