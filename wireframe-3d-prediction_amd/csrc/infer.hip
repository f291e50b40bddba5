// Forward-only encoder (wf3d.infer): the two kernels the block walk needs beyond the training forward's.
//
// Streaming 4-way pool.  The per-point MLP runs over one block of rows [r0, r0 + rows) of the flat row space at a time;
// the pools are a running state per (cloud, channel) that each block is folded into as it passes:
//     state[b * C + c] = (masked sum, unmasked sum, masked max, unmasked max)      one 16-byte piece
//     cnt[b]           = valid rows seen so far                                    behind the B * C pieces
// The cloud of a row comes from the int32 device table of B + 1 row offsets (a packed layout's `rows`; b * N for a dense
// batch), which only the kernels read.  A block may start and end anywhere.  It is cut into slices of `spr` rows:
//   - pool4_stream_partial_kernel reduces every slice that lies inside ONE cloud to one partial per channel, in the
//     shape of pool4_partial_v4_kernel (pool.hip): 16 bytes per lane, four loads in flight, a shuffle tree over the
//     wave's four row groups, an LDS tree over the four waves (C % 64 == 0), or thread = channel for any other C;
//   - pool4_stream_fold_kernel has ONE owner thread per (cloud, channel): it walks the slices that hold rows of its
//     cloud in ascending row order and adds the slice's partial — or, for a slice that straddles a cloud boundary or the
//     end of the live rows (at most two per cloud and block, `spr` rows each), the cloud's rows of that slice read
//     directly — into the state.  No atomics: the summation order is a function of (offsets, r0, rows, C) alone.
// Rows at or past offsets[B] belong to no cloud and are never read.  No arg-max is kept: nothing reads it without a
// backward.
//
// First layer without z.  first_layer_infer_kernel is first_layer_kernel (split.hip) with the stores of z, mu and rs
// taken out: the same expressions in the same order, so its h is that kernel's h_sx8 bit for bit.
//
// Forward-only edge head (wf3d.infer.edge_stream).  pair_infer_kernel is pair_fwd_kernel (edge.hip) over the edge rows
// [e0, e0 + n) of a layout, written into block buffers indexed by e - e0, without the stores nobody reads and without
// dropout: the same expressions in the same order, so its outputs are that kernel's rows bit for bit.
// block_live_kernel cuts a layout's live edge-row total into one count per block of the walk.
#include "wf3d_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// streaming pool
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

struct Stream4 { f32x4 msum, usum, mmax, umax; };            // running state of 4 channels

__device__ __forceinline__ f32x4 max4(const f32x4& a, const f32x4& o) {
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = o[e] > a[e] ? o[e] : a[e];
    return r;
}

__device__ __forceinline__ void stream4_merge(Stream4& a, const Stream4& o) {
    a.msum += o.msum;
    a.usum += o.usum;
    a.mmax = max4(a.mmax, o.mmax);
    a.umax = max4(a.umax, o.umax);
}

__device__ __forceinline__ Stream4 stream4_shfl_xor(const Stream4& a, int mask) {
    Stream4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        o.msum[e] = __shfl_xor(a.msum[e], mask, 64); o.usum[e] = __shfl_xor(a.usum[e], mask, 64);
        o.mmax[e] = __shfl_xor(a.mmax[e], mask, 64); o.umax[e] = __shfl_xor(a.umax[e], mask, 64);
    }
    return o;
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
    if (V4) {
        __shared__ Stream4 s_p[3][16];
        __shared__ float s_cnt[4];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int rsub = lane >> 4, c = blockIdx.x * 64 + (lane & 15) * 4;
        Stream4 a;
        a.msum = a.usum = f32x4{0.f, 0.f, 0.f, 0.f};
        a.mmax = a.umax = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        float cnt = 0.f;
        const float* base = pf + c;
        constexpr int U = 4;                               // 4 independent 16-B loads per lane in flight
        for (int n = n0 + wave * 4 + rsub; n < n1; n += 16 * U) {
            f32x4 v[U];
            float ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int nn = n + 16 * u;
                if (nn < n1) { v[u] = *reinterpret_cast<const f32x4*>(base + (size_t)nn * C); ok[u] = valid[nn]; }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int nn = n + 16 * u;
                if (nn < n1) {
                    a.usum += v[u];
                    a.umax = max4(a.umax, v[u]);
                    if (ok[u] != 0.f) {
                        a.msum += v[u];
                        cnt += 1.f;
                        a.mmax = max4(a.mmax, v[u]);
                    }
                }
            }
        }
        // wavefront shuffle tree over the wave's 4 row groups
        stream4_merge(a, stream4_shfl_xor(a, 16));
        stream4_merge(a, stream4_shfl_xor(a, 32));
        cnt += __shfl_xor(cnt, 16, 64);
        cnt += __shfl_xor(cnt, 32, 64);
        // LDS tree over the 4 waves
        if (wave > 0 && lane < 16) s_p[wave - 1][lane] = a;
        if (lane == 0) s_cnt[wave] = cnt;
        __syncthreads();
        if (wave == 0 && lane < 16) {
            stream4_merge(a, s_p[0][lane]);
            stream4_merge(a, s_p[1][lane]);
            stream4_merge(a, s_p[2][lane]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                part[(size_t)s * C + c + e] = f32x4{a.msum[e], a.usum[e], a.mmax[e], a.umax[e]};
            if (blockIdx.x == 0 && lane == 0) cnt_part[s] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        }
    } else {
        const int c = blockIdx.x * 256 + threadIdx.x;
        float msum = 0.f, usum = 0.f, mmax = -INFINITY, umax = -INFINITY, cnt = 0.f;
        if (c < C) {
            const float* p = pf + (size_t)n0 * C + c;
            for (int n = n0; n < n1; ++n, p += C) {
                const float v = *p;
                usum += v;
                umax = v > umax ? v : umax;
                if (valid[n] != 0.f) { msum += v; cnt += 1.f; mmax = v > mmax ? v : mmax; }
            }
            part[(size_t)s * C + c] = f32x4{msum, usum, mmax, umax};
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) cnt_part[s] = cnt;       // channel 0 exists: every thread counts the same rows
    }
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
            float msum = 0.f, usum = 0.f, mmax = -INFINITY, umax = -INFINITY, k = 0.f;
            for (long n = a - r0; n < e - r0; ++n) {
                const float v = pf[(size_t)n * C + c];
                usum += v;
                umax = v > umax ? v : umax;
                if (valid[n] != 0.f) { msum += v; k += 1.f; mmax = v > mmax ? v : mmax; }
            }
            st[0] += msum; st[1] += usum;
            st[2] = mmax > st[2] ? mmax : st[2];
            st[3] = umax > st[3] ? umax : st[3];
            cnt += k;
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

// grid (ceil(C / 256), B): what pool4_final_cloud (pool.hip) writes, without the arg-max rows
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

bool stream_v4(const float* pf, int C) { return C % 64 == 0 && (uintptr_t)pf % 16 == 0; }

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

// ---------------------------------------------------------------------------------------------------------------------
// first layer without z
// ---------------------------------------------------------------------------------------------------------------------
// first_layer_kernel (split.hip) without the stores of z, mu and rs: one wave per row computes the row in registers from
// its slice of W (kept in registers across rows) and writes h = act(LN(x·W^T + b)) in sx8.  Every expression that
// reaches h is that kernel's, in its order.
// FAST: K == 8, D a multiple of 512, 16-byte aligned x / W rows and ReLU.
template <int NS, bool FAST>
__global__ __launch_bounds__(256) void first_layer_infer_kernel(const float* __restrict__ x, int ldx, int K,
                                                                 const float* __restrict__ W, int ldw,
                                                                 const float* __restrict__ bias, int R, int D,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 int act, float eps, float* __restrict__ h_sx8) {
    if (R == 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool odd = lane & 1;
    // columns of a lane, slot i: [512 i + 4 lane, +4) (values 0..3) and [512 i + 256 + 4 lane, +4) (values 4..7)
    auto col = [&](int i, int j) { return 512 * i + 256 * (j >> 2) + lane * 4 + (j & 3); };
    float w[NS][8][8], b[NS][8], gm[NS][8], bt[NS][8];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        if (FAST) {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int c = col(i, 4 * hf);
                const f32x4 g4 = *reinterpret_cast<const f32x4*>(gamma + c), b4 = *reinterpret_cast<const f32x4*>(beta + c);
                f32x4 bb = {0.f, 0.f, 0.f, 0.f};
                if (bias) bb = *reinterpret_cast<const f32x4*>(bias + c);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    gm[i][4 * hf + j] = g4[j]; bt[i][4 * hf + j] = b4[j]; b[i][4 * hf + j] = bb[j];
                    const f32x4 w0 = *reinterpret_cast<const f32x4*>(W + (size_t)(c + j) * ldw), w1 = *reinterpret_cast<const f32x4*>(W + (size_t)(c + j) * ldw + 4);
#pragma unroll
                    for (int k = 0; k < 4; ++k) { w[i][4 * hf + j][k] = w0[k]; w[i][4 * hf + j][4 + k] = w1[k]; }
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = col(i, j);
                b[i][j] = (c < D && bias) ? bias[c] : 0.f;
                gm[i][j] = c < D ? gamma[c] : 1.f;
                bt[i][j] = c < D ? beta[c] : 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) w[i][j][k] = (c < D && k < K) ? W[(size_t)c * ldw + k] : 0.f;
            }
        }
    }
    // the next row's x is requested before this row is computed and stored
    auto load_x = [&](int row, float (&xr)[8]) {
        if (FAST) {
            const float* px = x + (size_t)min(row, R - 1) * ldx;           // clamped: the value of a row >= R is never used
            const f32x4 a = *reinterpret_cast<const f32x4*>(px), c4 = *reinterpret_cast<const f32x4*>(px + 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) { xr[k] = a[k]; xr[4 + k] = c4[k]; }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) xr[k] = (row < R && k < K) ? x[(size_t)row * ldx + k] : 0.f;
        }
    };
    float xn[8];
    load_x(blockIdx.x * 4 + wave, xn);
    for (int row = blockIdx.x * 4 + wave; row < R; row += gridDim.x * 4) {
        float xr[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) xr[k] = xn[k];
        load_x(row + gridDim.x * 4, xn);
        float v[NS][8];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float a = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) a = fmaf(xr[k], w[i][j][k], a);
                v[i][j] = (FAST || col(i, j) < D) ? a + b[i][j] : 0.f;
                s += v[i][j];
            }
        }
        const float mean = wf3d_wave_sum(s) / (float)D;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (FAST || col(i, j) < D) { const float d = v[i][j] - mean; q += d * d; }
        const float rstd = 1.0f / sqrtf(wf3d_wave_sum(q) / (float)D + eps);
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int c = col(i, 4 * hf);
                if (FAST || c < D) {               // D % 8 == 0: both lanes of a pair are in or out together
                    float o[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float y0 = (v[i][4 * hf + j] - mean) * rstd * gm[i][4 * hf + j] + bt[i][4 * hf + j];
                        o[j] = FAST ? fmaxf(y0, 0.f) : wf3d_act_rt(act, y0);
                    }
                    wf3d_store_sx8_pair(h_sx8 + (size_t)row * D + c, o, odd);
                }
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// forward-only edge head
// ---------------------------------------------------------------------------------------------------------------------
// pair_fwd_kernel (edge.hip) with a row origin: one wave per 8 consecutive edge rows e0 + l, l in [l0, l0 + 8), of the
// layout; every output is indexed by the block-local row l.  e0 % 8 == 0, so a wave's 8 rows are the 8 rows one wave of
// pair_fwd_kernel walks.  Two forms, by the pointers given:
//   h_sx8        : h = act(LN(pre)) as the sx8 operand alone (split route); pre, mu, rs are NULL
//   pre, mu, rs  : the pre-activation and its row statistics (fp32 route); h_sx8 is NULL
// No delta (only a backward reads it), no dropout.  `live_rows` is the BLOCK's live-row count: rows l at or past its
// 256-row extent are neither read (esample) nor written.  Nothing at or past row n is touched.
template <int NS>
__global__ __launch_bounds__(256) void pair_infer_kernel(const float* __restrict__ Pa, const float* __restrict__ Pb,
                                                          const float* __restrict__ cv, const float* __restrict__ wd,
                                                          int wd_stride, const int32_t* __restrict__ voff,
                                                          const int32_t* __restrict__ eoff,
                                                          const int32_t* __restrict__ esample, int e0, int n, int H,
                                                          float eps, float* __restrict__ pre, float* __restrict__ mu,
                                                          float* __restrict__ rs, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, int act,
                                                          float* __restrict__ h_sx8, int vd,
                                                          const int32_t* __restrict__ live_rows) {
    constexpr int EPW = 8;
    n = wf3d_live_extent(live_rows, n);
    const int lane = threadIdx.x & 63;
    const int l0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * EPW;
    if (l0 >= n) return;
    const int l1 = min(n, l0 + EPW);
    f32x4 wdv[NS], g4[NS], b4[NS], pa[NS];
#pragma unroll
    for (int t = 0; t < NS; ++t) {
        const int c = lane * 4 + 256 * t;
        wdv[t] = g4[t] = b4[t] = pa[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (c < H) {
#pragma unroll
            for (int k = 0; k < 4; ++k) wdv[t][k] = wd[(size_t)(c + k) * wd_stride];
            if (h_sx8) { g4[t] = *reinterpret_cast<const f32x4*>(gamma + c); b4[t] = *reinterpret_cast<const f32x4*>(beta + c); }
        }
    }
    // rows la..l1-1 of a padded layout's tail (contiguous, so the rest of this wave's rows): zeros in every output
    auto zero_tail = [&](int la) {
        for (int l = la; l < l1; ++l) {
#pragma unroll
            for (int t = 0; t < NS; ++t) {
                const int c = lane * 4 + 256 * t;
                if (c < H) {
                    if (pre) *reinterpret_cast<f32x4*>(pre + (size_t)l * H + c) = (f32x4){0.f, 0.f, 0.f, 0.f};
                    if (h_sx8) *reinterpret_cast<f32x4*>(h_sx8 + (size_t)l * H + c) = (f32x4){0.f, 0.f, 0.f, 0.f};
                }
            }
            if (pre && lane == 0) { mu[l] = 0.f; rs[l] = 0.f; }
        }
    };
    int s = esample[e0 + l0];
    if (s < 0) { zero_tail(l0); return; }
    int vbase = voff[s], v = voff[s + 1] - vbase, eend = eoff[s + 1];
    int i, j;
    edge_ij(e0 + l0 - eoff[s], v, i, j);                   // a block, like a wave, may start in the middle of a sample
    int pa_row = -1;
    for (int l = l0; l < l1; ++l) {
        const int e = e0 + l;
        if (e == eend) {                       // first edge of the next sample that has edges
            s = esample[e];
            if (s < 0) { zero_tail(l); return; }
            vbase = voff[s]; v = voff[s + 1] - vbase; eend = eoff[s + 1];
            i = 0; j = 1;
        }
        const int ri = vbase + i, rj = vbase + j;
        float dl2 = 0.f;                                   // |c_i - c_j|^2 over the vd coordinates, in pair_fwd_kernel's order
        for (int k = 0; k < vd; ++k) { const float d = cv[ri * vd + k] - cv[rj * vd + k]; dl2 = fmaf(d, d, dl2); }
        const float dl = sqrtf(dl2);
        f32x4 val[NS];
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            const int c = lane * 4 + 256 * t;
            val[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (c < H) {
                if (ri != pa_row) pa[t] = *reinterpret_cast<const f32x4*>(Pa + (size_t)ri * H + c);
                const f32x4 b = *reinterpret_cast<const f32x4*>(Pb + (size_t)rj * H + c);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    val[t][k] = pa[t][k] + b[k] + dl * wdv[t][k];
                    sum += val[t][k];
                }
                if (pre) *reinterpret_cast<f32x4*>(pre + (size_t)l * H + c) = val[t];
            }
        }
        pa_row = ri;
        const float mean = wf3d_wave_sum(sum) / (float)H;
        float q = 0.f;
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            const int c = lane * 4 + 256 * t;
            if (c < H) {
#pragma unroll
                for (int k = 0; k < 4; ++k) { const float d = val[t][k] - mean; q += d * d; }
            }
        }
        const float var = wf3d_wave_sum(q) / (float)H;
        const float rstd = 1.0f / sqrtf(var + eps);
        if (pre && lane == 0) {
            mu[l] = mean;
            rs[l] = rstd;
        }
        if (h_sx8) {
#pragma unroll
            for (int t = 0; t < NS; ++t) {
                const int c = lane * 4 + 256 * t;
                if (c < H) {
                    float o[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] = wf3d_act_rt(act, (val[t][k] - mean) * rstd * g4[t][k] + b4[t][k]);
                    // sx8 group = 8 columns = lanes (2m, 2m+1): even lane stores the 8 high parts, odd lane the 8 low parts
                    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
                    bf16x4 hi, lo;
#pragma unroll
                    for (int k = 0; k < 4; ++k) { hi[k] = (__bf16)o[k]; lo[k] = (__bf16)(o[k] - (float)hi[k]); }
                    const uint2 mine_hi = __builtin_bit_cast(uint2, hi), mine_lo = __builtin_bit_cast(uint2, lo);
                    const bool odd = lane & 1;
                    uint2 send = odd ? mine_hi : mine_lo, got;
                    got.x = __shfl_xor((int)send.x, 1, 64);
                    got.y = __shfl_xor((int)send.y, 1, 64);
                    const uint4 w = odd ? make_uint4(got.x, got.y, mine_lo.x, mine_lo.y) : make_uint4(mine_hi.x, mine_hi.y, got.x, got.y);
                    *reinterpret_cast<uint4*>(h_sx8 + (size_t)l * H + (c & ~7) + (odd ? 4 : 0)) = w;
                }
            }
        }
        if (++j == v) { ++i; j = i + 1; }
    }
}

// blive[k] = clamp(*total - k * rows, 0, min(rows, Re - k * rows)): the live rows of block k of the walk
__global__ __launch_bounds__(256) void block_live_kernel(const int32_t* __restrict__ total, int rows, int Re, int nblocks,
                                                          int32_t* __restrict__ blive) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nblocks) return;
    const long r0 = (long)k * rows;
    const long cap = max(0L, min((long)rows, (long)Re - r0));
    blive[k] = (int32_t)min(max((long)*total - r0, 0L), cap);
}

}  // namespace

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
    if (stream_v4(pf, C))
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

extern "C" int wf3d_first_layer_infer(const float* x, int R, int K, int ldx, const float* W, int ldw, const float* bias,
                                      int D, const float* gamma, const float* beta, int act, float eps, void* h_sx8,
                                      void* stream) {
    WF3D_CHECK(R >= 0 && K > 0 && K <= 8 && ldx >= K && ldw >= K, WF3D_ERR_UNSUPPORTED,
               "wf3d_first_layer_infer: needs 1 <= K <= 8 (K=%d)", K);
    WF3D_CHECK(D > 0 && D % 8 == 0 && D <= 1024, WF3D_ERR_UNSUPPORTED, "wf3d_first_layer_infer: D=%d must be a multiple of 8, <= 1024", D);
    WF3D_CHECK(act >= 0 && act <= 2, WF3D_ERR_ARG, "wf3d_first_layer_infer: bad act");
    if (R == 0) return WF3D_OK;
    WF3D_CHECK(x && W && gamma && beta && h_sx8, WF3D_ERR_ARG, "wf3d_first_layer_infer: null pointer");
    WF3D_CHECK(((uintptr_t)h_sx8 % 16 == 0) && ((uintptr_t)gamma % 16 == 0) && ((uintptr_t)beta % 16 == 0), WF3D_ERR_ARG,
               "wf3d_first_layer_infer: pointers must be 16-byte aligned");
    // the grid of wf3d_first_layer_fwd
    int blocks = wf3d_cdiv(R, 4);
    blocks = blocks > 4096 ? 4096 : (blocks < 1 ? 1 : blocks);
    hipStream_t st = (hipStream_t)stream;
    const bool fast = K == 8 && ldx % 4 == 0 && ((uintptr_t)x % 16 == 0) && act == WF3D_ACT_RELU && D % 512 == 0 && ldw % 4 == 0 &&
                      ((uintptr_t)W % 16 == 0) && (!bias || (uintptr_t)bias % 16 == 0);
#define WF3D_FLI(NS_, F_)                                                                                                  \
    hipLaunchKernelGGL((first_layer_infer_kernel<NS_, F_>), dim3(blocks), dim3(256), 0, st, x, ldx, K, W, ldw, bias, R, D, \
                       gamma, beta, act, eps, (float*)h_sx8)
    if (D <= 512) { if (fast) WF3D_FLI(1, true); else WF3D_FLI(1, false); }
    else          { if (fast) WF3D_FLI(2, true); else WF3D_FLI(2, false); }
#undef WF3D_FLI
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" int wf3d_edge_pair_infer(const float* Pa, const float* Pb, const float* cv, const float* wdelta,
                                    int wdelta_stride, const int32_t* voff, const int32_t* eoff, const int32_t* esample,
                                    int e0, int n, int H, int vd, float eps, const float* gamma, const float* beta, int act,
                                    float* pre, float* mu, float* rs, void* h_sx8, void* stream) {
    WF3D_CHECK(e0 >= 0 && e0 % 8 == 0 && n >= 0 && (long)e0 + n <= 0x7FFFFFFFL, WF3D_ERR_ARG,
               "wf3d_edge_pair_infer: bad rows e0=%d n=%d (e0 must be a non-negative multiple of 8)", e0, n);
    WF3D_CHECK(H > 0 && vd >= 1 && vd <= 8, WF3D_ERR_ARG, "wf3d_edge_pair_infer: bad dims (vertex_dim must be 1..8)");
    WF3D_CHECK(H % 4 == 0 && H <= 2048, WF3D_ERR_UNSUPPORTED, "wf3d_edge_pair_infer: hidden %d must be a multiple of 4, <= 2048", H);
    if (n == 0) return WF3D_OK;
    WF3D_CHECK(Pa && Pb && cv && wdelta && voff && eoff && esample, WF3D_ERR_ARG, "wf3d_edge_pair_infer: null pointer");
    const bool split = h_sx8 && !pre && !mu && !rs, fp32 = !h_sx8 && pre && mu && rs;
    WF3D_CHECK(split || fp32, WF3D_ERR_ARG, "wf3d_edge_pair_infer: give h_sx8 alone, or pre, mu and rs alone");
    if (split) {
        WF3D_CHECK(gamma && beta && act >= 0 && act <= 2, WF3D_ERR_ARG, "wf3d_edge_pair_infer: null gamma / beta or bad act");
        WF3D_CHECK(H % 8 == 0 && ((uintptr_t)h_sx8 % 16 == 0) && ((uintptr_t)gamma % 16 == 0) && ((uintptr_t)beta % 16 == 0),
                   WF3D_ERR_UNSUPPORTED, "wf3d_edge_pair_infer: needs hidden %% 8 == 0 and 16-byte aligned pointers");
    }
    const int ns = wf3d_cdiv(H, 256);
    hipStream_t st = (hipStream_t)stream;
#define WF3D_PI(NS_)                                                                                                   \
    hipLaunchKernelGGL((pair_infer_kernel<NS_>), dim3(wf3d_cdiv(n, 4 * 8)), dim3(256), 0, st, Pa, Pb, cv, wdelta,            \
                       wdelta_stride, voff, eoff, esample, e0, n, H, eps, pre, mu, rs, gamma, beta, act, (float*)h_sx8, vd,  \
                       wf3d_live_rows())
    if (ns <= 1) WF3D_PI(1); else if (ns <= 2) WF3D_PI(2); else if (ns <= 4) WF3D_PI(4); else WF3D_PI(8);
#undef WF3D_PI
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" int wf3d_block_live(const int32_t* total, int rows, int Re, int nblocks, int32_t* blive, void* stream) {
    WF3D_CHECK(rows > 0 && Re >= 0 && nblocks >= 0, WF3D_ERR_ARG, "wf3d_block_live: bad dims rows=%d Re=%d nblocks=%d", rows, Re, nblocks);
    if (nblocks == 0) return WF3D_OK;
    WF3D_CHECK(total && blive, WF3D_ERR_ARG, "wf3d_block_live: null pointer");
    hipLaunchKernelGGL(block_live_kernel, dim3(wf3d_cdiv(nblocks, 256)), dim3(256), 0, (hipStream_t)stream, total, rows, Re,
                       nblocks, blive);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}
