// Forward-only paths (wf3d.infer): the kernels the block walks need that have no training form.
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
// Forward-only edge head (wf3d.infer.edge_stream): block_live_kernel cuts a layout's live edge-row total into one count
// per block of the walk.
//
// The other two forward-only kernels are not here: wf3d_first_layer_infer is the !KEEP instantiation of
// first_layer_kernel (split.hip) and wf3d_edge_pair_infer that of pair_fwd_kernel (edge.hip), each beside the training
// entry point that shares its body.
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
// forward-only edge head
// ---------------------------------------------------------------------------------------------------------------------
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

extern "C" int wf3d_block_live(const int32_t* total, int rows, int Re, int nblocks, int32_t* blive, void* stream) {
    WF3D_CHECK(rows > 0 && Re >= 0 && nblocks >= 0, WF3D_ERR_ARG, "wf3d_block_live: bad dims rows=%d Re=%d nblocks=%d", rows, Re, nblocks);
    if (nblocks == 0) return WF3D_OK;
    WF3D_CHECK(total && blive, WF3D_ERR_ARG, "wf3d_block_live: null pointer");
    hipLaunchKernelGGL(block_live_kernel, dim3(wf3d_cdiv(nblocks, 256)), dim3(256), 0, (hipStream_t)stream, total, rows, Re,
                       nblocks, blive);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}
