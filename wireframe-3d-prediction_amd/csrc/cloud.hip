// Row f-3: the input pipeline in front of the hot path, datasets/building3d.py:95-190 of the reference —
// per sample: colour / 256, centroid + max-norm normalisation of xyz, random sampling of num_points rows, flip / z-rotation
// augmentation — as two kernels on clouds that stay resident in HBM.
//
//   cloud_normalize_kernel   once per cloud (when it is cached): raw float64 rows [n, C] (UTM coordinates ~6.5e6 m: fp32 cannot
//                            hold them) -> float64 normalised rows, centroid[3], max_distance; fp64 arithmetic in the
//                            reference's order (:118-121), one workgroup per cloud.
//   cloud_sample_kernel      per batch: out[b, p, :] = fp32(augment(norm[first[cloud[b]] + choice[b, p], :])) — the
//                            reference's gather (:127-128), flips and rotation about z (:130-145) on float64 values, rounded
//                            to fp32 once at the end like its final astype(np.float32) (:158).  The random choices and
//                            augmentation parameters come from the host, drawn from numpy in the reference's order, so a
//                            seeded run reproduces the reference's batches.
//   cloud_pack_kernel        per packed batch: whole clouds, in file order, one after the other into the [capacity, C] fp32
//                            input buffer of a captured step, with cloud_sample_kernel's augmentation; the rows behind
//                            the last cloud are written as zeros and point_counts[b] by the same launch.
//   wireframe_targets_kernel per packed batch: wf3d.targets.train_targets(..., full_width=True) from resident wireframes,
//                            one workgroup per sample.
//                            Both read one parameter block in device memory (include/wf3d.h), so a captured graph that
//                            holds the two launches serves every batch.
//   cloud_sample_dev kernels per fixed-size batch: cloud_sample_kernel's output with the random choice computed in the
//                            kernel (wf3d/sampling.py) from a seed word in device memory and the same parameter block:
//                            no per-point host data, capturable.
//   cloud_fps_kernel         per fixed-size batch: the same output with the rows chosen by farthest-point sampling
//                            (wf3d/sampling.py fps_indices), one workgroup per sample, the cloud in registers.
//   cloud_epoch_params_kernel per batch of a resident epoch: WRITES that parameter block and the seed words — which clouds
//                            (a keyed permutation per epoch, sharded over ranks), their augmentation, the row offsets —
//                            from a 16-byte state in device memory, so nothing of a batch is made on the host.
//   the `_ext` forms         cloud_sample_dev, cloud_fps, cloud_epoch_params and wireframe_targets once more with the
//                            augmentation extension (a random scale, per-point jitter, random point dropout;
//                            wf3d/sampling.py augment_point) as a compile-time form of the same bodies.
// Plus the host-side text parser for .xyz files (np.loadtxt replacement): wf3d_parse_floats.
#include <locale.h>
#include <stdio.h>
#include <stdlib.h>

#include <cmath>
#include <type_traits>

#include "wf3d_common.h"

namespace {

__device__ __forceinline__ double block_reduce_d(double v, double* s, bool take_max) {
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s[tid] = take_max ? fmax(s[tid], s[tid + o]) : s[tid] + s[tid + o];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

// one workgroup per cloud; `first` = row offsets of the packed clouds
__global__ __launch_bounds__(256) void cloud_normalize_kernel(const double* __restrict__ raw, const long* __restrict__ first,
                                                               int C, int color_lo, int color_hi, int normalize,
                                                               double* __restrict__ out, double* __restrict__ centroid,
                                                               double* __restrict__ max_distance) {
    __shared__ double s[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long r0 = first[b], n = first[b + 1] - r0;
    const double* in = raw + r0 * C;
    double* o = out + r0 * C;
    double cx = 0, cy = 0, cz = 0, md = 1.0;
    if (normalize) {
        double sx = 0, sy = 0, sz = 0;
        for (long i = tid; i < n; i += 256) { sx += in[i * C]; sy += in[i * C + 1]; sz += in[i * C + 2]; }
        cx = block_reduce_d(sx, s, false) / (double)n;
        cy = block_reduce_d(sy, s, false) / (double)n;
        cz = block_reduce_d(sz, s, false) / (double)n;
        double m = 0;
        for (long i = tid; i < n; i += 256) {
            const double x = in[i * C] - cx, y = in[i * C + 1] - cy, z = in[i * C + 2] - cz;
            m = fmax(m, sqrt(x * x + y * y + z * z));
        }
        md = block_reduce_d(m, s, true);
        if (tid == 0) { centroid[b * 3] = cx; centroid[b * 3 + 1] = cy; centroid[b * 3 + 2] = cz; max_distance[b] = md; }
    }
    for (long i = tid; i < n; i += 256) {
        for (int k = 0; k < C; ++k) {
            double v = in[i * C + k];
            if (k >= color_lo && k < color_hi) v = v / 256.0;                       // building3d.py:105,110
            if (normalize && k < 3) v = (v - (k == 0 ? cx : (k == 1 ? cy : cz))) / md;
            o[i * C + k] = v;
        }
    }
}

__global__ __launch_bounds__(256) void cloud_sample_kernel(const double* __restrict__ norm, const long* __restrict__ first,
                                                            const int* __restrict__ cloud, const int* __restrict__ choice,
                                                            const double* __restrict__ aug, int P, int C,
                                                            float* __restrict__ out) {
    const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const double* row = norm + (first[cloud[b]] + choice[(long)b * P + p]) * C;
    const double fx = aug[b * 4], fy = aug[b * 4 + 1], c = aug[b * 4 + 2], s = aug[b * 4 + 3];
    const double x = fx * row[0], y = fy * row[1];
    float* o = out + ((long)b * P + p) * C;
    o[0] = (float)(x * c - y * s);               // [x y z] . rotz(t)^T  (building3d.py:144)
    o[1] = (float)(x * s + y * c);
    for (int k = 2; k < C; ++k) o[k] = (float)row[k];
}

// ---- packed batches from resident clouds ------------------------------------------------------------------------------
// The parameter block of a batch of B samples (include/wf3d.h): aug [B, 4] doubles, cloud [B] ints, out_first [B + 1] ints.
struct BatchParams { const double* aug; const int* cloud; const int* out_first; };
__device__ __forceinline__ BatchParams batch_params(const void* params, int B) {
    const char* p = (const char*)params;
    return {(const double*)p, (const int*)(p + (size_t)B * 32), (const int*)(p + (size_t)B * 36)};
}

// the sample that owns output row r < out_first[B]: the last b with out_first[b] <= r (an empty sample owns nothing)
__device__ __forceinline__ int sample_of_row(const int* __restrict__ out_first, int B, int r) {
    int lo = 0, hi = B;                              // out_first[lo] <= r < out_first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (out_first[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// Source row of output row r, or -1 for a row that belongs to no cloud (it is written as zeros): rows from out_first[B]
// on, and — so that a block the host did not build can never make the kernel read outside `norm` — rows whose
// cloud index or position is outside the resident clouds.
__device__ __forceinline__ long pack_source_row(const BatchParams& P, const long* __restrict__ first, int B, int nclouds,
                                                int r, int& b) {
    if (r >= P.out_first[B]) return -1;
    b = sample_of_row(P.out_first, B, r);
    const int cl = P.cloud[b];
    if (cl < 0 || cl >= nclouds) return -1;
    const long k = r - P.out_first[b], r0 = first[cl];       // k < 0: a row in front of out_first[0] > 0
    return k >= 0 && k < first[cl + 1] - r0 ? r0 + k : -1;
}

__device__ __forceinline__ void pack_counts(const BatchParams& P, const long* __restrict__ first, int B, int nclouds, long t,
                                            int64_t* __restrict__ point_counts) {
    if (t < B) {
        const int cl = P.cloud[t];
        point_counts[t] = cl >= 0 && cl < nclouds ? first[cl + 1] - first[cl] : 0;
    }
}

// C = 8: a row is 64 B of float64 in, 32 B of fp32 out.  Two lanes per row: the even lane loads x y | z r (two 16-B
// loads, 32 contiguous bytes), the odd lane g b | a i, each stores its four fp32 as one 16-B store — consecutive lanes
// write consecutive 16 bytes, a wave reads 2 KiB and writes 1 KiB contiguous, and x and y (the rotation's operands) sit
// in one lane.
typedef double f64x2 __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(256) void cloud_pack8_kernel(const double* __restrict__ norm, const long* __restrict__ first,
                                                           int nclouds, const void* __restrict__ params, int B, int capacity,
                                                           float* __restrict__ out, int64_t* __restrict__ point_counts) {
    const BatchParams P = batch_params(params, B);
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    pack_counts(P, first, B, nclouds, t, point_counts);
    const long r = t >> 1;
    const int half = (int)(t & 1);
    if (r >= capacity) return;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    int b = 0;
    const long src = pack_source_row(P, first, B, nclouds, (int)r, b);
    if (src >= 0) {
        const f64x2* row = reinterpret_cast<const f64x2*>(norm + src * 8) + half * 2;
        const f64x2 u = row[0], v = row[1];
        if (half == 0) {
            const double fx = P.aug[b * 4], fy = P.aug[b * 4 + 1], c = P.aug[b * 4 + 2], s = P.aug[b * 4 + 3];
            const double x = fx * u[0], y = fy * u[1];
            o = f32x4{(float)(x * c - y * s), (float)(x * s + y * c), (float)v[0], (float)v[1]};
        } else {
            o = f32x4{(float)u[0], (float)u[1], (float)v[0], (float)v[1]};
        }
    }
    *reinterpret_cast<f32x4*>(out + r * 8 + half * 4) = o;
}

// any C (3 and 7 in this project): one lane per row
__global__ __launch_bounds__(256) void cloud_pack_kernel(const double* __restrict__ norm, const long* __restrict__ first,
                                                          int nclouds, const void* __restrict__ params, int B, int capacity,
                                                          int C, float* __restrict__ out, int64_t* __restrict__ point_counts) {
    const BatchParams P = batch_params(params, B);
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    pack_counts(P, first, B, nclouds, r, point_counts);
    if (r >= capacity) return;
    float* o = out + r * C;
    int b = 0;
    const long src = pack_source_row(P, first, B, nclouds, (int)r, b);
    if (src < 0) {
        for (int k = 0; k < C; ++k) o[k] = 0.f;
        return;
    }
    const double* row = norm + src * C;
    const double fx = P.aug[b * 4], fy = P.aug[b * 4 + 1], c = P.aug[b * 4 + 2], s = P.aug[b * 4 + 3];
    const double x = fx * row[0], y = fy * row[1];
    o[0] = (float)(x * c - y * s);
    o[1] = (float)(x * s + y * c);
    for (int k = 2; k < C; ++k) o[k] = (float)row[k];
}

// ---- fixed-size batches sampled on the device -------------------------------------------------------------------------
// wf3d/sampling.py choice_indices(seed_word, b, n, P)[p], the specification, in uint32 arithmetic: a keyed 6-round
// balanced Feistel permutation of 2h bits cycle-walked into [0, n) between two keyed offsets when n >= P (distinct
// rows), a hash scaled by multiply-high when n < P (independent rows).  O(1) state per sample, no scratch, no sort.
__device__ __forceinline__ uint32_t fmix32(uint32_t x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}

// what is the same for every row of sample b: block-uniform, so the compiler keeps it in scalar registers
struct SamplePlan { long r0; uint32_t n, key, key2, a, c, mask; int h; bool replace; };

// the keys of sample b of a batch over n rows under one seed word (1 <= n < 2^31)
__device__ __forceinline__ void plan_keys(SamplePlan& s, uint32_t seed_word, int b, uint32_t n, bool replace) {
    s.n = n;
    s.key = fmix32(fmix32(seed_word + 0x9E3779B9u) ^ ((uint32_t)(b + 1) * 0x85EBCA6Bu));
    s.key2 = fmix32(s.key ^ 0x68E31DA4u);
    s.a = __umulhi(fmix32(s.key ^ 0xB5297A4Du), s.n);
    s.c = __umulhi(fmix32(s.key ^ 0x1B56C4E9u), s.n);
    s.h = (32 - __clz((int)(s.n - 1)) + 1) >> 1;                 // n = 1: h = 0, the permutation of one value
    s.mask = (1u << s.h) - 1u;
    s.replace = replace;
}

// false: the sample has no source (cloud index outside the resident clouds, an empty cloud) and is written as zeros
__device__ __forceinline__ bool sample_plan(const BatchParams& Q, const long* __restrict__ first, int nclouds,
                                            const uint32_t* __restrict__ seed_words, int b, int P, SamplePlan& s) {
    const int cl = Q.cloud[b];
    if (cl < 0 || cl >= nclouds) return false;
    s.r0 = first[cl];
    const long n = first[cl + 1] - s.r0;
    if (n < 1 || n > 0x7FFFFFFFL) return false;
    plan_keys(s, seed_words[0], b, (uint32_t)n, n < P);
    return true;
}

__device__ __forceinline__ uint32_t sample_index(const SamplePlan& s, uint32_t p) {
    if (s.replace) return __umulhi(fmix32(fmix32(p ^ s.key) + s.key2), s.n);
    uint32_t x = p + s.a;                                        // p < P <= n and a < n < 2^31: no wrap
    x = x >= s.n ? x - s.n : x;
    // The cycle walk: pi permutes [0, 4^h) and x starts below n, so the walk returns below n after at most
    // 4^h - n + 1 applications (4^h < 4n: fewer than 4 expected).  The only divergent loop of the kernel.
    do {
        uint32_t l = x >> s.h, r = x & s.mask;
#pragma unroll
        for (uint32_t k = 0; k < 6; ++k) {
            const uint32_t t = l ^ (fmix32(r * 0x9E3779B1u + s.key + k * 0x7F4A7C15u) & s.mask);
            l = r;
            r = t;
        }
        x = (l << s.h) | r;
    } while (x >= s.n);
    x += s.c;
    return x >= s.n ? x - s.n : x;
}

// The gather of the sampled forms (the random sampler below, farthest-point sampling behind it): output row `o` from
// resident row `src` under sample b's flips and z-rotation, float64 and one rounding; zeros for a sample without a source.
struct Augment { double fx, fy, c, sn; };
__device__ __forceinline__ Augment sample_augment(const BatchParams& Q, int b, bool live) {
    if (!live) return {1, 1, 1, 0};
    return {Q.aug[b * 4], Q.aug[b * 4 + 1], Q.aug[b * 4 + 2], Q.aug[b * 4 + 3]};
}

// x c - y s and x s + y c with the operations cloud_sample_kernel's expressions compile to (the product with y rounded,
// the one with x fused into the sum), written out: wherever the gather is inlined it gives that kernel's bits
__device__ __forceinline__ void rotate_xy(const Augment& A, double u0, double u1, double& ox, double& oy) {
#pragma clang fp contract(off)
    const double x = A.fx * u0, y = A.fy * u1;
    ox = fma(x, A.c, -(y * A.sn));
    oy = fma(x, A.sn, y * A.c);
}

__device__ __forceinline__ uint64_t mix64(uint64_t key, uint64_t n) {           // csrc/random.hip's splitmix64 step
    uint64_t z = key + (n + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The augmentation extension (wf3d/sampling.py augment_point, the specification): row b of ext [B, 8] float64 beside the
// parameter block, {sx, sy, sz, sigma, clip, drop, 0, 0}.  It changes arithmetic and replaces an output position p by 0
// (a dropped row is a copy of row 0), nothing else: no value of it reaches an address.  NoExt is the plain form's.
struct NoExt {};
struct Ext { double sx, sy, sz, sigma, clip, drop; };
// what a kernel takes by value: nothing for the plain form (its arguments are what they were), the block's address
struct NoExtBlock { using Row = NoExt; };
struct ExtBlock { using Row = Ext; const double* ext; };
__device__ __forceinline__ NoExt sample_ext(const NoExtBlock&, int, bool) { return {}; }
__device__ __forceinline__ Ext sample_ext(const ExtBlock& xb, int b, bool live) {
    if (!live) return {1, 1, 1, 0, HUGE_VAL, 0};
    const double* e = xb.ext + (long)b * 8;
    return {e[0], e[1], e[2], e[3], e[4], e[5]};
}

// K of the specification for sample b (the sample's keys under the batch's seed word) under one of the two salts
constexpr uint64_t KEY_JITTER = 0x9B05688C2B3E6C1Full, KEY_DROP = 0x1F83D9ABFB41BD6Bull;
__device__ __forceinline__ uint64_t point_key(const SamplePlan& s, uint64_t salt) {
    return (((uint64_t)s.key << 32) | (uint64_t)s.key2) ^ salt;
}

// p_eff: 0 for a dropped output row (p >= 1 and u < drop; a NaN drop drops nothing), else p
__device__ __forceinline__ uint32_t effective_row(const SamplePlan& s, const NoExt&, uint32_t p) { return p; }
__device__ __forceinline__ uint32_t effective_row(const SamplePlan& s, const Ext& X, uint32_t p) {
    const double u = (double)(mix64(point_key(s, KEY_DROP), p) >> 11) * 0x1p-53;       // exact: 53 bits, a power of two
    return p >= 1u && u < X.drop ? 0u : p;
}

// S_k - 131070 of row p_eff: the sum of the four 16-bit fields of a 64-bit hash, centred (Irwin-Hall of four)
struct Noise { int s[3]; };
__device__ __forceinline__ Noise point_noise(const SamplePlan& s, uint32_t p_eff) {
    const uint64_t K = point_key(s, KEY_JITTER);
    Noise g;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint64_t z = mix64(K, 3ull * p_eff + (uint64_t)k);
        g.s[k] = (int)((z & 0xFFFF) + ((z >> 16) & 0xFFFF) + ((z >> 32) & 0xFFFF) + (z >> 48)) - 131070;
    }
    return g;
}

// v sk + min(max(sigma g, -clip), clip), every operation rounded on its own; sigma == 0 adds nothing; a NaN sigma or
// clip gives a NaN (numpy's minimum / maximum)
__device__ __forceinline__ double ext_axis(double v, double scale, const Ext& X, int s) {
#pragma clang fp contract(off)
    const double w = v * scale;
    if (X.sigma == 0.0) return w;
    double j = X.sigma * ((double)s * 0x1.bb67ae8584caap-16);    // the double nearest to sqrt(3) 2^-16
    j = j < -X.clip ? -X.clip : j;
    j = j > X.clip ? X.clip : j;
    j = X.clip != X.clip ? X.clip : j;
    return w + j;
}
__device__ __forceinline__ void ext_xyz(const NoExt&, const Noise&, double&, double&, double&) {}
__device__ __forceinline__ void ext_xyz(const Ext& X, const Noise& g, double& x, double& y, double& z) {
    x = ext_axis(x, X.sx, X, g.s[0]);
    y = ext_axis(y, X.sy, X, g.s[1]);
    z = ext_axis(z, X.sz, X, g.s[2]);
}

// C = 8: this lane's half of the row (cloud_pack8_kernel's layout), four fp32 as one 16-byte store; x, y and z all sit
// in the even lane, so the extension touches that lane only
template <class E>
__device__ __forceinline__ void gather_half_row8(const double* __restrict__ norm, bool live, long src, int half, const Augment& A,
                                                 const E& X, const Noise& g, float* __restrict__ o) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        const f64x2* row = reinterpret_cast<const f64x2*>(norm + src * 8) + half * 2;
        const f64x2 u = row[0], w = row[1];
        if (half == 0) {
            double x, y, z = w[0];
            rotate_xy(A, u[0], u[1], x, y);
            ext_xyz(X, g, x, y, z);
            v = f32x4{(float)x, (float)y, (float)z, (float)w[1]};
        } else {
            v = f32x4{(float)u[0], (float)u[1], (float)w[0], (float)w[1]};
        }
    }
    *reinterpret_cast<f32x4*>(o + half * 4) = v;
}

// any C: the whole row in one lane
template <class E>
__device__ __forceinline__ void gather_row(const double* __restrict__ norm, bool live, long src, int C, const Augment& A,
                                           const E& X, const Noise& g, float* __restrict__ o) {
    if (!live) {
        for (int k = 0; k < C; ++k) o[k] = 0.f;
        return;
    }
    const double* row = norm + src * C;
    double x, y, z = row[2];
    rotate_xy(A, row[0], row[1], x, y);
    ext_xyz(X, g, x, y, z);
    o[0] = (float)x;
    o[1] = (float)y;
    constexpr int K0 = std::is_same<E, NoExt>::value ? 2 : 3;   // z is the extension's too
    if (K0 == 3) o[2] = (float)z;
    for (int k = K0; k < C; ++k) o[k] = (float)row[k];
}

// C = 8, cloud_pack8_kernel's layout: two lanes per row, 16-byte accesses, consecutive lanes store consecutive 16 bytes.
// A wave owns 64 output rows: lane l computes the index of row l ONCE, and the two passes of 32 rows fetch theirs with
// one ds_bpermute each (from lane j * 32 + l / 2) — against computing every index in both lanes of its pair, this
// halves the Feistel rounds per row (6 x 11 VALU operations per application, times the longest walk of the wave) for
// two cross-lane reads per 64 rows.  The shuffles come before any store guard, with the whole wave active.
// The extension (E = Ext) rides the same scheme: lane l also decides whether row l is dropped (its index is then row 0's)
// and hashes its three noise sums once, and the passes fetch them with three more shuffles each.
template <class XB>
__global__ __launch_bounds__(256) void cloud_sample_dev8_kernel(const double* __restrict__ norm, const long* __restrict__ first,
                                                                 int nclouds, const void* __restrict__ params,
                                                                 const uint32_t* __restrict__ seed_words, int B, int P,
                                                                 float* __restrict__ out, const XB xb) {
    constexpr bool EXT = std::is_same<XB, ExtBlock>::value;
    const BatchParams Q = batch_params(params, B);
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const long wave_row = (long)blockIdx.x * 256 + (threadIdx.x & ~63);
    SamplePlan s;
    const bool live = sample_plan(Q, first, nclouds, seed_words, b, P, s);
    const typename XB::Row X = sample_ext(xb, b, live);
    uint32_t idx = 0;
    Noise g = {};
    if (live && wave_row + lane < P) {
        const uint32_t p_eff = effective_row(s, X, (uint32_t)(wave_row + lane));
        idx = sample_index(s, p_eff);
        if constexpr (EXT) g = point_noise(s, p_eff);
    }
    const uint32_t idx0 = __shfl(idx, lane >> 1, 64), idx1 = __shfl(idx, 32 + (lane >> 1), 64);
    Noise g0 = {}, g1 = {};
    if constexpr (EXT) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { g0.s[k] = __shfl(g.s[k], lane >> 1, 64); g1.s[k] = __shfl(g.s[k], 32 + (lane >> 1), 64); }
    }
    const Augment A = sample_augment(Q, b, live);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const long p = wave_row + j * 32 + (lane >> 1);
        if (p >= P) continue;
        gather_half_row8(norm, live, live ? s.r0 + (j ? idx1 : idx0) : 0, lane & 1, A, X, j ? g1 : g0, out + ((long)b * P + p) * 8);
    }
}

// any C (3 and 7 in this project): one lane per row
template <class XB>
__global__ __launch_bounds__(256) void cloud_sample_dev_kernel(const double* __restrict__ norm, const long* __restrict__ first,
                                                                int nclouds, const void* __restrict__ params,
                                                                const uint32_t* __restrict__ seed_words, int B, int P, int C,
                                                                float* __restrict__ out, const XB xb) {
    constexpr bool EXT = std::is_same<XB, ExtBlock>::value;
    const BatchParams Q = batch_params(params, B);
    const int b = blockIdx.y;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    SamplePlan s;
    const bool live = sample_plan(Q, first, nclouds, seed_words, b, P, s);
    const typename XB::Row X = sample_ext(xb, b, live);
    const uint32_t p_eff = live ? effective_row(s, X, (uint32_t)p) : 0u;
    Noise g = {};
    if constexpr (EXT) { if (live) g = point_noise(s, p_eff); }
    gather_row(norm, live, live ? s.r0 + sample_index(s, p_eff) : 0, C, sample_augment(Q, b, live), X, g, out + ((long)b * P + p) * C);
}

// ---- fixed-size batches by farthest-point sampling --------------------------------------------------------------------
// wf3d/sampling.py fps_indices(seed_word, b, xyz, P), the specification: from the row fps_start (the random sampler's
// offset a), L - 1 = min(n, P) - 1 dependent rounds of "lower every point's d to its squared distance from the row just
// picked, take the largest d, the lowest index among equals".  One workgroup of T = 256, 512 or 1024 threads per sample,
// nothing between workgroups.  Thread t owns the rows i = t, t + T, ...; a cloud of at most FPS_K * T rows keeps their
// coordinates and d in registers for all rounds (the register tier), a longer one keeps d in the caller's workspace
// and reads the coordinates again every round (correct, not tuned).  A round: the update and the thread's arg-max, a
// butterfly over the wave, one candidate per wave — with its coordinates, so that the pick reaches every thread together
// with the point — into one of TWO sets of LDS slots, ONE barrier, and every thread combines the T / 64 candidates.
// Round r + 1 writes the other set, and a wave reaches round r + 2's stores only behind round r + 1's barrier, which every
// wave passes after its reads of round r: no second barrier.  Every loop is bounded by P or n.
constexpr int FPS_K = 8, FPS_MAX_WAVES = 16;
static_assert(FPS_K == 8 && FPS_K * 64 * FPS_MAX_WAVES == WF3D_FPS_REG_ROWS, "the register tier's limit is the header's");
struct FpsSlot { double d; int idx, pad; double x, y, z; };

// r of the specification: every operation rounded on its own, in this association
__device__ __forceinline__ double fps_dist(double x, double y, double z, double xs, double ys, double zs) {
#pragma clang fp contract(off)
    const double dx = x - xs, dy = y - ys, dz = z - zs;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const double xy = xx + yy;
    return xy + zz;
}

// the arg-max of (d, i) over the wave, the lowest index among equal d, in every lane (no d is a NaN)
__device__ __forceinline__ void fps_wave_max(double& d, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(d, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (od > d || (od == d && oi < i)) { d = od; i = oi; }
    }
}

// The register tier's round for a thread with KC live row slots (KC = ceil(n / T), block-uniform): straight-line code, so the
// KC distance chains interleave.  A slot without a row (i >= n) holds d = -2, which no r lowers and no pick equals.
template <int KC>
__device__ __forceinline__ void fps_update(const double (&x)[FPS_K], const double (&y)[FPS_K], const double (&z)[FPS_K],
                                           double (&d)[FPS_K], double xs, double ys, double zs, int pick, int tid, int T,
                                           double& bd, int& bi) {
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int i = k * T + tid;
        const double q = fps_dist(x[k], y[k], z[k], xs, ys, zs);
        d[k] = i == pick ? -1.0 : (q < d[k] ? q : d[k]);
        if (d[k] > bd) { bd = d[k]; bi = i; }                    // ascending i: the first of equals stays
    }
}

// behind the round's barrier: the pick among the waves' candidates and its coordinates
// (eight slots are read at once — independent LDS reads, one wait — and those of waves the workgroup does not have,
// which nothing ever wrote, are masked out)
__device__ __forceinline__ int fps_combine(const FpsSlot* __restrict__ slot, int W, double& xs, double& ys, double& zs) {
    double d = -3.0;                                             // below every candidate: wave 0's is taken first
    int i = 0x7FFFFFFF, at = 0;
#pragma unroll
    for (int g = 0; g < FPS_MAX_WAVES; g += 8) {                 // eight at a time: 24 registers beside the cloud's 64
        if (g >= W) break;
        double od[8];
        int oi[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) { od[w] = slot[g + w].d; oi[w] = slot[g + w].idx; }
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const bool better = g + w < W && (od[w] > d || (od[w] == d && oi[w] < i));
            d = better ? od[w] : d;
            i = better ? oi[w] : i;
            at = better ? g + w : at;
        }
    }
    xs = slot[at].x; ys = slot[at].y; zs = slot[at].z;
    return i;
}

template <class XB>
__global__ __launch_bounds__(1024) void cloud_fps_kernel(const double* __restrict__ norm, const long* __restrict__ first,
                                                          int nclouds, const void* __restrict__ params,
                                                          const uint32_t* __restrict__ seed_words, int B, int P, int C, int shift,
                                                          float* __restrict__ out, int* __restrict__ idx_out,
                                                          double* __restrict__ ws_d, int* __restrict__ ws_order, long ws_rows,
                                                          const XB xb) {
    constexpr bool EXT = std::is_same<XB, ExtBlock>::value;
    __shared__ FpsSlot slot[2][FPS_MAX_WAVES];
    __shared__ int order_s[WF3D_FPS_REG_ROWS];
    const BatchParams Q = batch_params(params, B);
    const int b = blockIdx.x, tid = threadIdx.x, T = 1 << shift, lane = tid & 63, wave = tid >> 6, W = T >> 6;
    SamplePlan s = {};
    bool live = sample_plan(Q, first, nclouds, seed_words, b, P, s);
    const bool in_regs = live && s.n <= (uint32_t)(FPS_K * T);
    live = live && (in_regs || (long)s.n <= ws_rows);            // a cloud longer than the caller said: no room for its d
    const int n = live ? (int)s.n : 1, L = n < P ? n : P;
    int* order_w = ws_order + (long)b * ws_rows;                 // dereferenced by the workspace tier only
    if (live) {
        const double* cloud = norm + s.r0 * C;
        int pick = (int)s.a;                                     // fps_start
        double xs = cloud[(long)pick * C], ys = cloud[(long)pick * C + 1], zs = cloud[(long)pick * C + 2];
        if (in_regs) {
            double x[FPS_K], y[FPS_K], z[FPS_K], d[FPS_K];
#pragma unroll
            for (int k = 0; k < FPS_K; ++k) {
                const int i = k * T + tid;
                x[k] = y[k] = z[k] = 0.0;
                d[k] = -2.0;                                     // no row: below every row, picked ones included
                if (i < n) { x[k] = cloud[(long)i * C]; y[k] = cloud[(long)i * C + 1]; z[k] = cloud[(long)i * C + 2]; d[k] = HUGE_VAL; }
            }
            if (tid == 0) order_s[0] = pick;
            const int kc = (n + T - 1) >> shift;
            for (int r = 1; r < L; ++r) {
                double bd = -2.0;
                int bi = 0x7FFFFFFF;
                switch (kc) {
                    case 1: fps_update<1>(x, y, z, d, xs, ys, zs, pick, tid, T, bd, bi); break;
                    case 2: fps_update<2>(x, y, z, d, xs, ys, zs, pick, tid, T, bd, bi); break;
                    case 3: fps_update<3>(x, y, z, d, xs, ys, zs, pick, tid, T, bd, bi); break;
                    case 4: fps_update<4>(x, y, z, d, xs, ys, zs, pick, tid, T, bd, bi); break;
                    case 5: fps_update<5>(x, y, z, d, xs, ys, zs, pick, tid, T, bd, bi); break;
                    case 6: fps_update<6>(x, y, z, d, xs, ys, zs, pick, tid, T, bd, bi); break;
                    case 7: fps_update<7>(x, y, z, d, xs, ys, zs, pick, tid, T, bd, bi); break;
                    default: fps_update<8>(x, y, z, d, xs, ys, zs, pick, tid, T, bd, bi); break;
                }
                fps_wave_max(bd, bi);
                FpsSlot* mine = &slot[r & 1][wave];
                if (lane == 0) { mine->d = bd; mine->idx = bi; }
                const int ku = __builtin_amdgcn_readfirstlane(bi) >> shift;       // the wave's candidate is row ku of one lane
                if ((bi & (T - 1)) == tid) {
#pragma unroll
                    for (int k = 0; k < FPS_K; ++k)
                        if (k == ku) { mine->x = x[k]; mine->y = y[k]; mine->z = z[k]; }
                }
                __syncthreads();
                pick = fps_combine(slot[r & 1], W, xs, ys, zs);
                if (tid == 0) order_s[r] = pick;
            }
        } else {
            double* dw = ws_d + (long)b * ws_rows;
            for (long i = tid; i < n; i += T) dw[i] = HUGE_VAL;   // read back by this thread only
            if (tid == 0) order_w[0] = pick;
            for (int r = 1; r < L; ++r) {
                double bd = -2.0;
                int bi = 0x7FFFFFFF;
                for (long i = tid; i < n; i += T) {
                    double di = dw[i];
                    if (i == pick) {
                        dw[i] = di = -1.0;
                    } else {
                        const double q = fps_dist(cloud[i * C], cloud[i * C + 1], cloud[i * C + 2], xs, ys, zs);
                        if (q < di) dw[i] = di = q;
                    }
                    if (di > bd) { bd = di; bi = (int)i; }
                }
                fps_wave_max(bd, bi);
                if (lane == 0) {
                    FpsSlot* mine = &slot[r & 1][wave];
                    mine->d = bd; mine->idx = bi;
                    if (bi < n) { mine->x = cloud[(long)bi * C]; mine->y = cloud[(long)bi * C + 1]; mine->z = cloud[(long)bi * C + 2]; }
                }
                __syncthreads();
                pick = fps_combine(slot[r & 1], W, xs, ys, zs);
                if (tid == 0) order_w[r] = pick;
            }
        }
    }
    __syncthreads();                                             // the order, for every thread (block-uniform: `live` is)
    // the rows: idx(b, p) = order[p mod n], through cloud_sample_dev's gather; the rounds above know nothing of the
    // extension, a dropped row takes idx(b, 0)
    const Augment A = sample_augment(Q, b, live);
    const typename XB::Row X = sample_ext(xb, b, live);
    const long rows = (long)P << (C == 8 ? 1 : 0);               // C = 8: two lanes per row, consecutive lanes 16 bytes apart
    for (long t = tid; t < rows; t += T) {
        const long p = C == 8 ? t >> 1 : t;
        int idx = 0;
        Noise g = {};
        if (live) {
            long pe = p;
            if constexpr (EXT) pe = effective_row(s, X, (uint32_t)p);
            const int q = (int)(pe < n ? pe : pe % n);
            idx = in_regs ? order_s[q] : order_w[q];
            if constexpr (EXT) { if (C != 8 || (t & 1) == 0) g = point_noise(s, (uint32_t)pe); }
        }
        if (C == 8) gather_half_row8(norm, live, s.r0 + idx, (int)(t & 1), A, X, g, out + ((long)b * P + p) * 8);
        else gather_row(norm, live, s.r0 + idx, C, A, X, g, out + ((long)b * P + p) * C);
        if (idx_out && (C != 8 || (t & 1) == 0)) idx_out[(long)b * P + p] = idx;
    }
}

// ---- epochs drawn on the device ---------------------------------------------------------------------------------------
// wf3d/sampling.py epoch_batch, the specification: the parameter block and the seed words of batch number t of a
// shuffled, rank-sharded, augmented walk over `members`, from state = {key, t} in device memory.  One workgroup; thread
// i owns the slots [i * K, (i + 1) * K), K = ceil(B / 256) <= 16, so the packed form's row offsets are one scan over 256
// partial sums.
// cos and sin of |t| <= pi / 36 as the specification's fixed polynomials: every operation rounded on its own (no fma),
// so that numpy gives the same bits
__device__ __forceinline__ void epoch_cos_sin(double t, double& c, double& s) {
#pragma clang fp contract(off)
    const double x = t * t;
    double ps = 1.0, pc = 1.0;
#pragma unroll
    for (int k = 13; k >= 3; k -= 2) {
        ps = 1.0 - x * ps / (double)(k * (k - 1));
        pc = 1.0 - x * pc / (double)((k - 1) * (k - 2));
    }
    c = pc;
    s = t * ps;
}

__device__ __forceinline__ uint32_t cloud_rows(const long* __restrict__ first, int nclouds, int cl) {
    return cl >= 0 && cl < nclouds ? (uint32_t)(first[cl + 1] - first[cl]) : 0u;
}

// the extension's configuration, by value: {lo, hi - lo, sigma, clip, max_dropout}, one scale per axis or one for all,
// and where the rows go (ext [B, 8] float64).  NoEpochExt is the plain form's.
struct NoEpochExt {};
struct EpochExt { double lo, width, sigma, clip, max_dropout; int anisotropic; double* ext; };
constexpr uint64_t KEY_SCALE = 0xA54FF53A5F1D36F1ull, KEY_DROPOUT = 0x510E527FADE682D1ull;

__device__ __forceinline__ void epoch_ext_row(const NoEpochExt&, uint64_t, uint64_t, int) {}
// wf3d/sampling.py epoch_augment_ext: all eight doubles of row b, keyed by ctr = e 2^32 + g alone
__device__ __forceinline__ void epoch_ext_row(const EpochExt& X, uint64_t key, uint64_t ctr, int b) {
#pragma clang fp contract(off)
    double* e = X.ext + (long)b * 8;
    double sc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double u = (double)(mix64(key ^ (KEY_SCALE + (uint64_t)(X.anisotropic ? k : 0)), ctr) >> 11) * 0x1p-53;
        const double w = u * X.width;
        sc[k] = X.lo + w;
    }
    const double ud = (double)(mix64(key ^ KEY_DROPOUT, ctr) >> 11) * 0x1p-53;
    e[0] = sc[0]; e[1] = sc[1]; e[2] = sc[2]; e[3] = X.sigma; e[4] = X.clip; e[5] = ud * X.max_dropout; e[6] = 0.0; e[7] = 0.0;
}

template <class E>
__global__ __launch_bounds__(256) void cloud_epoch_params_kernel(uint64_t* state, const int32_t* __restrict__ members, int D,
                                                                  const long* __restrict__ first, int nclouds, int B, int world,
                                                                  int rank, int P, int augment, double span, double half_span,
                                                                  void* params, uint32_t* __restrict__ seed_words, const E X) {
    __shared__ uint32_t part[256];
    const int tid = threadIdx.x;
    const uint64_t key = state[0], t = state[1];
    __syncthreads();                                             // every read of the counter comes before its store
    if (tid == 0) {
        state[1] = t + 1;
        const uint32_t s = (uint32_t)mix64(key ^ 0x3C6EF372FE94F82Bull, t * (uint64_t)world + (uint64_t)rank);
#pragma unroll
        for (int k = 0; k < 5; ++k) seed_words[k] = s + 0x9E3779B9u * (uint32_t)k;       // wf3d_dropout_draw's five words
    }
    const uint32_t WB = (uint32_t)world * (uint32_t)B;
    const uint64_t S = (uint64_t)((uint32_t)D / WB);             // the host refuses world * B > D: S >= 1
    const uint64_t e = t / S;
    const uint32_t g0 = (uint32_t)(t % S) * WB + (uint32_t)rank * (uint32_t)B;          // g0 + B <= S * WB <= D
    SamplePlan plan;
    plan.r0 = 0;
    plan_keys(plan, (uint32_t)mix64(key, e), 0, (uint32_t)D, false);                   // choice_indices(word, 0, D, D)
    double* aug = (double*)params;
    int* cloud = (int*)((char*)params + (size_t)B * 32);
    int* out_first = (int*)((char*)params + (size_t)B * 36);
    const int K = (B + 255) >> 8, b0 = min(tid * K, B), b1 = min(b0 + K, B);
    uint32_t rows = 0;
    for (int b = b0; b < b1; ++b) {
        const uint32_t g = g0 + (uint32_t)b;
        const int cl = members[sample_index(plan, g)];
        cloud[b] = cl;
        if (P == 0) rows += cloud_rows(first, nclouds, cl);
        double fx = 1.0, fy = 1.0, c = 1.0, s = 0.0;
        const uint64_t ctr = (e << 32) + (uint64_t)g;
        epoch_ext_row(X, key, ctr, b);
        if (augment) {
            const uint64_t za = mix64(key ^ 0x6A09E667F3BCC908ull, ctr), zb = mix64(key ^ 0xBB67AE8584CAA73Bull, ctr);
            fx = (za >> 63) & 1 ? -1.0 : 1.0;
            fy = (za >> 62) & 1 ? -1.0 : 1.0;
            const double u = (double)(zb >> 11) * 0x1p-53;       // exact: 53 bits, a power of two
            double rot;
            {
#pragma clang fp contract(off)
                rot = u * span - half_span;
            }
            epoch_cos_sin(rot, c, s);
        }
        aug[b * 4] = fx; aug[b * 4 + 1] = fy; aug[b * 4 + 2] = c; aug[b * 4 + 3] = s;
        if (P > 0) out_first[b] = b * P;
    }
    if (P > 0) {
        if (tid == 0) out_first[B] = B * P;
        return;
    }
    // the packed form: out_first = the exclusive prefix sum of the clouds' row counts (uint32 arithmetic; the host has
    // checked that no batch of these members passes the buffers' capacity)
    part[tid] = rows;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const uint32_t v = tid >= o ? part[tid - o] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint32_t at = part[tid] - rows;
    for (int b = b0; b < b1; ++b) {
        out_first[b] = (int)at;
        at += cloud_rows(first, nclouds, cloud[b]);              // this thread's own store
    }
    if (tid == 255) out_first[B] = (int)part[255];
}

// wf3d/targets.py train_targets(..., full_width=True) for sample b = blockIdx.x: c_s vertices augmented like the points,
// zeros after; existence; the count; labels of all pairs of V vertices: the row is zeroed, then (after a barrier) every
// edge min < max < c_s stores 1.0 at its pair's position among the pairs of c_s vertices.
// EXT: the vertices follow the points' scale — (sx, sy, sz) of the sample's extension row, each product rounded on its
// own behind the rotation's float64 values, one rounding to fp32; no jitter, and nothing else changes.
template <bool EXT>
__global__ __launch_bounds__(256) void wireframe_targets_kernel(const double* __restrict__ wfv, const int32_t* __restrict__ wfe,
                                                                 const long* __restrict__ vfirst, const long* __restrict__ efirst,
                                                                 int nclouds, const void* __restrict__ params, int B, int V,
                                                                 float* __restrict__ vertices, float* __restrict__ existence,
                                                                 int64_t* __restrict__ counts, float* __restrict__ labels,
                                                                 const double* __restrict__ ext) {
    const BatchParams P = batch_params(params, B);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int cl = P.cloud[b];
    const bool known = cl >= 0 && cl < nclouds;
    const long v0 = known ? vfirst[cl] : 0, e0 = known ? efirst[cl] : 0;
    const long cs = known ? vfirst[cl + 1] - v0 : 0, ne = known ? efirst[cl + 1] - e0 : 0;
    const int c = (int)(cs < V ? cs : V);            // the host refuses c_s > V; the writes stay inside the row regardless
    const double fx = P.aug[b * 4], fy = P.aug[b * 4 + 1], co = P.aug[b * 4 + 2], si = P.aug[b * 4 + 3];
    if (tid == 0) counts[b] = cs;
    for (int i = tid; i < V; i += 256) {
        float* o = vertices + ((long)b * V + i) * 3;
        if (i < c) {
            const double* v = wfv + (v0 + i) * 3;
            const double x = fx * v[0], y = fy * v[1];
            double xr = x * co - y * si, yr = x * si + y * co, z = v[2];
            if constexpr (EXT) {
#pragma clang fp contract(off)
                xr = xr * ext[(long)b * 8];
                yr = yr * ext[(long)b * 8 + 1];
                z = z * ext[(long)b * 8 + 2];
            }
            o[0] = (float)xr;
            o[1] = (float)yr;
            o[2] = (float)z;
        } else {
            o[0] = o[1] = o[2] = 0.f;
        }
        existence[(long)b * V + i] = i < c ? 1.f : 0.f;
    }
    const long W = (long)V * (V - 1) / 2;
    float* lab = labels + (long)b * W;
    for (long k = tid; k < W; k += 256) lab[k] = 0.f;
    __syncthreads();
    for (long e = tid; e < ne; e += 256) {
        const int a = wfe[(e0 + e) * 2], d = wfe[(e0 + e) * 2 + 1];
        const int i = min(a, d), j = max(a, d);
        if (i >= 0 && i < j && j < c) lab[(long)i * c - (long)i * (i + 1) / 2 + (j - i - 1)] = 1.f;
    }
}

}  // namespace

extern "C" int wf3d_cloud_normalize(const double* raw, const long* first, int nclouds, int C, int color_lo, int color_hi,
                                    int normalize, double* out, double* centroid, double* max_distance, void* stream) {
    WF3D_CHECK(nclouds >= 0 && C >= 3 && C <= 16, WF3D_ERR_ARG, "wf3d_cloud_normalize: bad dims");
    if (nclouds == 0) return WF3D_OK;
    WF3D_CHECK(raw && first && out && (!normalize || (centroid && max_distance)), WF3D_ERR_ARG, "wf3d_cloud_normalize: null pointer");
    hipLaunchKernelGGL(cloud_normalize_kernel, dim3(nclouds), dim3(256), 0, (hipStream_t)stream, raw, first, C, color_lo, color_hi,
                       normalize, out, centroid, max_distance);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" int wf3d_cloud_sample(const double* norm, const long* first, const int* cloud, const int* choice, const double* aug,
                                 int B, int P, int C, float* out, void* stream) {
    WF3D_CHECK(B >= 0 && P >= 0 && C >= 3 && C <= 16, WF3D_ERR_ARG, "wf3d_cloud_sample: bad dims");
    if (B == 0 || P == 0) return WF3D_OK;
    WF3D_CHECK(norm && first && cloud && choice && aug && out, WF3D_ERR_ARG, "wf3d_cloud_sample: null pointer");
    WF3D_CHECK(B <= 65535, WF3D_ERR_UNSUPPORTED, "wf3d_cloud_sample: B > 65535");
    hipLaunchKernelGGL(cloud_sample_kernel, dim3(wf3d_cdiv(P, 256), B), dim3(256), 0, (hipStream_t)stream, norm, first, cloud, choice,
                       aug, P, C, out);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" int wf3d_cloud_pack(const double* norm, const long* first, int nclouds, const void* params, int B, int capacity,
                               int C, float* points, int64_t* point_counts, void* stream) {
    WF3D_CHECK(nclouds >= 1 && B >= 1 && B <= 4096 && capacity >= 1 && C >= 3 && C <= 16, WF3D_ERR_ARG, "wf3d_cloud_pack: bad dims");
    WF3D_CHECK(norm && first && params && points && point_counts, WF3D_ERR_ARG, "wf3d_cloud_pack: null pointer");
    WF3D_CHECK(((uintptr_t)params & 7) == 0, WF3D_ERR_ARG, "wf3d_cloud_pack: params must be 8-byte aligned");
    if (C == 8) {
        WF3D_CHECK((((uintptr_t)norm | (uintptr_t)points) & 15) == 0, WF3D_ERR_ARG, "wf3d_cloud_pack: norm and points must be 16-byte aligned");
        hipLaunchKernelGGL(cloud_pack8_kernel, dim3(wf3d_cdiv(2L * capacity > B ? 2L * capacity : B, 256)), dim3(256), 0, (hipStream_t)stream, norm, first,
                           nclouds, params, B, capacity, points, point_counts);
    } else {
        hipLaunchKernelGGL(cloud_pack_kernel, dim3(wf3d_cdiv(capacity > B ? capacity : B, 256)), dim3(256), 0, (hipStream_t)stream,
                           norm, first, nclouds, params, B, capacity, C, points, point_counts);
    }
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

// the plain entry point and its `_ext` form (E = Ext, `ext` required): one argument list, one launch
template <class XB>
static int cloud_sample_dev_launch(const double* norm, const long* first, int nclouds, const void* params,
                                   const uint32_t* seed_words, int B, int P, int C, float* points, const XB& xb, void* stream) {
    WF3D_CHECK(nclouds >= 1 && B >= 1 && B <= 4096 && P >= 1 && C >= 3 && C <= 16, WF3D_ERR_ARG, "wf3d_cloud_sample_dev: bad dims");
    WF3D_CHECK((long)B * P <= 0x7FFFFFFFL, WF3D_ERR_ARG, "wf3d_cloud_sample_dev: B * P must stay below 2^31");
    WF3D_CHECK(norm && first && params && seed_words && points, WF3D_ERR_ARG, "wf3d_cloud_sample_dev: null pointer");
    WF3D_CHECK(((uintptr_t)params & 7) == 0 && ((uintptr_t)seed_words & 3) == 0, WF3D_ERR_ARG,
               "wf3d_cloud_sample_dev: params must be 8-byte aligned, seed_words 4-byte aligned");
    const dim3 grid(wf3d_cdiv(P, 256), B);
    if (C == 8) {
        WF3D_CHECK((((uintptr_t)norm | (uintptr_t)points) & 15) == 0, WF3D_ERR_ARG, "wf3d_cloud_sample_dev: norm and points must be 16-byte aligned");
        hipLaunchKernelGGL(cloud_sample_dev8_kernel<XB>, grid, dim3(256), 0, (hipStream_t)stream, norm, first, nclouds, params,
                           seed_words, B, P, points, xb);
    } else {
        hipLaunchKernelGGL(cloud_sample_dev_kernel<XB>, grid, dim3(256), 0, (hipStream_t)stream, norm, first, nclouds, params,
                           seed_words, B, P, C, points, xb);
    }
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" int wf3d_cloud_sample_dev(const double* norm, const long* first, int nclouds, const void* params,
                                     const uint32_t* seed_words, int B, int P, int C, float* points, void* stream) {
    return cloud_sample_dev_launch(norm, first, nclouds, params, seed_words, B, P, C, points, NoExtBlock{}, stream);
}

extern "C" int wf3d_cloud_sample_dev_ext(const double* norm, const long* first, int nclouds, const void* params,
                                         const uint32_t* seed_words, int B, int P, int C, float* points, const double* ext,
                                         void* stream) {
    WF3D_CHECK(ext && ((uintptr_t)ext & 7) == 0, WF3D_ERR_ARG, "wf3d_cloud_sample_dev_ext: ext must be given, 8-byte aligned");
    return cloud_sample_dev_launch(norm, first, nclouds, params, seed_words, B, P, C, points, ExtBlock{ext}, stream);
}

// the workspace tier's d (float64) and order (int32) of max_rows rows per sample; nothing while every cloud fits the registers
extern "C" size_t wf3d_cloud_sample_fps_ws_bytes(int B, long max_rows) {
    if (B < 1 || max_rows <= WF3D_FPS_REG_ROWS) return 0;
    return ((size_t)B * (size_t)max_rows * 12 + 15) & ~(size_t)15;
}

template <class XB>
static int cloud_sample_fps_launch(const double* norm, const long* first, int nclouds, const void* params,
                                   const uint32_t* seed_words, int B, int P, int C, float* points, int32_t* idx_out,
                                   long max_rows, void* ws, size_t ws_bytes, const XB& xb, void* stream) {
    WF3D_CHECK(nclouds >= 1 && B >= 1 && B <= 4096 && P >= 1 && C >= 3 && C <= 16 && max_rows >= 1 && max_rows <= 0x7FFFFFFFL,
               WF3D_ERR_ARG, "wf3d_cloud_sample_fps: bad dims");
    WF3D_CHECK((long)B * P <= 0x7FFFFFFFL, WF3D_ERR_ARG, "wf3d_cloud_sample_fps: B * P must stay below 2^31");
    WF3D_CHECK(norm && first && params && seed_words && points, WF3D_ERR_ARG, "wf3d_cloud_sample_fps: null pointer");
    WF3D_CHECK(((uintptr_t)params & 7) == 0 && (((uintptr_t)seed_words | (uintptr_t)idx_out) & 3) == 0, WF3D_ERR_ARG,
               "wf3d_cloud_sample_fps: params must be 8-byte aligned, seed_words and idx_out 4-byte aligned");
    WF3D_CHECK(C != 8 || (((uintptr_t)norm | (uintptr_t)points) & 15) == 0, WF3D_ERR_ARG,
               "wf3d_cloud_sample_fps: norm and points must be 16-byte aligned");
    const size_t need = wf3d_cloud_sample_fps_ws_bytes(B, max_rows);
    WF3D_CHECK(need == 0 || (ws && ws_bytes >= need && ((uintptr_t)ws & 7) == 0), WF3D_ERR_ARG,
               "wf3d_cloud_sample_fps: workspace missing, misaligned or below wf3d_cloud_sample_fps_ws_bytes");
    // the workgroup by the longest cloud: FPS_K rows per thread
    const int shift = max_rows <= FPS_K * 256 ? 8 : (max_rows <= FPS_K * 512 ? 9 : 10);
    const long ws_rows = need ? max_rows : 0;
    double* ws_d = need ? (double*)ws : nullptr;
    int* ws_order = need ? (int*)(ws_d + (size_t)B * (size_t)ws_rows) : nullptr;
    hipLaunchKernelGGL(cloud_fps_kernel<XB>, dim3(B), dim3(1 << shift), 0, (hipStream_t)stream, norm, first, nclouds, params, seed_words,
                       B, P, C, shift, points, idx_out, ws_d, ws_order, ws_rows, xb);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" int wf3d_cloud_sample_fps(const double* norm, const long* first, int nclouds, const void* params,
                                     const uint32_t* seed_words, int B, int P, int C, float* points, int32_t* idx_out,
                                     long max_rows, void* ws, size_t ws_bytes, void* stream) {
    return cloud_sample_fps_launch(norm, first, nclouds, params, seed_words, B, P, C, points, idx_out, max_rows, ws, ws_bytes,
                                   NoExtBlock{}, stream);
}

extern "C" int wf3d_cloud_sample_fps_ext(const double* norm, const long* first, int nclouds, const void* params,
                                         const uint32_t* seed_words, int B, int P, int C, float* points, int32_t* idx_out,
                                         long max_rows, void* ws, size_t ws_bytes, const double* ext, void* stream) {
    WF3D_CHECK(ext && ((uintptr_t)ext & 7) == 0, WF3D_ERR_ARG, "wf3d_cloud_sample_fps_ext: ext must be given, 8-byte aligned");
    return cloud_sample_fps_launch(norm, first, nclouds, params, seed_words, B, P, C, points, idx_out, max_rows, ws, ws_bytes,
                                   ExtBlock{ext}, stream);
}

template <class E>
static int cloud_epoch_params_launch(uint64_t* state, const int32_t* members, int D, const long* first, int nclouds, int B,
                                     int world, int rank, int P, int augment, void* params, uint32_t* seed_words, const E& X,
                                     void* stream) {
    WF3D_CHECK(D >= 1 && nclouds >= 1 && B >= 1 && world >= 1 && rank >= 0 && rank < world && P >= 0 && (augment == 0 || augment == 1),
               WF3D_ERR_ARG, "wf3d_cloud_epoch_params: bad dims");
    WF3D_CHECK(B <= 4096, WF3D_ERR_UNSUPPORTED, "wf3d_cloud_epoch_params: B > 4096");
    WF3D_CHECK((long)world * B <= D, WF3D_ERR_ARG, "wf3d_cloud_epoch_params: world * B must not pass D (no whole step in an epoch)");
    WF3D_CHECK((long)B * P <= 0x7FFFFFFFL, WF3D_ERR_ARG, "wf3d_cloud_epoch_params: B * P must stay below 2^31");
    WF3D_CHECK(state && members && first && params && seed_words, WF3D_ERR_ARG, "wf3d_cloud_epoch_params: null pointer");
    WF3D_CHECK((((uintptr_t)state | (uintptr_t)params) & 7) == 0 && (((uintptr_t)seed_words | (uintptr_t)members) & 3) == 0, WF3D_ERR_ARG,
               "wf3d_cloud_epoch_params: state and params must be 8-byte aligned, members and seed_words 4-byte aligned");
    const double pi = 3.141592653589793;                         // the double numpy calls pi; both quotients rounded once
    hipLaunchKernelGGL(cloud_epoch_params_kernel<E>, dim3(1), dim3(256), 0, (hipStream_t)stream, state, members, D, first, nclouds, B,
                       world, rank, P, augment, pi / 18.0, pi / 36.0, params, seed_words, X);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" int wf3d_cloud_epoch_params(uint64_t* state, const int32_t* members, int D, const long* first, int nclouds, int B,
                                       int world, int rank, int P, int augment, void* params, uint32_t* seed_words, void* stream) {
    return cloud_epoch_params_launch(state, members, D, first, nclouds, B, world, rank, P, augment, params, seed_words, NoEpochExt{},
                                     stream);
}

// cfg (HOST memory): {lo, hi, anisotropic, sigma, clip, max_dropout, 0, 0}, held to wf3d.sampling.check_augment's rules
extern "C" int wf3d_cloud_epoch_params_ext(uint64_t* state, const int32_t* members, int D, const long* first, int nclouds, int B,
                                           int world, int rank, int P, int augment, void* params, uint32_t* seed_words,
                                           const double* cfg, double* ext, void* stream) {
    WF3D_CHECK(cfg && ext && ((uintptr_t)ext & 7) == 0, WF3D_ERR_ARG, "wf3d_cloud_epoch_params_ext: cfg and ext must be given, ext 8-byte aligned");
    const double lo = cfg[0], hi = cfg[1], sigma = cfg[3], clip = cfg[4], max_dropout = cfg[5];
    WF3D_CHECK(std::isfinite(lo) && std::isfinite(hi) && 0.0 < lo && lo <= hi, WF3D_ERR_ARG,
               "wf3d_cloud_epoch_params_ext: scale needs finite 0 < lo <= hi");
    WF3D_CHECK(cfg[2] == 0.0 || cfg[2] == 1.0, WF3D_ERR_ARG, "wf3d_cloud_epoch_params_ext: anisotropic must be 0 or 1");
    WF3D_CHECK(std::isfinite(sigma) && sigma >= 0.0, WF3D_ERR_ARG, "wf3d_cloud_epoch_params_ext: sigma must be finite and >= 0");
    WF3D_CHECK(clip > 0.0, WF3D_ERR_ARG, "wf3d_cloud_epoch_params_ext: clip must be > 0 (inf: no clip)");
    WF3D_CHECK(max_dropout >= 0.0 && max_dropout <= 1.0, WF3D_ERR_ARG, "wf3d_cloud_epoch_params_ext: max_dropout must be in [0, 1]");
    WF3D_CHECK(cfg[6] == 0.0 && cfg[7] == 0.0, WF3D_ERR_ARG, "wf3d_cloud_epoch_params_ext: cfg[6] and cfg[7] must be 0");
    const EpochExt X = {lo, hi - lo, sigma, clip, max_dropout, cfg[2] == 1.0 ? 1 : 0, ext};
    return cloud_epoch_params_launch(state, members, D, first, nclouds, B, world, rank, P, augment, params, seed_words, X, stream);
}

template <bool EXT>
static int wireframe_targets_launch(const double* wf_vertices, const int32_t* wf_edges, const long* vfirst, const long* efirst,
                                    int nclouds, const void* params, int B, int V, float* vertices, float* vertex_existence,
                                    int64_t* vertex_counts, float* edge_labels, const double* ext, void* stream) {
    WF3D_CHECK(nclouds >= 1 && B >= 1 && B <= 4096 && V >= 1 && V <= 32768, WF3D_ERR_ARG, "wf3d_wireframe_targets: bad dims");
    // wf_vertices / wf_edges / edge_labels may be NULL where they hold nothing (no vertices, no edges, V = 1)
    WF3D_CHECK(vfirst && efirst && params && vertices && vertex_existence && vertex_counts && (edge_labels || V < 2), WF3D_ERR_ARG,
               "wf3d_wireframe_targets: null pointer");
    WF3D_CHECK(((uintptr_t)params & 7) == 0, WF3D_ERR_ARG, "wf3d_wireframe_targets: params must be 8-byte aligned");
    WF3D_CHECK(!EXT || (ext && ((uintptr_t)ext & 7) == 0), WF3D_ERR_ARG, "wf3d_wireframe_targets_ext: ext must be given, 8-byte aligned");
    hipLaunchKernelGGL(wireframe_targets_kernel<EXT>, dim3(B), dim3(256), 0, (hipStream_t)stream, wf_vertices, wf_edges, vfirst, efirst,
                       nclouds, params, B, V, vertices, vertex_existence, vertex_counts, edge_labels, ext);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" int wf3d_wireframe_targets(const double* wf_vertices, const int32_t* wf_edges, const long* vfirst, const long* efirst,
                                      int nclouds, const void* params, int B, int V, float* vertices, float* vertex_existence,
                                      int64_t* vertex_counts, float* edge_labels, void* stream) {
    return wireframe_targets_launch<false>(wf_vertices, wf_edges, vfirst, efirst, nclouds, params, B, V, vertices, vertex_existence,
                                           vertex_counts, edge_labels, nullptr, stream);
}

extern "C" int wf3d_wireframe_targets_ext(const double* wf_vertices, const int32_t* wf_edges, const long* vfirst, const long* efirst,
                                          int nclouds, const void* params, int B, int V, float* vertices, float* vertex_existence,
                                          int64_t* vertex_counts, float* edge_labels, const double* ext, void* stream) {
    return wireframe_targets_launch<true>(wf_vertices, wf_edges, vfirst, efirst, nclouds, params, B, V, vertices, vertex_existence,
                                          vertex_counts, edge_labels, ext, stream);
}

// Host: the numbers of a whitespace-separated text table.  `#` starts a comment (to the end of the line: \n, \r\n or \r); numbers are
// parsed in the C locale whatever the process locale is.  out[0..max_vals) receives the values in file order; returns
// how many the file holds (> max_vals: call again with a larger buffer), -1 if the file cannot be read, -2 on a token
// (the characters up to whitespace, `#` or the end) that is not, as a whole, a decimal number, inf or nan,
// -3 (wf3d_parse_table only) if two non-empty rows hold different numbers of values.
static long parse_numbers(const char* path, double* out, long max_vals, long* ncols) {
    static locale_t c_loc = newlocale(LC_ALL_MASK, "C", (locale_t)0);
    FILE* f = fopen(path, "rb");
    if (!f) return -1;
    if (fseek(f, 0, SEEK_END) != 0) { fclose(f); return -1; }
    const long sz = ftell(f);
    if (sz < 0 || fseek(f, 0, SEEK_SET) != 0) { fclose(f); return -1; }
    char* buf = (char*)malloc((size_t)sz + 1);
    if (!buf) { fclose(f); return -1; }
    const size_t got = fread(buf, 1, (size_t)sz, f);
    fclose(f);
    if (got != (size_t)sz) { free(buf); return -1; }
    buf[got] = 0;
    long n = 0, in_row = 0, cols = 0;
    bool ragged = false;
    char* p = buf;
    auto end_row = [&]() {
        if (in_row) {
            if (cols == 0) cols = in_row; else if (in_row != cols) ragged = true;
            in_row = 0;
        }
    };
    for (;;) {
        while (*p == ' ' || *p == '\t' || *p == '\v' || *p == '\f') ++p;
        if (*p == '#') { while (*p && *p != '\n' && *p != '\r') ++p; }
        if (*p == '\n' || *p == '\r') { end_row(); ++p; continue; }       // \n, \r\n and a lone \r end a row, as for np.loadtxt
        if (!*p) break;
        // the token: up to whitespace, `#` or the end.  The number must be all of it (np.loadtxt refuses `3.4.5`,
        // `1.0-2.0`, `1e5x`), and strtod's hexadecimal and `nan(...)` forms are not numbers of a table either.
        const char* q = p;
        bool plain = true;
        for (; *q && *q != ' ' && *q != '\t' && *q != '\r' && *q != '\n' && *q != '\v' && *q != '\f' && *q != '#'; ++q)
            plain = plain && *q != 'x' && *q != 'X' && *q != '(';
        char* end;
        const double v = c_loc ? strtod_l(p, &end, c_loc) : strtod(p, &end);
        if (!plain || end != q) { free(buf); return -2; }
        if (n < max_vals && out) out[n] = v;
        ++n; ++in_row;
        p = end;
    }
    end_row();
    free(buf);
    if (ncols) { *ncols = cols; if (ragged) return -3; }
    return n;
}

extern "C" long wf3d_parse_floats(const char* path, double* out, long max_vals) { return parse_numbers(path, out, max_vals, nullptr); }

// Same, and *ncols = the number of values per row (np.loadtxt's second dimension).
extern "C" long wf3d_parse_table(const char* path, double* out, long max_vals, long* ncols) {
    if (!ncols) return -1;
    return parse_numbers(path, out, max_vals, ncols);
}
