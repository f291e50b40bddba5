// Shared device/host helpers for the wf3d HIP kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/wf3d.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define WF3D_WAVE 64

// Internal cross-translation-unit helpers are not part of the C ABI: hidden, so that libwf3d.so exports exactly what
// include/wf3d.h declares (tests/test_capi_symbols.py checks both directions).
#define WF3D_INTERNAL __attribute__((visibility("hidden")))

// ---- error plumbing (host) -------------------------------------------------
WF3D_INTERNAL void wf3d_set_error(const char* fmt, ...);
#define WF3D_CHECK(cond, code, ...)                \
    do {                                           \
        if (!(cond)) {                             \
            wf3d_set_error(__VA_ARGS__);           \
            return (code);                         \
        }                                          \
    } while (0)
#define WF3D_LAUNCH_CHECK()                                                   \
    do {                                                                      \
        hipError_t e_ = hipGetLastError();                                    \
        if (e_ != hipSuccess) {                                               \
            wf3d_set_error("%s:%d launch failed: %s", __FILE__, __LINE__,     \
                           hipGetErrorString(e_));                            \
            return WF3D_ERR_LAUNCH;                                           \
        }                                                                     \
    } while (0)

static inline int wf3d_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ---- dropout seed source (host + device) -------------------------------------
// Every mask kernel takes its seed as a wf3d_seed_t: the value itself (words == NULL), or, while the calling thread has
// set device seed words (wf3d_set_dropout_seed_words), an index into those words that the kernel loads at run time.
// The pointer is a kernel argument, so a captured graph replays with whatever words a draw kernel wrote before it.
struct wf3d_seed_t { uint32_t v; const uint32_t* words; };
// the seed argument of a launch that drops with probability drop_p (no words are read when nothing is dropped)
WF3D_INTERNAL wf3d_seed_t wf3d_seed_arg(float drop_p, uint32_t drop_seed);
// The three dropout arguments of a mask launch: the seed source, the 32-bit threshold an element's hash must reach to be
// kept (0: nothing is dropped, and no kernel then reads the other two) and the keep scale 1 / (1 - drop_p).
struct wf3d_drop_t { wf3d_seed_t seed; uint32_t thresh; float scale; };
static inline wf3d_drop_t wf3d_drop_args(float drop_p, uint32_t drop_seed) {
    return {wf3d_seed_arg(drop_p, drop_seed), drop_p > 0.f ? (uint32_t)((double)drop_p * 4294967296.0) : 0u,
            1.0f / (1.0f - drop_p)};
}

// ---- live-row count (host + device) -------------------------------------------
// While the calling thread has set one (wf3d_set_live_rows), the entry points that include/wf3d.h lists under "LIVE ROW
// COUNT" hand this pointer to their kernels, which read it once at entry; every other entry point never asks for it.
WF3D_INTERNAL const int32_t* wf3d_live_rows();

// ---- split-K (host) --------------------------------------------------------
// A GEMM whose output has too few tiles to fill the chip cuts its reduction into `ksplit` ranges of `kt_per` K slices;
// each range writes a slab of M x N partial sums into the caller's workspace and wf3d_splitk_combine folds them.  One
// planner; each kernel family's constants are one row.
struct SplitKRule {
    int nosplit_tiles;   // K is not split from this many output tiles up
    int target;          // workgroups (tiles x K ranges) to aim for
    int cap;             // K ranges at most
    int few_tiles;       // up to this many tiles the launch is a streaming reduction over K:
    int few_slices;      //   K slices per range at least (otherwise 4)
    int few_cap;         //   K ranges at most
    bool few_mult8;      //   range count rounded down to a multiple of 8 (the XCD-mapped launch order applies)
};
// fp32 wf3d_gemm and the register-staged split kernel.  Few tiles and a very long reduction (first-layer wgrad:
// 512 x 8 outputs over K = B*N rows) stream their operands from HBM: they need >= 2 workgroups per CU in flight.
constexpr SplitKRule WF3D_SPLITK_GEMM = {256, 512, 64, 8, 4, 256, false};
// LDS-DMA split forward / dgrad: K is split only below 192 tiles.  At 252 tiles (the edge MLP at cfg2) two K ranges +
// slabs + a combine launch cost more than the idle quarter-wave they fill (scripts/bench_edge_gemms.py: 62 -> 48,
// 52 -> 26, 36 -> 25, 86 -> 61 us for its four GEMMs).
constexpr SplitKRule WF3D_SPLITK_SPLIT = {192, 512, 64, 0, 4, 64, false};
// Split wgrad, 256x128 and 256x256 tiles (one full wave of 256 workgroups either way).  One to four output tiles (the
// edge MLP's 128 x 256 and 256 x 512 weights over ~10^5 - 10^6 edge rows) get a K range per CU (up to 256 slabs) as
// long as a range keeps >= 8 slices; more tiles keep the 64-range cap that bounds the slab traffic (with 64 ranges the
// 128 x 256 wgrad of cfg5 ran on 64 CUs at 2.0 TB/s, the 256 x 512 one on half the chip).
constexpr SplitKRule WF3D_SPLITK_TN = {256, 512, 64, 4, 8, 256, true};
constexpr SplitKRule WF3D_SPLITK_TN16 = {256, 256, 64, 4, 8, 256, true};

struct SplitK { int ksplit, kt_per; };

// `rounds` multiplies the target and the cap (the wgrad "tn_rounds" option)
static inline SplitK wf3d_splitk_plan(const SplitKRule& r, long tiles, int ktotal, int rounds = 1) {
    SplitK s{1, ktotal};
    if (tiles >= r.nosplit_tiles || ktotal < 8) return s;
    const bool few = tiles <= r.few_tiles;
    const int want = (int)(((long)r.target * rounds + tiles - 1) / tiles);
    const int most = ktotal / (few ? r.few_slices : 4);
    int ks = want < most ? want : most;
    const int cap = few ? r.few_cap : r.cap * rounds;
    if (ks > cap) ks = cap;
    if (few && r.few_mult8 && ks >= 8) ks &= ~7;
    if (ks < 2) return s;
    s.kt_per = wf3d_cdiv(ktotal, ks);
    s.ksplit = wf3d_cdiv(ktotal, s.kt_per);      // no empty range
    return s;
}

static inline size_t wf3d_splitk_slab_bytes(SplitK s, int M, int N) {
    return s.ksplit > 1 ? (size_t)s.ksplit * M * N * sizeof(float) : 0;
}

// At launch: a split whose slabs do not fit the caller's workspace runs as one K range.
static inline SplitK wf3d_splitk_fit(SplitK s, int ktotal, int M, int N, const void* ws, size_t ws_bytes) {
    const size_t need = wf3d_splitk_slab_bytes(s, M, N);
    return need && (ws == nullptr || ws_bytes < need) ? SplitK{1, ktotal} : s;
}

// C = sum of the `ksplit` slabs (+ bias[n]) (+ lr_u[m, :lr_k] . lr_v[n, :lr_k]) (+ addend[m, n]) (+ C if accumulate).
// The fold order is fixed (deterministic): slab after slab, or, for more than 16 slabs with N % 4 == 0 and a 16-B
// aligned workspace, 16 strided partial sums per output met in a shuffle tree.  narrow_only keeps slab after slab.
struct SplitKCombine {
    const float* slab; float* C; const float* bias; const float* addend; const float* lr_u; const float* lr_v;
    int M, N, ldc, ld_addend, lr_k, ld_lr_u, ld_lr_v, ksplit, accumulate;
    const int32_t* live;      // live-row count over the M rows (NULL: all of them); rows past the extent are not touched
};
WF3D_INTERNAL int wf3d_splitk_combine(const SplitKCombine& c, bool narrow_only, hipStream_t st);

// The register-staged split GEMM (gemm.hip, gemm_kernel<..., SPLIT>: 128 x 128 tiles, K in 32-wide slices, any K % 8
// == 0).  Its caller, gemm_split.hip, plans `s` with WF3D_SPLITK_GEMM; the slabs (s.ksplit > 1) are folded slab after
// slab.
WF3D_INTERNAL int wf3d_gemm_split_regs(int products, const void* A_sx8, const void* B_sx8, float* C, const float* bias,
                                       int M, int N, int K, int lda, int ldb, int ldc, int accumulate, SplitK s,
                                       float* slab, const int32_t* live, hipStream_t st);

// Attention: the kernels' argument block, its builder, the launch helper and the entry to the MFMA kernels
// (attn_mfma.hip) are declared in attn_args.h, which attn.hip and attn_mfma.hip include.
// the "attn_tiled" value of wf3d_set_option (attn.hip holds it)
WF3D_INTERNAL int wf3d_attn_set_tiled(int value);

// ---- device helpers --------------------------------------------------------
#ifdef __HIPCC__
// Row extent of a launch under a live-row count: R itself without one, else R256 = min(R, 256 * ceil(clamp(*live, 0, R)
// / 256)).  One wave-uniform load at kernel entry; every tile height and K slice of the kernels divides 256, so no
// kernel meets a partial tile at the extent.
__device__ __forceinline__ int wf3d_live_extent(const int32_t* live, int R) {
    if (live == nullptr) return R;
    const int n = min(max(*live, 0), R);
    return (int)min((long)R, ((long)n + 255) / 256 * 256);
}

// erf in fp32 to ~1 ulp, branch-free: both polynomial pieces (N. Juffa's minimax coefficients: |x| <= 0.9277 odd
// polynomial in x; beyond, 1 - exp(-|x| * P(|x|))) are evaluated and selected — 21 VALU operations against the ~42 of
// the library erff, whose two paths a wave with mixed arguments both walks anyway.  The edge head evaluates GELU or its
// derivative on every element of its [edges, 512 / 256 / 128] activations: at max_vertices = 256 the pair kernel and
// the LayerNorm backward of the first edge layer are bound by these instructions, not by HBM.
__device__ __forceinline__ float wf3d_erf(float a) {
    const float t = fabsf(a), s = a * a;
    float r = fmaf(-1.72853470e-5f, t, 3.83197126e-4f);
    const float u = fmaf(-3.88396438e-3f, t, 2.42546219e-2f);
    r = fmaf(r, s, u);
    r = fmaf(r, t, -1.06777877e-1f);
    r = fmaf(r, t, -6.34846687e-1f);
    r = fmaf(r, t, -1.28717512e-1f);
    r = fmaf(r, t, -t);
    r = copysignf(1.0f - __expf(r), a);
    float q = -5.96761703e-4f;
    q = fmaf(q, s, 4.99119423e-3f);
    q = fmaf(q, s, -2.67681349e-2f);
    q = fmaf(q, s, 1.12819925e-1f);
    q = fmaf(q, s, -3.76125336e-1f);
    q = fmaf(q, s, 1.28379166e-1f);
    q = fmaf(q, a, a);
    return t > 0.927734375f ? r : q;
}

// activations used on the path: ReLU (encoder / vertex head), erf-GELU (edge head)
template <int ACT>
__device__ __forceinline__ float wf3d_act(float y) {
    if (ACT == WF3D_ACT_RELU) return fmaxf(y, 0.0f);
    if (ACT == WF3D_ACT_GELU) return 0.5f * y * (1.0f + wf3d_erf(y * 0.70710678118654752440f));
    return y;
}
// d act(y) / dy
template <int ACT>
__device__ __forceinline__ float wf3d_act_grad(float y) {
    if (ACT == WF3D_ACT_RELU) return y > 0.0f ? 1.0f : 0.0f;
    if (ACT == WF3D_ACT_GELU) {
        const float cdf = 0.5f * (1.0f + wf3d_erf(y * 0.70710678118654752440f));
        const float pdf = 0.39894228040143267794f * __expf(-0.5f * y * y);
        return cdf + y * pdf;
    }
    return 1.0f;
}
__device__ __forceinline__ float wf3d_act_rt(int act, float y) {
    return act == WF3D_ACT_RELU ? wf3d_act<WF3D_ACT_RELU>(y)
         : act == WF3D_ACT_GELU ? wf3d_act<WF3D_ACT_GELU>(y) : y;
}
__device__ __forceinline__ float wf3d_act_grad_rt(int act, float y) {
    return act == WF3D_ACT_RELU ? wf3d_act_grad<WF3D_ACT_RELU>(y)
         : act == WF3D_ACT_GELU ? wf3d_act_grad<WF3D_ACT_GELU>(y) : 1.0f;
}

// Counter-based dropout keep-mask: the same (seed,row,col) gives the same bit
// in the forward prologue and in the backward kernels, so masks are never stored.
__device__ __forceinline__ bool wf3d_keep(uint32_t seed, uint32_t row, uint32_t col, uint32_t thresh) {
    uint32_t h = seed ^ (row * 0x9E3779B1u) ^ (col * 0x85EBCA77u + 0x27D4EB2Fu);
    h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
    return h >= thresh;
}

// The seed a mask kernel uses: read once at kernel entry (a wave-uniform load from the caller's device words).
__device__ __forceinline__ uint32_t wf3d_seed_load(const wf3d_seed_t& s) { return s.words ? s.words[s.v] : s.v; }

// edge rows of one sample: all pairs i < j of its v vertices in lexicographic order (EdgePredictor.py:83-86);
// edge index e -> (i, j), and the index of pair (i, i + 1)
__device__ __forceinline__ void edge_ij(int e, int v, int& i, int& j) {
    const float b = (float)(2 * v - 1);
    int ii = (int)floorf((b - sqrtf(fmaxf(b * b - 8.0f * (float)e, 0.f))) * 0.5f);
    ii = max(0, min(ii, v - 2));
    // offset(i) = i*(2v-i-1)/2 ; fix up float rounding
    while (ii + 1 <= v - 2 && ((ii + 1) * (2 * v - ii - 2)) / 2 <= e) ++ii;
    while (ii > 0 && (ii * (2 * v - ii - 1)) / 2 > e) --ii;
    i = ii;
    j = e - (ii * (2 * v - ii - 1)) / 2 + ii + 1;
}
__device__ __forceinline__ int edge_offset(int i, int v) { return (i * (2 * v - i - 1)) / 2; }

// the common width min(prediction width, Ep, Et) of the loss's edge term and of the training metrics when the prediction
// width is a device scalar (a padded edge head's edge_width; its predictions tensor is Ep >= width wide)
__device__ __forceinline__ int edge_common_width(int64_t w, int Ep, int Et) {
    int64_t m = w < (int64_t)Ep ? w : (int64_t)Ep;
    if ((int64_t)Et < m) m = Et;
    return m > 0 ? (int)m : 0;
}

__device__ __forceinline__ float wf3d_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wf3d_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// An sx8 group (8 columns: 16 B of bf16 high parts, 16 B of low parts; csrc/split.hip) written by a PAIR of lanes (lane-contiguous row passes): the even lane holds columns 0..3 of the group,
// the odd lane columns 4..7, each at `dst` = the address of its own four fp32 columns.  After one exchange the even lane
// owns the eight high parts (the group's first 16 bytes) and the odd lane the eight low parts (the second 16): every
// lane writes 16 bytes right where it read 16 — consecutive lanes, consecutive bytes — instead of two stores 32 B apart.
// (Measured on a plain copy of 131072 x 2048 floats, scripts/micro/copy_patterns.hip: 5.0 -> 5.4 TB/s for the store
// pattern alone, 5.7 with non-temporal loads and stores, which the 32-B-apart stores cannot use: 3.9 TB/s.)
__device__ __forceinline__ void wf3d_store_sx8_pair(float* dst, const float (&v)[4], bool odd) {
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    bf16x4 hi, lo;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        hi[j] = (__bf16)v[j];
        lo[j] = (__bf16)(v[j] - (float)hi[j]);
    }
    const u32x2 H = __builtin_bit_cast(u32x2, hi), L = __builtin_bit_cast(u32x2, lo);
    const unsigned s0 = odd ? H[0] : L[0], s1 = odd ? H[1] : L[1];
    // neighbour exchange inside each quad: DPP quad_perm [1, 0, 3, 2] (a VALU move, no trip through the LDS crossbar)
    const unsigned r0 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)s0, 0xB1, 0xF, 0xF, true);
    const unsigned r1 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)s1, 0xB1, 0xF, 0xF, true);
    const u32x4 o = odd ? u32x4{r0, r1, L[0], L[1]} : u32x4{H[0], H[1], r0, r1};
    __builtin_nontemporal_store(__builtin_bit_cast(f32x4, o), reinterpret_cast<f32x4*>(dst));
}


#endif
