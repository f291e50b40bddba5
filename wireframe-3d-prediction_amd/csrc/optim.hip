// Row f-2: the step tail of the reference's training loop (train.py:96,141-142) —
//     torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)   then   Adam(lr, weight_decay).step()
// as TWO launches over all parameter tensors at once instead of ~6 foreach kernels x 80 tensors:
//
//   gradsq_kernel   per 16 K-element chunk of every gradient: sum of squares -> partials[chunk]
//   clip_adam_kernel  every workgroup folds the partials (a few thousand floats, L2-resident) into the global norm and the
//                   clip coefficient min(1, max_norm / (norm + 1e-6)) — no third launch, no host read — then applies to
//                   its chunk:  g *= coef (in place, like clip_grad_norm_);  g += wd * p;  m = lerp(m, g, 1 - b1);
//                   v = b2 * v + (1 - b2) * g * g;  p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)      (torch's Adam, :142)
//                   Tensors with p == NULL are clip-only: the reference's lazily created point_pool_proj is in
//                   model.parameters() (so in the norm and scaled) but not in the optimizer.
//
// Capturable form (wf3d_clip_adam_step_dev): the Adam step and optionally lr are read from device memory, so that one
// captured launch sequence is right on every replay; a third launch advances the per-tensor step counters after the last
// Adam launch (no workgroup of the step can see an advanced counter).
//
// Grouped form (wf3d_clip_adam_step_groups): up to 16 parameter groups, each with its own lr (a value or a device
// scalar), betas, eps, weight decay (L2, or decoupled as in AdamW) and, in the host form, its own Adam step; in the
// capturable form every tensor's bias corrections come from its own counter.  The norm and the coefficient stay global.
// The group table rides in the kernel arguments, so a launch carries 48 tensors instead of 80; the partial sums are
// the same launches and the same positions as in the single-group form, so equal hyper-parameters give equal bits.
// All forms are ONE kernel template and one host routine over two tensor tables: WideTab (80 tensors, one group, one
// step pointer) and GroupedTab (48 tensors, a step pointer and a group index per tensor, 16 groups).
// With WF3D_ADAM_SKIP_NONFINITE a step whose norm is NaN or infinite writes nothing but the norm and a skipped-step
// count.  The sum of squares is an fp32 sum: finite gradients whose squares overflow it (norm above 1.8e19) count as
// non-finite too.
//
// HBM-bound: reads p, g, m, v and writes p, g, m, v once: 32 B per parameter (0.99 GB for the 31 M parameters).
// Tensor tables travel as kernel arguments (<= 80 tensors per launch), so per-step gradient reallocation costs nothing.
#include <math.h>

#include "wf3d_common.h"

namespace {

constexpr int OPT_CHUNK = 16384;          // elements per workgroup
constexpr int OPT_MAXT = 80;              // tensors per launch (kernel-argument budget: 80 x 40 B + 81 x 4 B < 4 KB)

struct SqArgs {
    const float* g[OPT_MAXT];
    long n[OPT_MAXT];
    int blk_begin[OPT_MAXT + 1];
    int ntensors;
};

constexpr int OPT_MAXS = 256;             // step counters per advance launch (256 x 8 B + 4 B)

struct StepArgs {
    float* s[OPT_MAXS];
    int n;
};

constexpr int OPT_MAXG = 16;              // parameter groups
constexpr int OPT_GMAXT = 48;             // tensors per grouped launch: the 16-group table takes the room of the other 32

// the hyper-parameters of NG parameter groups, one column per group; every derived scalar is formed in double before its
// one rounding to fp32, as torch does on the host: 1 - 0.999 must become 0.001f, not 1.0f - 0.999f (off by 5e-5)
template <int NG>
struct GroupTab {
    const float* lr_dev[NG];              // NULL: lr[k]
    double beta1d[NG], beta2d[NG];        // the capturable form's bias corrections are formed in double
    float lr[NG], beta1[NG], omb1[NG], beta2[NG], omb2[NG], eps[NG], wd[NG];
    float bc1[NG], bc2_sqrt[NG];          // the host form's, per group, from its 1-based step
    unsigned decoupled;                   // bit k: group k decays the parameter (AdamW), not the gradient

    void set(int k, double lr_, const float* lr_dev_, double b1, double b2, double eps_, double wd_, bool dec, int step) {
        lr_dev[k] = lr_dev_;
        beta1d[k] = b1; beta2d[k] = b2;
        lr[k] = (float)lr_; eps[k] = (float)eps_; wd[k] = (float)wd_;
        beta1[k] = (float)b1; omb1[k] = (float)(1.0 - b1);
        beta2[k] = (float)b2; omb2[k] = (float)(1.0 - b2);
        if (step) {
            bc1[k] = (float)(1.0 - pow(b1, (double)step));
            bc2_sqrt[k] = (float)sqrt(1.0 - pow(b2, (double)step));
        }
        if (dec) decoupled |= 1u << k;
    }
};

template <int MAXT_>
struct TensorTab {
    static constexpr int MAXT = MAXT_;
    float* p[MAXT];
    float* g[MAXT];
    float* m[MAXT];
    float* v[MAXT];
    long n[MAXT];
    int blk_begin[MAXT + 1];
    int ntensors;
};

// one group, so no group index, and ONE step pointer: the first optimised tensor's (every optimised tensor is at the
// same step, the caller's rule).  bind() keeps the first it is given, through all launches of a step.
struct WideTab : TensorTab<OPT_MAXT> {
    using Groups = GroupTab<1>;
    static constexpr bool SKIPS = false;  // no entry point asks the single-group form for the non-finite skip
    const float* step0;
    __device__ const float* step(int) const { return step0; }
    __device__ int group(int) const { return 0; }
    void bind(int i, const float* s, int) { if (p[i] && !step0) step0 = s; }
};

struct GroupedTab : TensorTab<OPT_GMAXT> {
    using Groups = GroupTab<OPT_MAXG>;
    static constexpr bool SKIPS = true;
    const float* steps[MAXT];             // capturable form: the tensor's own counter
    unsigned char groups[MAXT];
    __device__ const float* step(int t) const { return steps[t]; }
    __device__ int group(int t) const { return groups[t]; }
    void bind(int i, const float* s, int k) { steps[i] = s; groups[i] = p[i] ? (unsigned char)k : 0; }
};
static_assert(sizeof(WideTab) + sizeof(WideTab::Groups) + 64 <= 4096, "kernel-argument budget");
static_assert(sizeof(GroupedTab) + sizeof(GroupedTab::Groups) + 64 <= 4096, "kernel-argument budget");

template <typename A>
__device__ __forceinline__ int find_tensor(const A& a, int blk) {
    int lo = 0, hi = a.ntensors - 1;                 // last t with blk_begin[t] <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.blk_begin[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ float block_sum(float v, float* s_red) {
    v = wf3d_wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
    float t = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += s_red[w];       // every thread, same order
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(256) void gradsq_kernel(const SqArgs a, float* __restrict__ partials, int part_off) {
    __shared__ float s_red[4];
    const int t = find_tensor(a, blockIdx.x);
    const long base = (long)(blockIdx.x - a.blk_begin[t]) * OPT_CHUNK;
    const long n = a.n[t];
    const float* g = a.g[t];
    const long end = base + OPT_CHUNK < n ? base + OPT_CHUNK : n;
    float s = 0.f;
    if ((((uintptr_t)g) & 15) == 0) {
        for (long i = base + threadIdx.x * 4; i < end; i += 1024) {
            if (i + 4 <= end) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(g + i);
                s += x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3];
            } else {
                for (long j = i; j < end; ++j) s += g[j] * g[j];
            }
        }
    } else {
        for (long i = base + threadIdx.x; i < end; i += 256) s += g[i] * g[i];
    }
    s = block_sum(s, s_red);
    if (threadIdx.x == 0) partials[part_off + blockIdx.x] = s;
}

// every workgroup folds the same partials in the same order: one norm, bit for bit, across workgroups and launches
__device__ __forceinline__ float fold_norm(const float* __restrict__ partials, int npart, float* s_red) {
    float s = 0.f;
    for (int i = threadIdx.x; i < npart; i += 256) s += partials[i];
    return sqrtf(block_sum(s, s_red));
}

__device__ __forceinline__ float clip_coef(float norm, float max_norm) {
    const float coef = max_norm / (norm + 1e-6f);                // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1)
    // max_norm <= 0: no clipping.  A NaN norm must poison every gradient as clip_grad_norm_ does (torch.clamp keeps the
    // NaN): fminf(NaN, 1) would return 1 and let a step with a non-finite gradient through unscaled.
    return max_norm > 0.f ? (norm != norm ? norm : fminf(coef, 1.0f)) : 1.0f;
}

// one workgroup's chunk [base, end) of one tensor: upd(p, g, m, v) per element, as f32x4 where all four are 16-byte
// aligned
template <typename F>
__device__ __forceinline__ void walk_chunk(float* p, float* g, float* m, float* v, long base, long end, F upd) {
    const bool vec = (((uintptr_t)g | (uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
    if (vec) {
        for (long i = base + threadIdx.x * 4; i < end; i += 1024) {
            if (i + 4 <= end) {
                f32x4 pp = *reinterpret_cast<f32x4*>(p + i), gg = *reinterpret_cast<f32x4*>(g + i);
                f32x4 mm = *reinterpret_cast<f32x4*>(m + i), vv = *reinterpret_cast<f32x4*>(v + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float a0 = pp[e], a1 = gg[e], a2 = mm[e], a3 = vv[e];
                    upd(a0, a1, a2, a3);
                    pp[e] = a0; gg[e] = a1; mm[e] = a2; vv[e] = a3;
                }
                *reinterpret_cast<f32x4*>(p + i) = pp; *reinterpret_cast<f32x4*>(g + i) = gg;
                *reinterpret_cast<f32x4*>(m + i) = mm; *reinterpret_cast<f32x4*>(v + i) = vv;
            } else {
                for (long j = i; j < end; ++j) upd(p[j], g[j], m[j], v[j]);
            }
        }
    } else {
        for (long i = base + threadIdx.x; i < end; i += 256) upd(p[i], g[i], m[i], v[i]);
    }
}

// The Adam launch of every form: one global norm and one coefficient over every tensor, the Adam hyper-parameters per
// parameter group of the table A, the Adam step (DEV: read from the device) per A::step().
// SKIP: a norm that is NaN or infinite (an fp32 overflow of the sum of squares included) ends every workgroup before
// its first store; the norm itself is still reported.  All workgroups of all launches of a step take the same decision:
// they fold the same partials to the same bits.
template <typename A, bool DEV, bool SKIP>
__global__ __launch_bounds__(256) void clip_adam_kernel(const A a, const typename A::Groups gt,
                                                         const float* __restrict__ partials, int npart, float max_norm,
                                                         float* __restrict__ norm_out) {
    __shared__ float s_red[4];
    const float norm = fold_norm(partials, npart, s_red);
    const float coef = clip_coef(norm, max_norm);
    if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) *norm_out = norm;
    if (SKIP && !(norm < INFINITY)) return;
    const int t = find_tensor(a, blockIdx.x);
    const long base = (long)(blockIdx.x - a.blk_begin[t]) * OPT_CHUNK;
    const long n = a.n[t];
    const long end = base + OPT_CHUNK < n ? base + OPT_CHUNK : n;
    float* p = a.p[t];
    if (p == nullptr) {                               // clip-only: no group, no counter
        float* g = a.g[t];
        for (long i = base + threadIdx.x; i < end; i += 256) g[i] *= coef;
        return;
    }
    const int k = a.group(t);
    float bc1 = gt.bc1[k], bc2_sqrt = gt.bc2_sqrt[k];
    if (DEV) {
        // as the host forms them: in double from the 1-based step (the counter holds the step BEFORE this update, as
        // torch.optim.Adam(capturable=True)'s state["step"]), one rounding to fp32
        const double ts = (double)*a.step(t) + 1.0;
        bc1 = (float)(1.0 - pow(gt.beta1d[k], ts));
        bc2_sqrt = (float)sqrt(1.0 - pow(gt.beta2d[k], ts));
    }
    const float lr = gt.lr_dev[k] ? *gt.lr_dev[k] : gt.lr[k];
    const float beta1 = gt.beta1[k], omb1 = gt.omb1[k], beta2 = gt.beta2[k], omb2 = gt.omb2[k], eps = gt.eps[k], wd = gt.wd[k];
    const float step = lr / bc1;
    // both moments from the gradient ge that enters them; returns the Adam decrement
    auto adam = [&](float ge, float& mm, float& vv) {
        // exp_avg.lerp_(grad, 1 - beta1), from the nearer end as torch.lerp does: at beta1 <= 0.5 (weight >= 0.5) the
        // form m + w (ge - m) leaves a rounding of m's size in a result of ge's size, which sqrt(v) ~ |ge| then divides
        mm = omb1 < 0.5f ? fmaf(omb1, ge - mm, mm) : fmaf(-beta1, ge - mm, ge);
        vv = fmaf(omb2 * ge, ge, beta2 * vv);             // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
        return step * (mm / (sqrtf(vv) / bc2_sqrt + eps));
    };
    if (!((gt.decoupled >> k) & 1)) {
        walk_chunk(p, a.g[t], a.m[t], a.v[t], base, end, [&](float& pp, float& gg, float& mm, float& vv) {
            gg *= coef;                                   // the clipped gradient is what stays in .grad
            pp -= adam(fmaf(wd, pp, gg), mm, vv);         // L2 weight decay folded into the gradient (torch Adam)
        });
    } else {
        // decoupled decay (torch.optim.AdamW: p *= 1 - lr wd, then the Adam step): the gradient enters the moments
        // as it is, and the whole decrement is formed before the one subtraction, so p is rounded once
        const float lrwd = lr * wd;
        walk_chunk(p, a.g[t], a.m[t], a.v[t], base, end, [&](float& pp, float& gg, float& mm, float& vv) {
            gg *= coef;
            const float d = fmaf(lrwd, pp, adam(gg, mm, vv));
            pp -= d;
        });
    }
}

__global__ __launch_bounds__(256) void step_advance_kernel(const StepArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < a.n) a.s[i][0] += 1.0f;
}

// the advance of a step that may have been skipped: decided from the stored norm as the Adam launches decided from the
// partials (norm is that sum's square root); `skipped`, non-NULL in one launch of a step, counts the skipped steps
__global__ __launch_bounds__(256) void step_advance_finite_kernel(const StepArgs a, const float* __restrict__ norm,
                                                                   int64_t* __restrict__ skipped) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (!(*norm < INFINITY)) {
        if (i == 0 && skipped) *skipped += 1;
        return;
    }
    if (i < a.n) a.s[i][0] += 1.0f;
}

}  // namespace

extern "C" size_t wf3d_clip_adam_ws_floats(const long* numel, int ntensors) {
    size_t blocks = 0;
    for (int i = 0; i < ntensors; ++i) blocks += (size_t)wf3d_cdiv(numel[i] > 0 ? numel[i] : 1, OPT_CHUNK);
    return blocks + 1;
}

// The first half of every form: the tables are checked, then partials[c] = the sum of squares of chunk c, chunks
// numbered through the whole table in order.  Neither the number nor the position of a partial depends on how the
// tensors are cut into launches, here or in the Adam launches that fold them.
static int gradsq_launch(const char* fn, float* const* params, float* const* grads, float* const* exp_avg,
                         float* const* exp_avg_sq, const long* numel, int ntensors, float* ws, size_t ws_floats, hipStream_t st,
                         int* npart_out) {
    WF3D_CHECK(ws && ws_floats >= wf3d_clip_adam_ws_floats(numel, ntensors), WF3D_ERR_WS, "%s: workspace too small", fn);
    for (int i = 0; i < ntensors; ++i) {
        WF3D_CHECK(grads[i] && numel[i] > 0, WF3D_ERR_ARG, "%s: tensor %d has no gradient", fn, i);
        WF3D_CHECK(!params[i] || (exp_avg[i] && exp_avg_sq[i]), WF3D_ERR_ARG, "%s: tensor %d lacks optimizer state", fn, i);
    }
    int npart = 0;
    for (int t0 = 0; t0 < ntensors; t0 += OPT_MAXT) {
        const int nt = ntensors - t0 < OPT_MAXT ? ntensors - t0 : OPT_MAXT;
        SqArgs a;
        a.ntensors = nt;
        int blk = 0;
        for (int i = 0; i < nt; ++i) {
            a.g[i] = grads[t0 + i]; a.n[i] = numel[t0 + i]; a.blk_begin[i] = blk;
            blk += wf3d_cdiv(numel[t0 + i], OPT_CHUNK);
        }
        for (int i = nt; i <= OPT_MAXT; ++i) a.blk_begin[i] = blk;
        hipLaunchKernelGGL(gradsq_kernel, dim3(blk), dim3(256), 0, st, a, ws, npart);
        WF3D_LAUNCH_CHECK();
        npart += blk;
    }
    *npart_out = npart;
    return WF3D_OK;
}

// The capturable forms' last launches, after the last Adam launch on the same stream: no workgroup of this step reads an
// advanced counter.  norm non-NULL (the skip flag): the counters stay where a non-finite *norm stopped the step, and the
// first launch (there is one even without counters) adds that step to *skipped.
static int advance_steps(float* const* params, float* const* steps, int ntensors, const float* norm, int64_t* skipped,
                         hipStream_t st) {
    StepArgs a;
    a.n = 0;
    bool first = true;
    auto flush = [&]() {
        const dim3 grid(a.n ? wf3d_cdiv(a.n, 256) : 1);
        if (norm)
            hipLaunchKernelGGL(step_advance_finite_kernel, grid, dim3(256), 0, st, a, norm, first ? skipped : nullptr);
        else
            hipLaunchKernelGGL(step_advance_kernel, grid, dim3(256), 0, st, a);
        first = false;
        a.n = 0;
    };
    for (int i = 0; i < ntensors; ++i) {
        if (!params[i]) continue;
        a.s[a.n++] = steps[i];
        if (a.n == OPT_MAXS) {
            flush();
            WF3D_LAUNCH_CHECK();
        }
    }
    if (a.n || (norm && first)) {
        flush();
        WF3D_LAUNCH_CHECK();
    }
    return WF3D_OK;
}

// The whole step of every form over tensor tables of type A, cut after A::MAXT tensors: the sums of squares, the Adam
// launches and, in the capturable form (steps non-NULL), the counter advance.  group NULL: every tensor in group 0.
template <typename A>
static int clip_adam_run(const char* fn, float* const* params, float* const* grads, float* const* exp_avg,
                         float* const* exp_avg_sq, const long* numel, const int* group, float* const* steps, int ntensors,
                         const typename A::Groups& gt, double max_norm, bool skip, int64_t* skipped, float* ws,
                         size_t ws_floats, float* total_norm, hipStream_t st) {
    int npart = 0;
    const int rc = gradsq_launch(fn, params, grads, exp_avg, exp_avg_sq, numel, ntensors, ws, ws_floats, st, &npart);
    if (rc) return rc;
    auto kern = steps ? &clip_adam_kernel<A, true, false> : &clip_adam_kernel<A, false, false>;
    if constexpr (A::SKIPS)
        if (skip) kern = &clip_adam_kernel<A, true, true>;
    A a = {};                                             // one table for all launches: WideTab keeps its step pointer
    for (int t0 = 0; t0 < ntensors; t0 += A::MAXT) {
        const int nt = ntensors - t0 < A::MAXT ? ntensors - t0 : A::MAXT;
        a.ntensors = nt;
        int blk = 0;
        for (int i = 0; i < nt; ++i) {
            a.p[i] = params[t0 + i]; a.g[i] = grads[t0 + i]; a.m[i] = exp_avg[t0 + i]; a.v[i] = exp_avg_sq[t0 + i];
            a.n[i] = numel[t0 + i]; a.blk_begin[i] = blk;
            a.bind(i, steps ? steps[t0 + i] : nullptr, group ? group[t0 + i] : 0);
            blk += wf3d_cdiv(numel[t0 + i], OPT_CHUNK);
        }
        for (int i = nt; i <= A::MAXT; ++i) a.blk_begin[i] = blk;
        hipLaunchKernelGGL(kern, dim3(blk), dim3(256), 0, st, a, gt, ws, npart, (float)max_norm, t0 == 0 ? total_norm : nullptr);
        WF3D_LAUNCH_CHECK();
    }
    if (!steps) return WF3D_OK;
    return advance_steps(params, steps, ntensors, skip ? total_norm : nullptr, skipped, st);
}

extern "C" int wf3d_clip_adam_step(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                   const long* numel, int ntensors, double max_norm, double lr, double beta1, double beta2,
                                   double eps, double weight_decay, int step, float* ws, size_t ws_floats, float* total_norm,
                                   void* stream) {
    WF3D_CHECK(ntensors >= 0 && params && grads && exp_avg && exp_avg_sq && numel, WF3D_ERR_ARG, "wf3d_clip_adam_step: null table");
    if (ntensors == 0) return WF3D_OK;
    WF3D_CHECK(step >= 1 && lr >= 0. && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1., WF3D_ERR_ARG, "wf3d_clip_adam_step: bad hyper-parameters");
    GroupTab<1> gt = {};
    gt.set(0, lr, nullptr, beta1, beta2, eps, weight_decay, false, step);
    return clip_adam_run<WideTab>("wf3d_clip_adam_step", params, grads, exp_avg, exp_avg_sq, numel, nullptr, nullptr, ntensors, gt,
                                  max_norm, false, nullptr, ws, ws_floats, total_norm, (hipStream_t)stream);
}

extern "C" int wf3d_clip_adam_step_dev(float* const* params, float* const* grads, float* const* exp_avg,
                                       float* const* exp_avg_sq, float* const* steps, const long* numel, int ntensors,
                                       double max_norm, double lr, const float* lr_dev, double beta1, double beta2, double eps,
                                       double weight_decay, float* ws, size_t ws_floats, float* total_norm, void* stream) {
    WF3D_CHECK(ntensors >= 0 && params && grads && exp_avg && exp_avg_sq && steps && numel, WF3D_ERR_ARG,
               "wf3d_clip_adam_step_dev: null table");
    if (ntensors == 0) return WF3D_OK;
    WF3D_CHECK(lr >= 0. && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1., WF3D_ERR_ARG,
               "wf3d_clip_adam_step_dev: bad hyper-parameters");
    for (int i = 0; i < ntensors; ++i)
        WF3D_CHECK(!params[i] || steps[i], WF3D_ERR_ARG, "wf3d_clip_adam_step_dev: tensor %d has no step counter", i);
    // every optimised tensor is at the same step (the caller's rule): the first one's counter gives the bias corrections.
    // A table of clip-only tensors has none, and no workgroup reads one.
    GroupTab<1> gt = {};
    gt.set(0, lr, lr_dev, beta1, beta2, eps, weight_decay, false, 0);
    return clip_adam_run<WideTab>("wf3d_clip_adam_step_dev", params, grads, exp_avg, exp_avg_sq, numel, nullptr, steps, ntensors,
                                  gt, max_norm, false, nullptr, ws, ws_floats, total_norm, (hipStream_t)stream);
}

extern "C" int wf3d_clip_adam_step_groups(float* const* params, float* const* grads, float* const* exp_avg,
                                          float* const* exp_avg_sq, const long* numel, const int* group, float* const* steps,
                                          int ntensors, const double* lr, const float* const* lr_dev, const double* beta1,
                                          const double* beta2, const double* eps, const double* weight_decay,
                                          const int* decoupled, const int* step, int ngroups, double max_norm, int flags,
                                          int64_t* skipped, float* ws, size_t ws_floats, float* total_norm, void* stream) {
    const char* fn = "wf3d_clip_adam_step_groups";
    WF3D_CHECK(ntensors >= 0 && params && grads && exp_avg && exp_avg_sq && numel && group, WF3D_ERR_ARG, "%s: null table", fn);
    WF3D_CHECK(ngroups >= 0 && ngroups <= OPT_MAXG, WF3D_ERR_UNSUPPORTED, "%s: %d parameter groups (at most %d)", fn, ngroups,
               OPT_MAXG);
    WF3D_CHECK(!ngroups || (lr && beta1 && beta2 && eps && weight_decay && decoupled && (steps || step)), WF3D_ERR_ARG,
               "%s: null group table", fn);
    WF3D_CHECK(!(flags & ~WF3D_ADAM_SKIP_NONFINITE), WF3D_ERR_ARG, "%s: unknown flags %#x", fn, (unsigned)flags);
    const bool skip = flags & WF3D_ADAM_SKIP_NONFINITE;
    // the host form advances its steps on the host, where nobody knows whether the device skipped
    WF3D_CHECK(!skip || (steps && skipped && total_norm), WF3D_ERR_ARG,
               "%s: WF3D_ADAM_SKIP_NONFINITE needs device step counters, a skipped-step counter and total_norm", fn);
    if (ntensors == 0) return WF3D_OK;
    GroupTab<OPT_MAXG> gt = {};
    for (int k = 0; k < ngroups; ++k) {
        WF3D_CHECK(lr[k] >= 0. && beta1[k] >= 0. && beta1[k] < 1. && beta2[k] >= 0. && beta2[k] < 1. && (steps || step[k] >= 1),
                   WF3D_ERR_ARG, "%s: bad hyper-parameters in group %d", fn, k);
        gt.set(k, lr[k], lr_dev ? lr_dev[k] : nullptr, beta1[k], beta2[k], eps[k], weight_decay[k], decoupled[k], steps ? 0 : step[k]);
    }
    for (int i = 0; i < ntensors; ++i) {
        if (!params[i]) continue;
        WF3D_CHECK(group[i] >= 0 && group[i] < ngroups, WF3D_ERR_ARG, "%s: tensor %d is in group %d of %d", fn, i, group[i], ngroups);
        WF3D_CHECK(!steps || steps[i], WF3D_ERR_ARG, "%s: tensor %d has no step counter", fn, i);
    }
    return clip_adam_run<GroupedTab>(fn, params, grads, exp_avg, exp_avg_sq, numel, group, steps, ntensors, gt, max_norm, skip,
                                     skipped, ws, ws_floats, total_norm, (hipStream_t)stream);
}

