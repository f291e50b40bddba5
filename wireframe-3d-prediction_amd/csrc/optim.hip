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
// All forms are ONE kernel template and one host routine over three tensor tables: WideTab (80 tensors, one group, one
// step pointer), GroupedTab (48 tensors, a step pointer and a group index per tensor, 16 groups) and EmaTab (GroupedTab
// with an average per tensor, 40 tensors).
// With WF3D_ADAM_SKIP_NONFINITE a step whose norm is NaN or infinite writes nothing but the norm and a skipped-step
// count.  The sum of squares is an fp32 sum: finite gradients whose squares overflow it (norm above 1.8e19) count as
// non-finite too.
//
// Averaged weights (wf3d_clip_adam_step_ema): a tensor with an EMA pointer gets ema = fmaf(1 - d, p' - ema, ema) from the
// parameter value p' that the same thread has just stored, 40 B per parameter instead of a second pass of 12.  The fifth
// pointer takes the EMA form's table down to 40 tensors (EmaTab); the partial sums do not move, so p, g, m, v and the
// norm keep the bits of the step without the average.  wf3d_ema_swap exchanges parameters and averages.
// Learning-rate schedules (wf3d_lr_schedule): one thread per group evaluates warm-up x decay in double from a device
// int64 count of applied updates and writes float(lr * factor) where the Adam launches read their lr_dev; the count
// advances with the Adam counters, in the same launch and under the same finite-norm decision.
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

template <int MAXT_>
struct PerTensorTab : TensorTab<MAXT_> {
    using Groups = GroupTab<OPT_MAXG>;
    static constexpr bool SKIPS = true;
    const float* steps[MAXT_];            // capturable form: the tensor's own counter
    unsigned char groups[MAXT_];
    __device__ const float* step(int t) const { return steps[t]; }
    __device__ int group(int t) const { return groups[t]; }
    void bind(int i, const float* s, int k) { steps[i] = s; groups[i] = this->p[i] ? (unsigned char)k : 0; }
};

struct GroupedTab : PerTensorTab<OPT_GMAXT> {};

constexpr int OPT_EMAXT = 40;             // tensors per EMA launch: the fifth pointer and the decay rows take the room of 8

// the grouped table with an average per tensor: ema' = fmaf(1 - d, p' - ema, ema) after the parameter's store
struct EmaTab : PerTensorTab<OPT_EMAXT> {
    float* ema[OPT_EMAXT];                // NULL: the tensor keeps no average
    double decay[OPT_MAXG];               // d per group, for the warm-up that the capturable form evaluates per tensor
    float omd[OPT_MAXG];                  // 1 - d, rounded once from double (host form with warm-up: at the group's step)
    int warmup;                           // capturable form: d = min(decay, (1 + n) / (10 + n)), n = the tensor's counter
};
template <typename A> constexpr bool has_ema = false;
template <> constexpr bool has_ema<EmaTab> = true;
static_assert(sizeof(WideTab) + sizeof(WideTab::Groups) + 64 <= 4096, "kernel-argument budget");
static_assert(sizeof(GroupedTab) + sizeof(GroupedTab::Groups) + 64 <= 4096, "kernel-argument budget");
static_assert(sizeof(EmaTab) + sizeof(EmaTab::Groups) + 64 <= 4096, "kernel-argument budget");

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

// one workgroup's chunk [base, end) of one tensor: upd(p, g, m, v) per element, as f32x4 where all pointers are 16-byte
// aligned.  E: the tensor has an average e, which follows the parameter value that upd left (the one that is stored)
// by ema' = fmaf(omd, p' - ema, ema), whichever decay branch upd is
template <bool E, typename F>
__device__ __forceinline__ void walk_chunk(float* p, float* g, float* m, float* v, float* e, float omd, long base, long end,
                                           F upd) {
    const bool vec = (((uintptr_t)g | (uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (E ? (uintptr_t)e : 0)) & 15) == 0;
    auto one = [&](long j) {
        float a0 = p[j], a1 = g[j], a2 = m[j], a3 = v[j];
        upd(a0, a1, a2, a3);
        p[j] = a0; g[j] = a1; m[j] = a2; v[j] = a3;
        if (E) {
            const float a4 = e[j];
            e[j] = fmaf(omd, a0 - a4, a4);
        }
    };
    if (vec) {
        for (long i = base + threadIdx.x * 4; i < end; i += 1024) {
            if (i + 4 <= end) {
                f32x4 pp = *reinterpret_cast<f32x4*>(p + i), gg = *reinterpret_cast<f32x4*>(g + i);
                f32x4 mm = *reinterpret_cast<f32x4*>(m + i), vv = *reinterpret_cast<f32x4*>(v + i);
                f32x4 ee = {};
                if (E) ee = *reinterpret_cast<f32x4*>(e + i);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float a0 = pp[c], a1 = gg[c], a2 = mm[c], a3 = vv[c];
                    upd(a0, a1, a2, a3);
                    pp[c] = a0; gg[c] = a1; mm[c] = a2; vv[c] = a3;
                    if (E) ee[c] = fmaf(omd, a0 - ee[c], ee[c]);
                }
                *reinterpret_cast<f32x4*>(p + i) = pp; *reinterpret_cast<f32x4*>(g + i) = gg;
                *reinterpret_cast<f32x4*>(m + i) = mm; *reinterpret_cast<f32x4*>(v + i) = vv;
                if (E) *reinterpret_cast<f32x4*>(e + i) = ee;
            } else {
                for (long j = i; j < end; ++j) one(j);
            }
        }
    } else {
        for (long i = base + threadIdx.x; i < end; i += 256) one(i);
    }
}

// The Adam launch of every form: one global norm and one coefficient over every tensor, the Adam hyper-parameters per
// parameter group of the table A, the Adam step (DEV: read from the device) per A::step().
// SKIP: a norm that is NaN or infinite (an fp32 overflow of the sum of squares included) ends every workgroup before
// its first store; the norm itself is still reported.  All workgroups of all launches of a step take the same decision:
// they fold the same partials to the same bits.
// EMA (A = EmaTab): a tensor with a.ema[t] updates its average in the same pass, after the parameter; a skipped step
// returns before it, a clip-only tensor has none, and lr = 0 still moves it towards the unchanged parameter.
template <typename A, bool DEV, bool SKIP, bool EMA>
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
    float* e = nullptr;
    float omd = 0.f;
    if constexpr (EMA) {
        e = a.ema[t];
        omd = a.omd[k];
        if (DEV && a.warmup) {
            // as the host forms it: in double from the tensor's Adam step BEFORE this update, 1 - d rounded once
            const double n = (double)*a.step(t);
            omd = (float)(1.0 - fmin(a.decay[k], (1.0 + n) / (10.0 + n)));
        }
    }
    auto walk = [&](auto upd) {
        if constexpr (EMA) {
            if (e) {
                walk_chunk<true>(p, a.g[t], a.m[t], a.v[t], e, omd, base, end, upd);
                return;
            }
        }
        walk_chunk<false>(p, a.g[t], a.m[t], a.v[t], nullptr, 0.f, base, end, upd);
    };
    if (!((gt.decoupled >> k) & 1)) {
        walk([&](float& pp, float& gg, float& mm, float& vv) {
            gg *= coef;                                   // the clipped gradient is what stays in .grad
            pp -= adam(fmaf(wd, pp, gg), mm, vv);         // L2 weight decay folded into the gradient (torch Adam)
        });
    } else {
        // decoupled decay (torch.optim.AdamW: p *= 1 - lr wd, then the Adam step): the gradient enters the moments
        // as it is, and the whole decrement is formed before the one subtraction, so p is rounded once
        const float lrwd = lr * wd;
        walk([&](float& pp, float& gg, float& mm, float& vv) {
            gg *= coef;
            const float d = fmaf(lrwd, pp, adam(gg, mm, vv));
            pp -= d;
        });
    }
}

// one thread per parameter group: the rate of the update that comes next, float(lr * factor(*step)), where the Adam
// launches of the same step read it.  The rows are wf3d.optim.lr_factor's, evaluated in double without contraction.
constexpr int OPT_MAXMS = 8;              // milestones of a multistep decay

struct SchedTab {
    double lr[OPT_MAXG], warmup_start[OPT_MAXG], min_factor[OPT_MAXG], gamma[OPT_MAXG];
    long warmup_steps[OPT_MAXG], decay_steps[OPT_MAXG], milestones[OPT_MAXG][OPT_MAXMS];
    unsigned char decay[OPT_MAXG], nmilestones[OPT_MAXG], write[OPT_MAXG];
    int ngroups;
};
static_assert(sizeof(SchedTab) + 64 <= 4096, "kernel-argument budget");

__global__ __launch_bounds__(64) void lr_schedule_kernel(const SchedTab s, const int64_t* __restrict__ step,
                                                         float* __restrict__ last_lr) {
#pragma clang fp contract(off)
    const int k = threadIdx.x;
    if (k >= s.ngroups || !s.write[k]) return;
    const long t = (long)*step, W = s.warmup_steps[k], T = s.decay_steps[k];
    const double ws = s.warmup_start[k], mf = s.min_factor[k];
    const double fw = t < W ? ws + (1.0 - ws) * (double)t / (double)W : 1.0;
    const long u = t > W ? t - W : 0;
    double fd = 1.0;                                             // T >= 1 where a decay reads it
    switch (s.decay[k]) {
        case WF3D_LR_COSINE: fd = mf + (1.0 - mf) * 0.5 * (1.0 + cos(M_PI * (double)(u < T ? u : T) / (double)T)); break;
        case WF3D_LR_LINEAR: fd = 1.0 + (mf - 1.0) * (double)(u < T ? u : T) / (double)T; break;
        case WF3D_LR_EXPONENTIAL: fd = fmax(pow(s.gamma[k], (double)u), mf); break;
        case WF3D_LR_MULTISTEP: {
            int c = 0;
            for (int i = 0; i < s.nmilestones[k]; ++i) c += s.milestones[k][i] <= u;
            fd = pow(s.gamma[k], (double)c);
            break;
        }
        default: break;
    }
    last_lr[k] = (float)(s.lr[k] * (fw * fd));
}

// parameters and their averages change places: chunks as in gradsq_kernel, f32x4 where both are 16-byte aligned
struct SwapArgs {
    float* a[OPT_MAXT];
    float* b[OPT_MAXT];
    long n[OPT_MAXT];
    int blk_begin[OPT_MAXT + 1];
    int ntensors;
};

__global__ __launch_bounds__(256) void ema_swap_kernel(const SwapArgs s) {
    const int t = find_tensor(s, blockIdx.x);
    const long base = (long)(blockIdx.x - s.blk_begin[t]) * OPT_CHUNK;
    const long n = s.n[t];
    const long end = base + OPT_CHUNK < n ? base + OPT_CHUNK : n;
    float* a = s.a[t];
    float* b = s.b[t];
    auto one = [&](long j) {
        const float x = a[j];
        a[j] = b[j];
        b[j] = x;
    };
    if ((((uintptr_t)a | (uintptr_t)b) & 15) == 0) {
        for (long i = base + threadIdx.x * 4; i < end; i += 1024) {
            if (i + 4 <= end) {
                const f32x4 x = *reinterpret_cast<f32x4*>(a + i), y = *reinterpret_cast<f32x4*>(b + i);
                *reinterpret_cast<f32x4*>(a + i) = y;
                *reinterpret_cast<f32x4*>(b + i) = x;
            } else {
                for (long j = i; j < end; ++j) one(j);
            }
        }
    } else {
        for (long i = base + threadIdx.x; i < end; i += 256) one(i);
    }
}

// `sched`, non-NULL in the first launch of a step: the schedules' count of applied updates, which moves when at least
// one Adam counter does (int64: an fp32 counter stops being exact at 2^24)
__global__ __launch_bounds__(256) void step_advance_kernel(const StepArgs a, int64_t* __restrict__ sched) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0 && sched && a.n > 0) *sched += 1;
    if (i < a.n) a.s[i][0] += 1.0f;
}

// the advance of a step that may have been skipped: decided from the stored norm as the Adam launches decided from the
// partials (norm is that sum's square root); `skipped`, non-NULL in one launch of a step, counts the skipped steps
__global__ __launch_bounds__(256) void step_advance_finite_kernel(const StepArgs a, const float* __restrict__ norm,
                                                                   int64_t* __restrict__ skipped, int64_t* __restrict__ sched) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (!(*norm < INFINITY)) {
        if (i == 0 && skipped) *skipped += 1;
        return;
    }
    if (i == 0 && sched && a.n > 0) *sched += 1;
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
                         int64_t* sched, hipStream_t st) {
    StepArgs a;
    a.n = 0;
    bool first = true;
    auto flush = [&]() {
        const dim3 grid(a.n ? wf3d_cdiv(a.n, 256) : 1);
        if (norm)
            hipLaunchKernelGGL(step_advance_finite_kernel, grid, dim3(256), 0, st, a, norm, first ? skipped : nullptr,
                               first ? sched : nullptr);
        else
            hipLaunchKernelGGL(step_advance_kernel, grid, dim3(256), 0, st, a, first ? sched : nullptr);
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
// `a` arrives with what its type holds beside the tensors (EmaTab: the decay rows); ema and sched (the schedules' count
// of applied updates) are NULL in the forms that have none.
template <typename A>
static int clip_adam_run(const char* fn, A a, float* const* params, float* const* grads, float* const* exp_avg,
                         float* const* exp_avg_sq, float* const* ema, const long* numel, const int* group,
                         float* const* steps, int ntensors, const typename A::Groups& gt, double max_norm, bool skip,
                         int64_t* skipped, int64_t* sched, float* ws, size_t ws_floats, float* total_norm, hipStream_t st) {
    int npart = 0;
    const int rc = gradsq_launch(fn, params, grads, exp_avg, exp_avg_sq, numel, ntensors, ws, ws_floats, st, &npart);
    if (rc) return rc;
    constexpr bool EMA = has_ema<A>;
    auto kern = steps ? &clip_adam_kernel<A, true, false, EMA> : &clip_adam_kernel<A, false, false, EMA>;
    if constexpr (A::SKIPS)
        if (skip) kern = &clip_adam_kernel<A, true, true, EMA>;
    // `a` is one table for all launches: WideTab keeps its step pointer
    for (int t0 = 0; t0 < ntensors; t0 += A::MAXT) {
        const int nt = ntensors - t0 < A::MAXT ? ntensors - t0 : A::MAXT;
        a.ntensors = nt;
        int blk = 0;
        for (int i = 0; i < nt; ++i) {
            a.p[i] = params[t0 + i]; a.g[i] = grads[t0 + i]; a.m[i] = exp_avg[t0 + i]; a.v[i] = exp_avg_sq[t0 + i];
            a.n[i] = numel[t0 + i]; a.blk_begin[i] = blk;
            if constexpr (EMA) a.ema[i] = params[t0 + i] ? ema[t0 + i] : nullptr;
            a.bind(i, steps ? steps[t0 + i] : nullptr, group ? group[t0 + i] : 0);
            blk += wf3d_cdiv(numel[t0 + i], OPT_CHUNK);
        }
        for (int i = nt; i <= A::MAXT; ++i) a.blk_begin[i] = blk;
        hipLaunchKernelGGL(kern, dim3(blk), dim3(256), 0, st, a, gt, ws, npart, (float)max_norm, t0 == 0 ? total_norm : nullptr);
        WF3D_LAUNCH_CHECK();
    }
    if (!steps) return WF3D_OK;
    return advance_steps(params, steps, ntensors, skip ? total_norm : nullptr, skipped, sched, st);
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
    return clip_adam_run("wf3d_clip_adam_step", WideTab{}, params, grads, exp_avg, exp_avg_sq, nullptr, numel, nullptr, nullptr,
                         ntensors, gt, max_norm, false, nullptr, nullptr, ws, ws_floats, total_norm, (hipStream_t)stream);
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
    return clip_adam_run("wf3d_clip_adam_step_dev", WideTab{}, params, grads, exp_avg, exp_avg_sq, nullptr, numel, nullptr, steps,
                         ntensors, gt, max_norm, false, nullptr, nullptr, ws, ws_floats, total_norm, (hipStream_t)stream);
}

// The grouped entry points' common body.  ema NULL: wf3d_clip_adam_step_groups' tables and kernels, whoever calls.
static int clip_adam_groups(const char* fn, float* const* params, float* const* grads, float* const* exp_avg,
                            float* const* exp_avg_sq, float* const* ema, const long* numel, const int* group,
                            float* const* steps, int ntensors, const double* lr, const float* const* lr_dev,
                            const double* beta1, const double* beta2, const double* eps, const double* weight_decay,
                            const int* decoupled, const double* ema_decay, const int* step, int ngroups, double max_norm,
                            int flags, int known_flags, int64_t* skipped, int64_t* sched, float* ws, size_t ws_floats,
                            float* total_norm, void* stream) {
    WF3D_CHECK(ntensors >= 0 && params && grads && exp_avg && exp_avg_sq && numel && group, WF3D_ERR_ARG, "%s: null table", fn);
    WF3D_CHECK(ngroups >= 0 && ngroups <= OPT_MAXG, WF3D_ERR_UNSUPPORTED, "%s: %d parameter groups (at most %d)", fn, ngroups,
               OPT_MAXG);
    WF3D_CHECK(!ngroups || (lr && beta1 && beta2 && eps && weight_decay && decoupled && (steps || step)), WF3D_ERR_ARG,
               "%s: null group table", fn);
    WF3D_CHECK(!(flags & ~known_flags), WF3D_ERR_ARG, "%s: unknown flags %#x", fn, (unsigned)flags);
    const bool skip = flags & WF3D_ADAM_SKIP_NONFINITE;
    // the host form advances its steps on the host, where nobody knows whether the device skipped
    WF3D_CHECK(!skip || (steps && skipped && total_norm), WF3D_ERR_ARG,
               "%s: WF3D_ADAM_SKIP_NONFINITE needs device step counters, a skipped-step counter and total_norm", fn);
    WF3D_CHECK(!sched || steps, WF3D_ERR_ARG, "%s: schedule_step needs device step counters (the host form counts on the host)", fn);
    WF3D_CHECK(!ema || !ngroups || ema_decay, WF3D_ERR_ARG, "%s: an ema table needs ema_decay", fn);
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
    if (!ema)
        return clip_adam_run(fn, GroupedTab{}, params, grads, exp_avg, exp_avg_sq, nullptr, numel, group, steps, ntensors, gt,
                             max_norm, skip, skipped, sched, ws, ws_floats, total_norm, (hipStream_t)stream);
    const bool warm = flags & WF3D_ADAM_EMA_WARMUP;
    EmaTab a = {};
    a.warmup = warm && steps;
    for (int k = 0; k < ngroups; ++k) {
        double d = ema_decay[k];
        WF3D_CHECK(d >= 0. && d < 1., WF3D_ERR_ARG, "%s: ema_decay %g of group %d is outside [0, 1)", fn, d, k);
        a.decay[k] = d;
        if (warm && !steps) {                             // the group's step before this update, as the kernel's n
            const double n = (double)(step[k] - 1);
            d = fmin(d, (1.0 + n) / (10.0 + n));
        }
        a.omd[k] = (float)(1.0 - d);
    }
    for (int i = 0; i < ntensors; ++i)
        WF3D_CHECK(!ema[i] || (params[i] && ema_decay[group[i]] > 0.), WF3D_ERR_ARG,
                   "%s: tensor %d has an average but no parameter, or its group no ema_decay", fn, i);
    return clip_adam_run(fn, a, params, grads, exp_avg, exp_avg_sq, ema, numel, group, steps, ntensors, gt, max_norm, skip,
                         skipped, sched, ws, ws_floats, total_norm, (hipStream_t)stream);
}

extern "C" int wf3d_clip_adam_step_groups(float* const* params, float* const* grads, float* const* exp_avg,
                                          float* const* exp_avg_sq, const long* numel, const int* group, float* const* steps,
                                          int ntensors, const double* lr, const float* const* lr_dev, const double* beta1,
                                          const double* beta2, const double* eps, const double* weight_decay,
                                          const int* decoupled, const int* step, int ngroups, double max_norm, int flags,
                                          int64_t* skipped, float* ws, size_t ws_floats, float* total_norm, void* stream) {
    return clip_adam_groups("wf3d_clip_adam_step_groups", params, grads, exp_avg, exp_avg_sq, nullptr, numel, group, steps,
                            ntensors, lr, lr_dev, beta1, beta2, eps, weight_decay, decoupled, nullptr, step, ngroups, max_norm,
                            flags, WF3D_ADAM_SKIP_NONFINITE, skipped, nullptr, ws, ws_floats, total_norm, stream);
}

extern "C" int wf3d_clip_adam_step_ema(float* const* params, float* const* grads, float* const* exp_avg,
                                       float* const* exp_avg_sq, float* const* ema, const long* numel, const int* group,
                                       float* const* steps, int ntensors, const double* lr, const float* const* lr_dev,
                                       const double* beta1, const double* beta2, const double* eps,
                                       const double* weight_decay, const int* decoupled, const double* ema_decay,
                                       const int* step, int ngroups, double max_norm, int flags, int64_t* skipped,
                                       int64_t* schedule_step, float* ws, size_t ws_floats, float* total_norm,
                                       void* stream) {
    return clip_adam_groups("wf3d_clip_adam_step_ema", params, grads, exp_avg, exp_avg_sq, ema, numel, group, steps, ntensors,
                            lr, lr_dev, beta1, beta2, eps, weight_decay, decoupled, ema_decay, step, ngroups, max_norm, flags,
                            WF3D_ADAM_SKIP_NONFINITE | WF3D_ADAM_EMA_WARMUP, skipped, schedule_step, ws, ws_floats,
                            total_norm, stream);
}

extern "C" int wf3d_lr_schedule(const double* lr, const long* warmup_steps, const double* warmup_start, const int* decay,
                                const long* decay_steps, const double* min_factor, const double* gamma,
                                const long* milestones, const int* nmilestones, const int* write, int ngroups,
                                const int64_t* schedule_step, float* last_lr, void* stream) {
    const char* fn = "wf3d_lr_schedule";
    WF3D_CHECK(ngroups >= 0 && ngroups <= OPT_MAXG, WF3D_ERR_UNSUPPORTED, "%s: %d parameter groups (at most %d)", fn, ngroups,
               OPT_MAXG);
    if (ngroups == 0) return WF3D_OK;
    WF3D_CHECK(lr && warmup_steps && warmup_start && decay && decay_steps && min_factor && gamma && milestones && nmilestones &&
               write && schedule_step && last_lr, WF3D_ERR_ARG, "%s: null table", fn);
    SchedTab s = {};
    s.ngroups = ngroups;
    for (int k = 0; k < ngroups; ++k) {
        const int kind = decay[k], nm = nmilestones[k];
        const bool timed = kind == WF3D_LR_COSINE || kind == WF3D_LR_LINEAR;
        WF3D_CHECK(lr[k] >= 0. && warmup_steps[k] >= 0 && warmup_start[k] >= 0. && warmup_start[k] <= 1. &&
                   kind >= WF3D_LR_CONSTANT && kind <= WF3D_LR_MULTISTEP && (!timed || decay_steps[k] >= 1) &&
                   min_factor[k] >= 0. && min_factor[k] <= 1. && nm >= 0 && nm <= OPT_MAXMS &&
                   (kind < WF3D_LR_EXPONENTIAL || (gamma[k] > 0. && gamma[k] <= 1.)),
                   WF3D_ERR_ARG, "%s: bad schedule in group %d", fn, k);
        for (int i = 0; i < nm; ++i) {
            WF3D_CHECK(milestones[k * OPT_MAXMS + i] >= (i ? milestones[k * OPT_MAXMS + i - 1] : 0), WF3D_ERR_ARG,
                       "%s: the milestones of group %d decrease", fn, k);
            s.milestones[k][i] = milestones[k * OPT_MAXMS + i];
        }
        s.lr[k] = lr[k]; s.warmup_start[k] = warmup_start[k]; s.min_factor[k] = min_factor[k]; s.gamma[k] = gamma[k];
        s.warmup_steps[k] = warmup_steps[k]; s.decay_steps[k] = decay_steps[k];
        s.decay[k] = (unsigned char)kind; s.nmilestones[k] = (unsigned char)nm; s.write[k] = write[k] != 0;
    }
    hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, s, schedule_step, last_lr);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" int wf3d_ema_swap(float* const* params, float* const* ema, const long* numel, int ntensors, void* stream) {
    const char* fn = "wf3d_ema_swap";
    WF3D_CHECK(ntensors >= 0 && (!ntensors || (params && ema && numel)), WF3D_ERR_ARG, "%s: null table", fn);
    for (int i = 0; i < ntensors; ++i)
        WF3D_CHECK(params[i] && ema[i] && params[i] != ema[i] && numel[i] > 0, WF3D_ERR_ARG, "%s: tensor %d lacks a side", fn, i);
    for (int t0 = 0; t0 < ntensors; t0 += OPT_MAXT) {
        const int nt = ntensors - t0 < OPT_MAXT ? ntensors - t0 : OPT_MAXT;
        SwapArgs s;
        s.ntensors = nt;
        int blk = 0;
        for (int i = 0; i < nt; ++i) {
            s.a[i] = params[t0 + i]; s.b[i] = ema[t0 + i]; s.n[i] = numel[t0 + i]; s.blk_begin[i] = blk;
            blk += wf3d_cdiv(numel[t0 + i], OPT_CHUNK);
        }
        for (int i = nt; i <= OPT_MAXT; ++i) s.blk_begin[i] = blk;
        hipLaunchKernelGGL(ema_swap_kernel, dim3(blk), dim3(256), 0, (hipStream_t)stream, s);
        WF3D_LAUNCH_CHECK();
    }
    return WF3D_OK;
}

