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

// the device-side scalars of the capturable form (unused by the host-step launch)
struct AdamDev {
    const float* step;    // the Adam step BEFORE this update (torch.optim.Adam(capturable=True) state["step"])
    const float* lr;      // NULL: the lr argument
    double beta1, beta2;
};

struct AdamArgs {
    float* p[OPT_MAXT];
    float* g[OPT_MAXT];
    float* m[OPT_MAXT];
    float* v[OPT_MAXT];
    long n[OPT_MAXT];
    int blk_begin[OPT_MAXT + 1];
    int ntensors;
};

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
// aligned; p == NULL: a clip-only tensor, g *= coef
template <typename F>
__device__ __forceinline__ void walk_chunk(float* p, float* g, float* m, float* v, long base, long end, float coef, F upd) {
    const bool vec = (((uintptr_t)g | (uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
    if (p == nullptr) {                               // clip-only tensor
        for (long i = base + threadIdx.x; i < end; i += 256) g[i] *= coef;
        return;
    }
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

template <bool DEV>
__global__ __launch_bounds__(256) void clip_adam_kernel(const AdamArgs a, const float* __restrict__ partials, int npart,
                                                         float max_norm, float lr, float beta1, float omb1, float beta2,
                                                         float omb2, float eps, float wd, float bc1, float bc2_sqrt,
                                                         float* __restrict__ norm_out, const AdamDev dv) {
    __shared__ float s_red[4];
    if (DEV) {
        // as the host forms them: in double from the 1-based step, one rounding to fp32
        const double t = (double)*dv.step + 1.0;
        bc1 = (float)(1.0 - pow(dv.beta1, t));
        bc2_sqrt = (float)sqrt(1.0 - pow(dv.beta2, t));
        if (dv.lr) lr = *dv.lr;
    }
    const float norm = fold_norm(partials, npart, s_red);
    const float coef = clip_coef(norm, max_norm);
    if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) *norm_out = norm;
    const int t = find_tensor(a, blockIdx.x);
    const long base = (long)(blockIdx.x - a.blk_begin[t]) * OPT_CHUNK;
    const long n = a.n[t];
    const long end = base + OPT_CHUNK < n ? base + OPT_CHUNK : n;
    const float step = lr / bc1;      // omb1 = 1 - beta1, omb2 = 1 - beta2 come rounded from double (1.0f - 0.999f is off by 5e-5)
    walk_chunk(a.p[t], a.g[t], a.m[t], a.v[t], base, end, coef, [&](float& pp, float& gg, float& mm, float& vv) {
        gg *= coef;                                   // the clipped gradient is what stays in .grad
        const float ge = fmaf(wd, pp, gg);            // L2 weight decay folded into the gradient (torch Adam)
        // exp_avg.lerp_(grad, 1 - beta1), from the nearer end as torch.lerp does: at beta1 <= 0.5 (weight >= 0.5) the
        // form m + w (ge - m) leaves a rounding of m's size in a result of ge's size, which sqrt(v) ~ |ge| then divides
        mm = omb1 < 0.5f ? fmaf(omb1, ge - mm, mm) : fmaf(-beta1, ge - mm, ge);
        vv = fmaf(omb2 * ge, ge, beta2 * vv);         // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
        pp -= step * (mm / (sqrtf(vv) / bc2_sqrt + eps));
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// Grouped form (wf3d_clip_adam_step_groups): one global norm and one coefficient over every tensor, the Adam
// hyper-parameters per parameter group, the Adam step per group (host form) or per tensor (capturable form).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int OPT_MAXG = 16;              // parameter groups
constexpr int OPT_GMAXT = 48;             // tensors per grouped launch: the group table takes the room of the other 32

struct GroupTab {
    const float* lr_dev[OPT_MAXG];        // NULL: lr[k]
    double beta1d[OPT_MAXG], beta2d[OPT_MAXG];                    // the capturable form's bias corrections are formed in double
    float lr[OPT_MAXG], beta1[OPT_MAXG], omb1[OPT_MAXG], beta2[OPT_MAXG], omb2[OPT_MAXG], eps[OPT_MAXG], wd[OPT_MAXG];
    float bc1[OPT_MAXG], bc2_sqrt[OPT_MAXG];                      // the host form's, per group
    unsigned decoupled;                   // bit k: group k decays the parameter (AdamW), not the gradient
};

struct GroupAdamArgs {
    float* p[OPT_GMAXT];
    float* g[OPT_GMAXT];
    float* m[OPT_GMAXT];
    float* v[OPT_GMAXT];
    const float* step[OPT_GMAXT];         // capturable form: the tensor's own counter
    long n[OPT_GMAXT];
    int blk_begin[OPT_GMAXT + 1];
    int ntensors;
    unsigned char group[OPT_GMAXT];
};
static_assert(sizeof(GroupAdamArgs) + sizeof(GroupTab) + 64 <= 4096, "kernel-argument budget");

// SKIP: a norm that is NaN or infinite (an fp32 overflow of the sum of squares included) ends every workgroup before
// its first store; the norm itself is still reported.  All workgroups of all launches of a step take the same decision:
// they fold the same partials to the same bits.
template <bool DEV, bool SKIP>
__global__ __launch_bounds__(256) void clip_adam_groups_kernel(const GroupAdamArgs a, const GroupTab gt,
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
    const int k = a.group[t];
    float bc1 = gt.bc1[k], bc2_sqrt = gt.bc2_sqrt[k];
    if (DEV) {
        const double ts = (double)*a.step[t] + 1.0;   // as the host forms them, from this tensor's own step
        bc1 = (float)(1.0 - pow(gt.beta1d[k], ts));
        bc2_sqrt = (float)sqrt(1.0 - pow(gt.beta2d[k], ts));
    }
    const float lr = gt.lr_dev[k] ? *gt.lr_dev[k] : gt.lr[k];
    const float beta1 = gt.beta1[k], omb1 = gt.omb1[k], beta2 = gt.beta2[k], omb2 = gt.omb2[k], eps = gt.eps[k], wd = gt.wd[k];
    const float step = lr / bc1;
    if (!((gt.decoupled >> k) & 1)) {
        // L2 decay: clip_adam_kernel's expression, unchanged
        walk_chunk(p, a.g[t], a.m[t], a.v[t], base, end, coef, [&](float& pp, float& gg, float& mm, float& vv) {
            gg *= coef;
            const float ge = fmaf(wd, pp, gg);
            mm = omb1 < 0.5f ? fmaf(omb1, ge - mm, mm) : fmaf(-beta1, ge - mm, ge);
            vv = fmaf(omb2 * ge, ge, beta2 * vv);
            pp -= step * (mm / (sqrtf(vv) / bc2_sqrt + eps));
        });
    } else {
        // decoupled decay (torch.optim.AdamW: p *= 1 - lr wd, then the Adam step): the gradient enters the moments
        // as it is, and the whole decrement is formed before the one subtraction, so p is rounded once
        const float lrwd = lr * wd;
        walk_chunk(p, a.g[t], a.m[t], a.v[t], base, end, coef, [&](float& pp, float& gg, float& mm, float& vv) {
            gg *= coef;
            mm = omb1 < 0.5f ? fmaf(omb1, gg - mm, mm) : fmaf(-beta1, gg - mm, gg);
            vv = fmaf(omb2 * gg, gg, beta2 * vv);
            const float d = fmaf(lrwd, pp, step * (mm / (sqrtf(vv) / bc2_sqrt + eps)));
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

// shared by the two single-group entry points: `dv` null for the host step (bc1 / bc2_sqrt given), else the capturable form
static int clip_adam_launch(const char* fn, float* const* params, float* const* grads, float* const* exp_avg,
                            float* const* exp_avg_sq, const long* numel, int ntensors, double max_norm, double lr, double beta1,
                            double beta2, double eps, double weight_decay, float bc1, float bc2_sqrt, const AdamDev* dv,
                            float* ws, size_t ws_floats, float* total_norm, hipStream_t st) {
    int npart = 0;
    const int rc = gradsq_launch(fn, params, grads, exp_avg, exp_avg_sq, numel, ntensors, ws, ws_floats, st, &npart);
    if (rc) return rc;
    for (int t0 = 0; t0 < ntensors; t0 += OPT_MAXT) {
        const int nt = ntensors - t0 < OPT_MAXT ? ntensors - t0 : OPT_MAXT;
        AdamArgs a;
        a.ntensors = nt;
        int blk = 0;
        for (int i = 0; i < nt; ++i) {
            a.p[i] = params[t0 + i]; a.g[i] = grads[t0 + i]; a.m[i] = exp_avg[t0 + i]; a.v[i] = exp_avg_sq[t0 + i];
            a.n[i] = numel[t0 + i]; a.blk_begin[i] = blk;
            blk += wf3d_cdiv(numel[t0 + i], OPT_CHUNK);
        }
        for (int i = nt; i <= OPT_MAXT; ++i) a.blk_begin[i] = blk;
        if (dv)
            hipLaunchKernelGGL(clip_adam_kernel<true>, dim3(blk), dim3(256), 0, st, a, ws, npart, (float)max_norm, (float)lr,
                               (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay, 0.f,
                               0.f, t0 == 0 ? total_norm : nullptr, *dv);
        else
            hipLaunchKernelGGL(clip_adam_kernel<false>, dim3(blk), dim3(256), 0, st, a, ws, npart, (float)max_norm, (float)lr,
                               (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay, bc1,
                               bc2_sqrt, t0 == 0 ? total_norm : nullptr, AdamDev{});
        WF3D_LAUNCH_CHECK();
    }
    return WF3D_OK;
}

extern "C" int wf3d_clip_adam_step(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                   const long* numel, int ntensors, double max_norm, double lr, double beta1, double beta2,
                                   double eps, double weight_decay, int step, float* ws, size_t ws_floats, float* total_norm,
                                   void* stream) {
    WF3D_CHECK(ntensors >= 0 && params && grads && exp_avg && exp_avg_sq && numel, WF3D_ERR_ARG, "wf3d_clip_adam_step: null table");
    if (ntensors == 0) return WF3D_OK;
    WF3D_CHECK(step >= 1 && lr >= 0. && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1., WF3D_ERR_ARG, "wf3d_clip_adam_step: bad hyper-parameters");
    // hyper-parameters arrive as doubles (Python floats) and every derived scalar is formed in double before the one
    // rounding to fp32, as torch does on the host: 1 - 0.999 must become 0.001f, not 1.0f - 0.999f
    const float bc1 = (float)(1.0 - pow(beta1, (double)step));
    const float bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)step));
    return clip_adam_launch("wf3d_clip_adam_step", params, grads, exp_avg, exp_avg_sq, numel, ntensors, max_norm, lr, beta1,
                            beta2, eps, weight_decay, bc1, bc2_sqrt, nullptr, ws, ws_floats, total_norm, (hipStream_t)stream);
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

extern "C" int wf3d_clip_adam_step_dev(float* const* params, float* const* grads, float* const* exp_avg,
                                       float* const* exp_avg_sq, float* const* steps, const long* numel, int ntensors,
                                       double max_norm, double lr, const float* lr_dev, double beta1, double beta2, double eps,
                                       double weight_decay, float* ws, size_t ws_floats, float* total_norm, void* stream) {
    WF3D_CHECK(ntensors >= 0 && params && grads && exp_avg && exp_avg_sq && steps && numel, WF3D_ERR_ARG,
               "wf3d_clip_adam_step_dev: null table");
    if (ntensors == 0) return WF3D_OK;
    WF3D_CHECK(lr >= 0. && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1., WF3D_ERR_ARG,
               "wf3d_clip_adam_step_dev: bad hyper-parameters");
    const float* step0 = nullptr;
    for (int i = 0; i < ntensors; ++i) {
        WF3D_CHECK(!params[i] || steps[i], WF3D_ERR_ARG, "wf3d_clip_adam_step_dev: tensor %d has no step counter", i);
        if (params[i] && !step0) step0 = steps[i];
    }
    hipStream_t st = (hipStream_t)stream;
    if (step0) {
        // every optimised tensor is at the same step (the caller's rule): the first one's counter gives the bias corrections
        const AdamDev dv{step0, lr_dev, beta1, beta2};
        const int rc = clip_adam_launch("wf3d_clip_adam_step_dev", params, grads, exp_avg, exp_avg_sq, numel, ntensors, max_norm,
                                        lr, beta1, beta2, eps, weight_decay, 0.f, 0.f, &dv, ws, ws_floats, total_norm, st);
        if (rc) return rc;
    } else {
        // clip-only tensors: the step counter never enters
        const int rc = clip_adam_launch("wf3d_clip_adam_step_dev", params, grads, exp_avg, exp_avg_sq, numel, ntensors, max_norm,
                                        lr, beta1, beta2, eps, weight_decay, 1.f, 1.f, nullptr, ws, ws_floats, total_norm, st);
        if (rc) return rc;
    }
    return advance_steps(params, steps, ntensors, nullptr, nullptr, st);
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
    GroupTab gt = {};
    for (int k = 0; k < ngroups; ++k) {
        WF3D_CHECK(lr[k] >= 0. && beta1[k] >= 0. && beta1[k] < 1. && beta2[k] >= 0. && beta2[k] < 1. && (steps || step[k] >= 1),
                   WF3D_ERR_ARG, "%s: bad hyper-parameters in group %d", fn, k);
        // every derived scalar in double before its one rounding to fp32, as in the single-group forms
        gt.lr_dev[k] = lr_dev ? lr_dev[k] : nullptr;
        gt.beta1d[k] = beta1[k]; gt.beta2d[k] = beta2[k];
        gt.lr[k] = (float)lr[k]; gt.eps[k] = (float)eps[k]; gt.wd[k] = (float)weight_decay[k];
        gt.beta1[k] = (float)beta1[k]; gt.omb1[k] = (float)(1.0 - beta1[k]);
        gt.beta2[k] = (float)beta2[k]; gt.omb2[k] = (float)(1.0 - beta2[k]);
        if (!steps) {
            gt.bc1[k] = (float)(1.0 - pow(beta1[k], (double)step[k]));
            gt.bc2_sqrt[k] = (float)sqrt(1.0 - pow(beta2[k], (double)step[k]));
        }
        if (decoupled[k]) gt.decoupled |= 1u << k;
    }
    for (int i = 0; i < ntensors; ++i) {
        if (!params[i]) continue;
        WF3D_CHECK(group[i] >= 0 && group[i] < ngroups, WF3D_ERR_ARG, "%s: tensor %d is in group %d of %d", fn, i, group[i], ngroups);
        WF3D_CHECK(!steps || steps[i], WF3D_ERR_ARG, "%s: tensor %d has no step counter", fn, i);
    }
    hipStream_t st = (hipStream_t)stream;
    int npart = 0;
    int rc = gradsq_launch(fn, params, grads, exp_avg, exp_avg_sq, numel, ntensors, ws, ws_floats, st, &npart);
    if (rc) return rc;
    for (int t0 = 0; t0 < ntensors; t0 += OPT_GMAXT) {
        const int nt = ntensors - t0 < OPT_GMAXT ? ntensors - t0 : OPT_GMAXT;
        GroupAdamArgs a = {};
        a.ntensors = nt;
        int blk = 0;
        for (int i = 0; i < nt; ++i) {
            a.p[i] = params[t0 + i]; a.g[i] = grads[t0 + i]; a.m[i] = exp_avg[t0 + i]; a.v[i] = exp_avg_sq[t0 + i];
            a.step[i] = steps ? steps[t0 + i] : nullptr;
            a.group[i] = params[t0 + i] ? (unsigned char)group[t0 + i] : 0;
            a.n[i] = numel[t0 + i]; a.blk_begin[i] = blk;
            blk += wf3d_cdiv(numel[t0 + i], OPT_CHUNK);
        }
        for (int i = nt; i <= OPT_GMAXT; ++i) a.blk_begin[i] = blk;
        float* norm_out = t0 == 0 ? total_norm : nullptr;
        const float mx = (float)max_norm;
        if (steps && skip)
            hipLaunchKernelGGL((clip_adam_groups_kernel<true, true>), dim3(blk), dim3(256), 0, st, a, gt, ws, npart, mx, norm_out);
        else if (steps)
            hipLaunchKernelGGL((clip_adam_groups_kernel<true, false>), dim3(blk), dim3(256), 0, st, a, gt, ws, npart, mx, norm_out);
        else
            hipLaunchKernelGGL((clip_adam_groups_kernel<false, false>), dim3(blk), dim3(256), 0, st, a, gt, ws, npart, mx, norm_out);
        WF3D_LAUNCH_CHECK();
    }
    if (!steps) return WF3D_OK;
    return advance_steps(params, steps, ntensors, skip ? total_norm : nullptr, skipped, st);
}
