// The argument block of the attention kernels (attn.hip: VALU, any head width; attn_mfma.hip: MFMA, head_dim 64 and the
// multiples of 4 up to 128), its builder, and the one launch helper.  wf3d_attn_fwd / wf3d_attn_bwd (attn.hip) validate, build the block once and
// launch the VALU kernels themselves or hand the block to wf3d_attn_mfma_launch.
#pragma once
#include "wf3d_common.h"

struct AttnArgs {
    const float* qkv;      // [Rv, 3E]
    float* ctx;            // [Rv, E]      forward out; backward reads it (through a const pointer)
    float* lse;            // [Rv, heads]  forward out; backward reads it
    const float* dctx;     // bwd in  [Rv, E]
    float* dqkv;           // bwd out [Rv, 3E]
    const int32_t* voff;   // [S+1]
    int E, heads, hd;
    int rows;              // rows reserved per staged operand in LDS; set by whoever sizes the LDS of the launch
                           // (wf3d_attn_launch refuses 0)
    float scale;           // 1 / sqrt(hd)
    wf3d_seed_t seed; uint32_t thresh; float dscale;      // thresh == 0: no dropout
};

// from the arguments of wf3d_attn_fwd (dctx = dqkv = NULL) / wf3d_attn_bwd; everything but `rows`
static inline AttnArgs wf3d_attn_args(const float* qkv, const int32_t* voff, int E, int heads, float drop_p,
                                      uint32_t drop_seed, const float* ctx, const float* lse, const float* dctx,
                                      float* dqkv) {
    AttnArgs a{};
    a.qkv = qkv; a.ctx = (float*)ctx; a.lse = (float*)lse; a.dctx = dctx; a.dqkv = dqkv; a.voff = voff;
    a.E = E; a.heads = heads; a.hd = E / heads;
    a.scale = 1.0f / sqrtf((float)a.hd);
    if (drop_p > 0.f) { const wf3d_drop_t d = wf3d_drop_args(drop_p, drop_seed); a.seed = d.seed; a.thresh = d.thresh; a.dscale = d.scale; }
    return a;
}

// launch `kernel` (256 threads) with `lds` bytes of dynamic LDS; beyond the 64 KiB a kernel may use without asking, its
// limit is raised first
template <typename K>
static int wf3d_attn_launch(const char* who, K kernel, dim3 grid, size_t lds, const AttnArgs& p, hipStream_t stream) {
    WF3D_CHECK(p.rows > 0, WF3D_ERR_ARG, "%s: the LDS rows of the launch are not set", who);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        WF3D_CHECK(e == hipSuccess, WF3D_ERR_LAUNCH, "%s: cannot raise dynamic LDS to %zu", who, lds);
    }
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, p);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

// The MFMA kernels (attn_mfma.hip): family 1 = sample resident in LDS (head_dim 64, vmax <= 256), 2 = key-tiled (any
// vmax; head_dim 64, or 68..128 on the kernels of padded width 96 / 128 chosen from p.hd); the families are attn.hip's
// attn_family.  Owns their LDS layout (`rows`), LDS sizes and launches.
WF3D_INTERNAL int wf3d_attn_mfma_launch(AttnArgs p, int family, bool backward, int S, int vmax, hipStream_t stream);
