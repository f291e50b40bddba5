// MFMA self-attention for head_dim = 64 (the reference's 512/8) and, key-tiled only, for every head_dim that is a
// multiple of 4 in 68..128 (512/4, 1024/8, 768/8, ...; "key-tiled, head widths 64 < hd <= 128" below): exact-fp32 matrix
// cores (v_mfma_f32_32x32x2_f32), 256 threads, each wave64 owning 32-row query (or key) blocks while the other operand's
// rows sit in LDS.  Widths up to 60 and above 128 have no kernel here (attn.hip's VALU kernels serve them).
//
// Orientation trick: the score tile is computed TRANSPOSED, S^T = K·Q^T, so that the softmax axis
// (keys) runs over a lane's accumulator registers (+ one exchange with lane^32) and never across
// lanes, and the probability tile is already the B operand of the next contraction
// O^T = V^T·P^T, which sums over the accumulator's ROW index (cdna_hip_programming.md §3 "An
// accumulator tile as the next MFMA's operand"): MFMA step e pairs k = row(e, half 0) with
// row(e, half 1), i.e. B = acc register e as it stands; A = V[row(e, half)][d] is one conflict-free
// ds_read_b32.  The reduction index d of QK^T is assigned as d = 32*(lane>>5) + step so a lane's
// operand is 32 contiguous floats of its row.
//
// Backward = two sweeps with the same LDS footprint (no atomics): sweep 1 per query block
// (S^T, dP^T = V·dO^T, dS^T, dQ^T = K^T·dS^T), sweep 2 per key block with the roles of rows and
// columns swapped (S = Q·K^T, dP = dO·V^T, dK^T = Q^T·dS, dV^T = dO^T·P).  delta_i = dO_i·O_i.
//
// Shared pieces ("tile steps" below): zero2, store_tile_row and row_delta serve every kernel; dq_tile (sweep 1 against a
// 32-row block of a K / V tile) and dkv_tile (sweep 2 against a 32-row block of a scaled-Q / dO tile with its lse and
// delta rows) state the backward arithmetic and serve the resident backward kernel.  Two ownership schemes:
//   resident (attn_fwd/bwd_mfma_kernel, up to 256 vertices): one workgroup per (head, sample) stages the WHOLE sample
//     once (the "tile" is the sample, first row 0), its waves loop over the 32-row blocks; softmax in two passes over
//     the sample's score tiles held in registers; backward restages between the sweeps in one launch.
//   key-tiled (attn_fwd_tiled_kernel, attn_bwd_tiled_dq/dkv_kernel, any vertex count): one workgroup per (head, sample,
//     group of 4 row blocks), each wave keeps ONE block for the whole kernel and the other operand is walked in tiles
//     of KT rows; online softmax; one launch per backward sweep.
// The key-tiled backward kernels keep dq_tile's / dkv_tile's body (first row k0 / i0 instead of 0) and their zero fill
// written out, and both forward kernels their score step (S^T tiles, key mask, running maximum): called as shared steps
// these compile to other instruction streams that measured 0.1 - 0.15 % (tiled backward, per kernel) and 0.5 - 0.9 %
// (forward) slower.  A change to one copy of a step goes into the other.
#include "attn_args.h"

namespace {

constexpr int HD = 64;
constexpr int LDR = HD + 4;                 // padded LDS row (floats): 16 lanes of a b128 group hit 16 slots

__device__ __forceinline__ int rowof(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// stage rows [r0, r0+n) x 64 columns (col0..) of src[*, ld] into dst[npad][LDR], zero rows >= n
__device__ __forceinline__ void stage64(float* dst, const float* __restrict__ src, int ld, int r0, int n, int npad,
                                        int col0, float mul) {
    for (int idx = threadIdx.x; idx < npad * 16; idx += blockDim.x) {
        const int r = idx >> 4, c = (idx & 15) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r < n) v = *reinterpret_cast<const f32x4*>(src + (size_t)(r0 + r) * ld + col0 + c) * mul;
        *reinterpret_cast<f32x4*>(dst + r * LDR + c) = v;
    }
}

// H contiguous floats (this lane's half of a 2H-wide row: H = 32 at head_dim 64) from global, zero when !ok
template <int H>
__device__ __forceinline__ void load_half_row(float (&f)[H], const float* __restrict__ p, bool ok, float mul) {
#pragma unroll
    for (int k = 0; k < H / 4; ++k) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ok) v = *reinterpret_cast<const f32x4*>(p + 4 * k);
#pragma unroll
        for (int j = 0; j < 4; ++j) f[4 * k + j] = v[j] * mul;
    }
}

// acc[32x32] += A·B with A rows read from LDS (row = arow, this lane's half), B = H register values
template <int H>
__device__ __forceinline__ f32x16 mm_rows_regs(const float* lds_row_half, const float (&b)[H]) {
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int k = 0; k < H / 4; ++k) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(lds_row_half + 4 * k);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[4 * k + j], acc, 0, 0, 0);
    }
    return acc;
}

// ---- tile steps ------------------------------------------------------------------------------------------------------
// A lane is (l31 = lane & 31: its row of the wave's 32-row block, h = lane >> 5: its half); a staged tile holds `nt`
// 32-row blocks and starts at row k0 (keys) or i0 (queries) of the sample.

__device__ __forceinline__ void zero2(f32x16 (&a)[2]) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) a[dt][e] = 0.f;
}

// this lane's row of a [32 rows x 64] transposed accumulator pair, times mul, to out[0..64)
__device__ __forceinline__ void store_tile_row(float* out, const f32x16 (&o)[2], int h, float mul) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v = {o[dt][4 * g], o[dt][4 * g + 1], o[dt][4 * g + 2], o[dt][4 * g + 3]};
            *reinterpret_cast<f32x4*>(out + dt * 32 + 8 * g + 4 * h) = v * mul;
        }
}

// delta_i = dO_i . O_i from this lane's half row of ctx (op; zero when !ok) and of dO (df), summed over both halves
__device__ __forceinline__ float row_delta(const float* op, bool ok, const float (&df)[32]) {
    float delta = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ok) v = *reinterpret_cast<const f32x4*>(op + 4 * k);
#pragma unroll
        for (int j = 0; j < 4; ++j) delta += v[j] * df[4 * k + j];
    }
    return delta + __shfl_xor(delta, 32, 64);
}

// backward sweep 1, block jt of a staged K / V tile: dq += (K block)^T · dS^T for this lane's query (mask row `row`,
// scaled q in qf, dO in df).
__device__ __forceinline__ void dq_tile(f32x16 (&dq)[2], const AttnArgs& p, uint32_t seed, const float* Ks,
                                        const float* Vs, int jt, int k0, int n, uint32_t row, const float (&qf)[32],
                                        const float (&df)[32], float lse_i, float delta, int l31, int h) {
    const f32x16 st = mm_rows_regs(Ks + (jt * 32 + l31) * LDR + 32 * h, qf);
    const f32x16 dp = mm_rows_regs(Vs + (jt * 32 + l31) * LDR + 32 * h, df);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int jl = jt * 32 + rowof(e, h), j = k0 + jl;
        const float pr = j < n ? expf(st[e] - lse_i) : 0.f;
        float g = dp[e];
        if (p.thresh) g = wf3d_keep(seed, row, (uint32_t)j, p.thresh) ? g * p.dscale : 0.f;
        const float ds = pr * (g - delta);
        const float* kr = Ks + jl * LDR + l31;
        dq[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[0], ds, dq[0], 0, 0, 0);
        dq[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[32], ds, dq[1], 0, 0, 0);
    }
}

// backward sweep 2, block `it` of a staged (scaled Q, dO) tile: dk += (Q block)^T · dS, dv += (dO block)^T · P~ for this
// lane's key j (k in kf, v in vf); dl / ls = delta_i / lse_i of the tile's rows (lse = +inf for padded queries); row0 =
// the tile's first row in [Rv, *].
__device__ __forceinline__ void dkv_tile(f32x16 (&dk)[2], f32x16 (&dv)[2], const AttnArgs& p, uint32_t seed,
                                         const float* Qs, const float* Gs, const float* dl, const float* ls, int it,
                                         int row0, int head, int j, const float (&kf)[32], const float (&vf)[32],
                                         int l31, int h) {
    const f32x16 sc = mm_rows_regs(Qs + (it * 32 + l31) * LDR + 32 * h, kf);     // S[i][j], rows = queries
    const f32x16 dp = mm_rows_regs(Gs + (it * 32 + l31) * LDR + 32 * h, vf);     // dP[i][j]
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int il = it * 32 + rowof(e, h);
        const float pr = expf(sc[e] - ls[il]);                                   // 0 for padded queries
        float mk = 1.0f;
        if (p.thresh) mk = wf3d_keep(seed, (uint32_t)((row0 + il) * p.heads + head), (uint32_t)j, p.thresh) ? p.dscale : 0.f;
        const float ds = pr * (dp[e] * mk - dl[il]);
        const float pt = pr * mk;
        const float* qr = Qs + il * LDR + l31;
        const float* gr = Gs + il * LDR + l31;
        dk[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(qr[0], ds, dk[0], 0, 0, 0);
        dk[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(qr[32], ds, dk[1], 0, 0, 0);
        dv[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(gr[0], pt, dv[0], 0, 0, 0);
        dv[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(gr[32], pt, dv[1], 0, 0, 0);
    }
}

// ---- resident: the sample's rows in LDS, p.rows (a multiple of 32) reserved per operand -----------------------------

__global__ __launch_bounds__(256, 1) void attn_fwd_mfma_kernel(const AttnArgs p) {
    const uint32_t seed = p.thresh ? wf3d_seed_load(p.seed) : 0u;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int head = blockIdx.x, s = blockIdx.y;
    const int r0 = p.voff[s], n = p.voff[s + 1] - r0;
    if (n <= 0) return;
    const int npad = (n + 31) & ~31, nt = npad >> 5;
    const int E3 = 3 * p.E;
    float* Ks = sm;
    float* Vs = sm + p.rows * LDR;
    stage64(Ks, p.qkv, E3, r0, n, npad, p.E + head * HD, 1.0f);
    stage64(Vs, p.qkv, E3, r0, n, npad, 2 * p.E + head * HD, 1.0f);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    for (int qb = wave; qb < nt; qb += 4) {
        const int i = qb * 32 + l31;                       // this lane's query
        const bool iok = i < n;
        float qf[32];
        load_half_row(qf, p.qkv + (size_t)(r0 + i) * E3 + head * HD + 32 * h, iok, p.scale);
        f32x16 st[8];                                      // S^T tiles: rows = keys, column = this lane's query
        float m = -INFINITY;
#pragma unroll
        for (int jt = 0; jt < 8; ++jt) {
            if (jt < nt) {
                st[jt] = mm_rows_regs(Ks + (jt * 32 + l31) * LDR + 32 * h, qf);
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    if (jt * 32 + rowof(e, h) >= n) st[jt][e] = -INFINITY;
                    m = fmaxf(m, st[jt][e]);
                }
            }
        }
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float l = 0.f;
#pragma unroll
        for (int jt = 0; jt < 8; ++jt) {
            if (jt < nt) {
#pragma unroll
                for (int e = 0; e < 16; ++e) { st[jt][e] = expf(st[jt][e] - m); l += st[jt][e]; }
            }
        }
        l += __shfl_xor(l, 32, 64);
        const float inv = 1.0f / l;
        if (iok && h == 0) p.lse[(size_t)(r0 + i) * p.heads + head] = m + logf(l);
        f32x16 o[2];
        zero2(o);
#pragma unroll
        for (int jt = 0; jt < 8; ++jt) {
            if (jt < nt) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int j = jt * 32 + rowof(e, h);
                    float pv = st[jt][e] * inv;
                    if (p.thresh) pv = wf3d_keep(seed, (uint32_t)((r0 + i) * p.heads + head), (uint32_t)j, p.thresh) ? pv * p.dscale : 0.f;
                    const float* vr = Vs + j * LDR + l31;
                    o[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[0], pv, o[0], 0, 0, 0);
                    o[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[32], pv, o[1], 0, 0, 0);
                }
            }
        }
        if (iok) store_tile_row(p.ctx + (size_t)(r0 + i) * p.E + head * HD, o, h, 1.0f);
    }
}

__global__ __launch_bounds__(256) void attn_bwd_mfma_kernel(const AttnArgs p) {
    const uint32_t seed = p.thresh ? wf3d_seed_load(p.seed) : 0u;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int head = blockIdx.x, s = blockIdx.y;
    const int r0 = p.voff[s], n = p.voff[s + 1] - r0;
    if (n <= 0) return;
    const int npad = (n + 31) & ~31, nt = npad >> 5;
    const int E3 = 3 * p.E;
    const float* ctx = p.ctx;
    float* Xa = sm;                                        // sweep 1: K        sweep 2: scaled Q
    float* Xb = sm + p.rows * LDR;                         // sweep 1: V        sweep 2: dO
    float* dl = Xb + p.rows * LDR;                         // [rows] delta_i
    float* ls = dl + p.rows;                               // [rows] lse_i (+inf for padded queries)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, h = lane >> 5;

    stage64(Xa, p.qkv, E3, r0, n, npad, p.E + head * HD, 1.0f);
    stage64(Xb, p.qkv, E3, r0, n, npad, 2 * p.E + head * HD, 1.0f);
    for (int i = threadIdx.x; i < npad; i += blockDim.x)
        ls[i] = i < n ? p.lse[(size_t)(r0 + i) * p.heads + head] : INFINITY;
    __syncthreads();
    // ---- sweep 1: per query block -> dQ, delta
    for (int qb = wave; qb < nt; qb += 4) {
        const int i = qb * 32 + l31;
        const bool iok = i < n;
        float qf[32], df[32];
        load_half_row(qf, p.qkv + (size_t)(r0 + i) * E3 + head * HD + 32 * h, iok, p.scale);
        load_half_row(df, p.dctx + (size_t)(r0 + i) * p.E + head * HD + 32 * h, iok, 1.0f);
        const float delta = row_delta(ctx + (size_t)(r0 + i) * p.E + head * HD + 32 * h, iok, df);
        if (h == 0) dl[i] = delta;
        const float lse_i = iok ? ls[i] : INFINITY;
        f32x16 dq[2];
        zero2(dq);
        for (int jt = 0; jt < nt; ++jt)
            dq_tile(dq, p, seed, Xa, Xb, jt, 0, n, (uint32_t)((r0 + i) * p.heads + head), qf, df, lse_i, delta, l31, h);
        if (iok) store_tile_row(p.dqkv + (size_t)(r0 + i) * E3 + head * HD, dq, h, p.scale);
    }
    __syncthreads();
    // ---- sweep 2: per key block -> dK, dV   (Xa = scaled Q, Xb = dO)
    stage64(Xa, p.qkv, E3, r0, n, npad, head * HD, p.scale);
    stage64(Xb, p.dctx, p.E, r0, n, npad, head * HD, 1.0f);
    __syncthreads();
    for (int kb = wave; kb < nt; kb += 4) {
        const int j = kb * 32 + l31;                       // this lane's key
        const bool jok = j < n;
        float kf[32], vf[32];
        load_half_row(kf, p.qkv + (size_t)(r0 + j) * E3 + p.E + head * HD + 32 * h, jok, 1.0f);
        load_half_row(vf, p.qkv + (size_t)(r0 + j) * E3 + 2 * p.E + head * HD + 32 * h, jok, 1.0f);
        f32x16 dk[2], dv[2];
        zero2(dk);
        zero2(dv);
        for (int it = 0; it < nt; ++it) dkv_tile(dk, dv, p, seed, Xa, Xb, dl, ls, it, r0, head, j, kf, vf, l31, h);
        if (jok) {
            store_tile_row(p.dqkv + (size_t)(r0 + j) * E3 + p.E + head * HD, dk, h, 1.0f);
            store_tile_row(p.dqkv + (size_t)(r0 + j) * E3 + 2 * p.E + head * HD, dv, h, 1.0f);
        }
    }
}

// ---- key-tiled ("flash" form): any vertex count ----------------------------------------------------------------------
// A workgroup is (head, sample, group of 4 row blocks).  KT = 128: two tiles are 2 x 128 x 68 floats = 68 KiB, so two
// workgroups share a CU's 160 KiB (one stages while the other computes; the kernels fit 256 registers per lane, the
// two-per-SIMD budget), and a sample of V vertices is ceil(V / 128) workgroups per head instead of one, which is what
// fills the chip at small batch.  Forward: online softmax, the running maximum m, sum l and the output tile o[2] stay
// in registers and are rescaled by exp(m_old - m_new) per tile; dropout multiplies what goes into o, never what goes
// into l, so the result is keep * dscale * softmax as in the resident kernel.  Backward: sweep 1 (dQ) walks K / V tiles,
// sweep 2 (dK, dV) walks tiles of scaled Q and dO with lse and delta_i (recomputed while dO is staged) beside them.
// Every output row is written by one wave in a fixed tile order: no atomics, bit-reproducible.
constexpr int KT = 128;

__global__ __launch_bounds__(256, 2) void attn_fwd_tiled_kernel(const AttnArgs p) {
    const uint32_t seed = p.thresh ? wf3d_seed_load(p.seed) : 0u;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int head = blockIdx.x, s = blockIdx.y, q0 = blockIdx.z * KT;
    const int r0 = p.voff[s], n = p.voff[s + 1] - r0;
    if (n <= 0 || q0 >= n) return;
    const int E3 = 3 * p.E;
    float* Ks = sm;
    float* Vs = sm + KT * LDR;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const bool live = q0 + wave * 32 < n;                  // a wave past the sample's rows only helps staging
    const int i = q0 + wave * 32 + l31;                    // this lane's query
    const bool iok = i < n;
    float qf[32];
    load_half_row(qf, p.qkv + (size_t)(r0 + i) * E3 + head * HD + 32 * h, iok, p.scale);
    float m = -INFINITY, l = 0.f;
    f32x16 o[2];
    zero2(o);
    for (int k0 = 0; k0 < n; k0 += KT) {
        const int tn = min(KT, n - k0), tpad = (tn + 31) & ~31, nt = tpad >> 5;
        if (k0) __syncthreads();
        stage64(Ks, p.qkv, E3, r0 + k0, tn, tpad, p.E + head * HD, 1.0f);
        stage64(Vs, p.qkv, E3, r0 + k0, tn, tpad, 2 * p.E + head * HD, 1.0f);
        __syncthreads();
        if (!live) continue;
        f32x16 st[KT / 32];                                // S^T tiles: rows = keys, column = this lane's query
        float tm = m;
#pragma unroll
        for (int jt = 0; jt < KT / 32; ++jt) {
            if (jt < nt) {
                st[jt] = mm_rows_regs(Ks + (jt * 32 + l31) * LDR + 32 * h, qf);
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    if (k0 + jt * 32 + rowof(e, h) >= n) st[jt][e] = -INFINITY;
                    tm = fmaxf(tm, st[jt][e]);
                }
            }
        }
        tm = fmaxf(tm, __shfl_xor(tm, 32, 64));            // finite from the first tile on: key 0 exists
        const float alpha = expf(m - tm);                  // 0 on the first tile (m = -inf)
        m = tm;
        l *= alpha;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[dt][e] *= alpha;
#pragma unroll
        for (int jt = 0; jt < KT / 32; ++jt) {
            if (jt < nt) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int jl = jt * 32 + rowof(e, h);
                    float pv = expf(st[jt][e] - m);
                    l += pv;
                    if (p.thresh) pv = wf3d_keep(seed, (uint32_t)((r0 + i) * p.heads + head), (uint32_t)(k0 + jl), p.thresh) ? pv * p.dscale : 0.f;
                    const float* vr = Vs + jl * LDR + l31;
                    o[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[0], pv, o[0], 0, 0, 0);
                    o[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[32], pv, o[1], 0, 0, 0);
                }
            }
        }
    }
    l += __shfl_xor(l, 32, 64);
    if (iok) {
        if (h == 0) p.lse[(size_t)(r0 + i) * p.heads + head] = m + logf(l);
        store_tile_row(p.ctx + (size_t)(r0 + i) * p.E + head * HD, o, h, 1.0f / l);
    }
}

// backward sweep 1: a wave owns a query block, K / V are walked in tiles -> dQ.  The dQ step (dq_tile's body) and the
// zero fill are written out: called, they cost 0.1 % at 8 x 513.
__global__ __launch_bounds__(256, 2) void attn_bwd_tiled_dq_kernel(const AttnArgs p) {
    const uint32_t seed = p.thresh ? wf3d_seed_load(p.seed) : 0u;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int head = blockIdx.x, s = blockIdx.y, q0 = blockIdx.z * KT;
    const int r0 = p.voff[s], n = p.voff[s + 1] - r0;
    if (n <= 0 || q0 >= n) return;
    const int E3 = 3 * p.E;
    const float* ctx = p.ctx;
    float* Ks = sm;
    float* Vs = sm + KT * LDR;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const bool live = q0 + wave * 32 < n;
    const int i = q0 + wave * 32 + l31;
    const bool iok = i < n;
    float qf[32], df[32];
    load_half_row(qf, p.qkv + (size_t)(r0 + i) * E3 + head * HD + 32 * h, iok, p.scale);
    load_half_row(df, p.dctx + (size_t)(r0 + i) * p.E + head * HD + 32 * h, iok, 1.0f);
    const float delta = row_delta(ctx + (size_t)(r0 + i) * p.E + head * HD + 32 * h, iok, df);
    const float lse_i = iok ? p.lse[(size_t)(r0 + i) * p.heads + head] : INFINITY;
    f32x16 dq[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) dq[dt][e] = 0.f;
    for (int k0 = 0; k0 < n; k0 += KT) {
        const int tn = min(KT, n - k0), tpad = (tn + 31) & ~31, nt = tpad >> 5;
        if (k0) __syncthreads();
        stage64(Ks, p.qkv, E3, r0 + k0, tn, tpad, p.E + head * HD, 1.0f);
        stage64(Vs, p.qkv, E3, r0 + k0, tn, tpad, 2 * p.E + head * HD, 1.0f);
        __syncthreads();
        if (!live) continue;
        for (int jt = 0; jt < nt; ++jt) {
            const f32x16 st = mm_rows_regs(Ks + (jt * 32 + l31) * LDR + 32 * h, qf);
            const f32x16 dp = mm_rows_regs(Vs + (jt * 32 + l31) * LDR + 32 * h, df);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int jl = jt * 32 + rowof(e, h), j = k0 + jl;
                const float pr = j < n ? expf(st[e] - lse_i) : 0.f;
                float g = dp[e];
                if (p.thresh) g = wf3d_keep(seed, (uint32_t)((r0 + i) * p.heads + head), (uint32_t)j, p.thresh) ? g * p.dscale : 0.f;
                const float ds = pr * (g - delta);
                const float* kr = Ks + jl * LDR + l31;
                dq[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[0], ds, dq[0], 0, 0, 0);
                dq[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[32], ds, dq[1], 0, 0, 0);
            }
        }
    }
    if (iok) store_tile_row(p.dqkv + (size_t)(r0 + i) * E3 + head * HD, dq, h, p.scale);
}

// backward sweep 2: a wave owns a key block, scaled Q / dO (+ lse, delta) are walked in tiles -> dK, dV.  As in the dQ
// kernel the step (dkv_tile's body) and the zero fill are written out: called, they cost 0.1 - 0.15 % at 8 x 513.
__global__ __launch_bounds__(256, 2) void attn_bwd_tiled_dkv_kernel(const AttnArgs p) {
    const uint32_t seed = p.thresh ? wf3d_seed_load(p.seed) : 0u;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int head = blockIdx.x, s = blockIdx.y, j0 = blockIdx.z * KT;
    const int r0 = p.voff[s], n = p.voff[s + 1] - r0;
    if (n <= 0 || j0 >= n) return;
    const int E3 = 3 * p.E;
    const float* ctx = p.ctx;
    float* Qs = sm;                                        // scaled Q tile
    float* Gs = sm + KT * LDR;                             // dO tile
    float* dl = Gs + KT * LDR;                             // [KT] delta_i
    float* ls = dl + KT;                                   // [KT] lse_i (+inf for padded queries)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const bool live = j0 + wave * 32 < n;
    const int j = j0 + wave * 32 + l31;                    // this lane's key
    const bool jok = j < n;
    float kf[32], vf[32];
    load_half_row(kf, p.qkv + (size_t)(r0 + j) * E3 + p.E + head * HD + 32 * h, jok, 1.0f);
    load_half_row(vf, p.qkv + (size_t)(r0 + j) * E3 + 2 * p.E + head * HD + 32 * h, jok, 1.0f);
    f32x16 dk[2], dv[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) { dk[dt][e] = 0.f; dv[dt][e] = 0.f; }
    for (int i0 = 0; i0 < n; i0 += KT) {
        const int tn = min(KT, n - i0), tpad = (tn + 31) & ~31, nt = tpad >> 5;
        if (i0) __syncthreads();
        stage64(Qs, p.qkv, E3, r0 + i0, tn, tpad, head * HD, p.scale);
        // dO rows, and delta_i from the 16 lanes that hold a row (tpad * 16 is a multiple of the block: no lane idles)
        for (int idx = threadIdx.x; idx < tpad * 16; idx += blockDim.x) {
            const int r = idx >> 4, c = (idx & 15) * 4;
            f32x4 g = {0.f, 0.f, 0.f, 0.f};
            float d = 0.f;
            if (r < tn) {
                const size_t at = (size_t)(r0 + i0 + r) * p.E + head * HD + c;
                g = *reinterpret_cast<const f32x4*>(p.dctx + at);
                const f32x4 ov = *reinterpret_cast<const f32x4*>(ctx + at);
                d = g[0] * ov[0] + g[1] * ov[1] + g[2] * ov[2] + g[3] * ov[3];
            }
            *reinterpret_cast<f32x4*>(Gs + r * LDR + c) = g;
#pragma unroll
            for (int x = 8; x > 0; x >>= 1) d += __shfl_xor(d, x, 64);
            if ((idx & 15) == 0) {
                dl[r] = d;
                ls[r] = r < tn ? p.lse[(size_t)(r0 + i0 + r) * p.heads + head] : INFINITY;
            }
        }
        __syncthreads();
        if (!live) continue;
        for (int it = 0; it < nt; ++it) {
            const f32x16 sc = mm_rows_regs(Qs + (it * 32 + l31) * LDR + 32 * h, kf);     // S[i][j], rows = queries
            const f32x16 dp = mm_rows_regs(Gs + (it * 32 + l31) * LDR + 32 * h, vf);     // dP[i][j]
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int il = it * 32 + rowof(e, h);
                const float pr = expf(sc[e] - ls[il]);                                   // 0 for padded queries
                float mk = 1.0f;
                if (p.thresh) mk = wf3d_keep(seed, (uint32_t)((r0 + i0 + il) * p.heads + head), (uint32_t)j, p.thresh) ? p.dscale : 0.f;
                const float ds = pr * (dp[e] * mk - dl[il]);
                const float pt = pr * mk;
                const float* qr = Qs + il * LDR + l31;
                const float* gr = Gs + il * LDR + l31;
                dk[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(qr[0], ds, dk[0], 0, 0, 0);
                dk[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(qr[32], ds, dk[1], 0, 0, 0);
                dv[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(gr[0], pt, dv[0], 0, 0, 0);
                dv[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(gr[32], pt, dv[1], 0, 0, 0);
            }
        }
    }
    if (jok) {
        store_tile_row(p.dqkv + (size_t)(r0 + j) * E3 + p.E + head * HD, dk, h, 1.0f);
        store_tile_row(p.dqkv + (size_t)(r0 + j) * E3 + 2 * p.E + head * HD, dv, h, 1.0f);
    }
}

// ---- key-tiled, head widths 64 < hd <= 128 ----------------------------------------------------------------------------
// The three kernels above on a padded width P = 96 or 128 (the smallest >= hd): a lane half owns P/2 contiguous floats of
// its row, P/32 accumulator tiles replace the two, an LDS row is P + 4 floats (= 4 mod 32 like 68, so the b128 / b32
// patterns stay conflict-free).  Columns hd..P-1 are zeros in LDS and in registers: every global access is one 16-byte
// group of four columns (hd % 4 == 0), and a group at column >= hd is neither read nor written - the next head's
// columns, or the next tensor, sit there.  A workgroup still owns QG = 128 rows (4 waves x 32); the other operand is
// walked in tiles of KTW = KTW_OF<P> rows.  Arithmetic, tile order, dropout counters and the lse / delta handling are
// the width-64 kernels'; a change to a step there goes in here too.  The width-64 kernels are not this template's P = 64
// instantiation: built that way (masks compiled out) it gives the same bits from other instruction streams, 0.8 - 1.2 %
// slower beyond 256 vertices ("Attention at other head widths").
//
// Registers: at P = 128 the dkv kernel holds kf, vf (64 each), dk, dv (4 x 16 each) and two score tiles, more than 256,
// so the wide kernels are __launch_bounds__(256, 1): 512 unified VGPR + AGPR per lane, no scratch (DESIGN.md section 4
// has the compiler's figures); where an instantiation needs no more than 256 of them, two workgroups share a CU.
constexpr int QG = 128;                     // rows per workgroup
// Rows per staged tile of the wide kernels (a multiple of 32, at most QG), chosen per padded width by measurement
// ("Attention at other head widths"):
//   P = 96:  64.  Two tiles are 50 KiB instead of 100, the forward needs 250 registers with two score tiles in place of
//            four (308), the dQ kernel 238: two workgroups of either share a CU.  Forward 30 % and backward 9 - 11 %
//            faster at 256 and 512 vertices than with 128-row tiles, equal at 64 and 128.
//   P = 128: 128.  Two tiles are 132 KiB of the 160 KiB.  Every kernel needs more than 256 registers at either tile
//            size, so a CU holds one workgroup whatever the LDS allows, and 64-row tiles only double the barriers:
//            within 1 % at 256 and 512 vertices, forward behind there.
template <int P> constexpr int KTW_OF = P == 96 ? 64 : 128;

// stage rows [r0, r0+n) x hd columns (col0..) of src[*, ld] into dst[npad][P + 4], zero rows >= n and columns hd..P-1;
// 32 lanes per row, each one 16-byte group (at P = 96 the last 8 of them idle)
template <int P>
__device__ __forceinline__ void stage_wide(float* dst, const float* __restrict__ src, int ld, int r0, int n, int npad,
                                           int col0, int hd, float mul) {
    for (int idx = threadIdx.x; idx < npad * 32; idx += blockDim.x) {
        const int r = idx >> 5, c = (idx & 31) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r < n && c < hd) v = *reinterpret_cast<const f32x4*>(src + (size_t)(r0 + r) * ld + col0 + c) * mul;
        if (c < P) *reinterpret_cast<f32x4*>(dst + r * (P + 4) + c) = v;
    }
}

// this lane's half row (columns c0 .. c0 + P/2 of the head, p pointing at column c0) from global; zero when !ok and from
// column hd on
template <int P>
__device__ __forceinline__ void load_half_row_wide(float (&f)[P / 2], const float* __restrict__ p, int c0, int hd,
                                                   bool ok, float mul) {
#pragma unroll
    for (int k = 0; k < P / 8; ++k) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ok && c0 + 4 * k < hd) v = *reinterpret_cast<const f32x4*>(p + 4 * k);
#pragma unroll
        for (int j = 0; j < 4; ++j) f[4 * k + j] = v[j] * mul;
    }
}

// this lane's row of a [32 rows x P] transposed accumulator set, times mul, to out[0..hd)
template <int P>
__device__ __forceinline__ void store_tile_row_wide(float* out, const f32x16 (&o)[P / 32], int h, int hd, float mul) {
#pragma unroll
    for (int dt = 0; dt < P / 32; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = dt * 32 + 8 * g + 4 * h;
            f32x4 v = {o[dt][4 * g], o[dt][4 * g + 1], o[dt][4 * g + 2], o[dt][4 * g + 3]};
            if (c < hd) *reinterpret_cast<f32x4*>(out + c) = v * mul;
        }
}

// delta_i = dO_i . O_i from this lane's half row of ctx (op, at column c0; zero when !ok and from column hd on) and of
// dO (df), summed over both halves
template <int P>
__device__ __forceinline__ float row_delta_wide(const float* op, int c0, int hd, bool ok, const float (&df)[P / 2]) {
    float delta = 0.f;
#pragma unroll
    for (int k = 0; k < P / 8; ++k) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ok && c0 + 4 * k < hd) v = *reinterpret_cast<const f32x4*>(op + 4 * k);
#pragma unroll
        for (int j = 0; j < 4; ++j) delta += v[j] * df[4 * k + j];
    }
    return delta + __shfl_xor(delta, 32, 64);
}

template <int P>
__global__ __launch_bounds__(256, 1) void attn_fwd_wide_kernel(const AttnArgs p) {
    constexpr int LDW = P + 4, HF = P / 2, NO = P / 32, KTW = KTW_OF<P>;
    const uint32_t seed = p.thresh ? wf3d_seed_load(p.seed) : 0u;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int head = blockIdx.x, s = blockIdx.y, q0 = blockIdx.z * QG;
    const int r0 = p.voff[s], n = p.voff[s + 1] - r0;
    if (n <= 0 || q0 >= n) return;
    const int E3 = 3 * p.E, hd = p.hd;
    float* Ks = sm;
    float* Vs = sm + KTW * LDW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const bool live = q0 + wave * 32 < n;                  // a wave past the sample's rows only helps staging
    const int i = q0 + wave * 32 + l31;                    // this lane's query
    const bool iok = i < n;
    float qf[HF];
    load_half_row_wide<P>(qf, p.qkv + (size_t)(r0 + i) * E3 + head * hd + HF * h, HF * h, hd, iok, p.scale);
    float m = -INFINITY, l = 0.f;
    f32x16 o[NO];
#pragma unroll
    for (int dt = 0; dt < NO; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
    for (int k0 = 0; k0 < n; k0 += KTW) {
        const int tn = min(KTW, n - k0), tpad = (tn + 31) & ~31, nt = tpad >> 5;
        if (k0) __syncthreads();
        stage_wide<P>(Ks, p.qkv, E3, r0 + k0, tn, tpad, p.E + head * hd, hd, 1.0f);
        stage_wide<P>(Vs, p.qkv, E3, r0 + k0, tn, tpad, 2 * p.E + head * hd, hd, 1.0f);
        __syncthreads();
        if (!live) continue;
        f32x16 st[KTW / 32];                               // S^T tiles: rows = keys, column = this lane's query
        float tm = m;
#pragma unroll
        for (int jt = 0; jt < KTW / 32; ++jt) {
            if (jt < nt) {
                st[jt] = mm_rows_regs(Ks + (jt * 32 + l31) * LDW + HF * h, qf);
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    if (k0 + jt * 32 + rowof(e, h) >= n) st[jt][e] = -INFINITY;
                    tm = fmaxf(tm, st[jt][e]);
                }
            }
        }
        tm = fmaxf(tm, __shfl_xor(tm, 32, 64));            // finite from the first tile on: key 0 exists
        const float alpha = expf(m - tm);                  // 0 on the first tile (m = -inf)
        m = tm;
        l *= alpha;
#pragma unroll
        for (int dt = 0; dt < NO; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[dt][e] *= alpha;
#pragma unroll
        for (int jt = 0; jt < KTW / 32; ++jt) {
            if (jt < nt) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int jl = jt * 32 + rowof(e, h);
                    float pv = expf(st[jt][e] - m);
                    l += pv;
                    if (p.thresh) pv = wf3d_keep(seed, (uint32_t)((r0 + i) * p.heads + head), (uint32_t)(k0 + jl), p.thresh) ? pv * p.dscale : 0.f;
                    const float* vr = Vs + jl * LDW + l31;
#pragma unroll
                    for (int dt = 0; dt < NO; ++dt)
                        o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[32 * dt], pv, o[dt], 0, 0, 0);
                }
            }
        }
    }
    l += __shfl_xor(l, 32, 64);
    if (iok) {
        if (h == 0) p.lse[(size_t)(r0 + i) * p.heads + head] = m + logf(l);
        store_tile_row_wide<P>(p.ctx + (size_t)(r0 + i) * p.E + head * hd, o, h, hd, 1.0f / l);
    }
}

// backward sweep 1: a wave owns a query block, K / V are walked in tiles -> dQ
template <int P>
__global__ __launch_bounds__(256, 1) void attn_bwd_wide_dq_kernel(const AttnArgs p) {
    constexpr int LDW = P + 4, HF = P / 2, NO = P / 32, KTW = KTW_OF<P>;
    const uint32_t seed = p.thresh ? wf3d_seed_load(p.seed) : 0u;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int head = blockIdx.x, s = blockIdx.y, q0 = blockIdx.z * QG;
    const int r0 = p.voff[s], n = p.voff[s + 1] - r0;
    if (n <= 0 || q0 >= n) return;
    const int E3 = 3 * p.E, hd = p.hd;
    const float* ctx = p.ctx;
    float* Ks = sm;
    float* Vs = sm + KTW * LDW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const bool live = q0 + wave * 32 < n;
    const int i = q0 + wave * 32 + l31;
    const bool iok = i < n;
    float qf[HF], df[HF];
    load_half_row_wide<P>(qf, p.qkv + (size_t)(r0 + i) * E3 + head * hd + HF * h, HF * h, hd, iok, p.scale);
    load_half_row_wide<P>(df, p.dctx + (size_t)(r0 + i) * p.E + head * hd + HF * h, HF * h, hd, iok, 1.0f);
    const float delta = row_delta_wide<P>(ctx + (size_t)(r0 + i) * p.E + head * hd + HF * h, HF * h, hd, iok, df);
    const float lse_i = iok ? p.lse[(size_t)(r0 + i) * p.heads + head] : INFINITY;
    f32x16 dq[NO];
#pragma unroll
    for (int dt = 0; dt < NO; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) dq[dt][e] = 0.f;
    for (int k0 = 0; k0 < n; k0 += KTW) {
        const int tn = min(KTW, n - k0), tpad = (tn + 31) & ~31, nt = tpad >> 5;
        if (k0) __syncthreads();
        stage_wide<P>(Ks, p.qkv, E3, r0 + k0, tn, tpad, p.E + head * hd, hd, 1.0f);
        stage_wide<P>(Vs, p.qkv, E3, r0 + k0, tn, tpad, 2 * p.E + head * hd, hd, 1.0f);
        __syncthreads();
        if (!live) continue;
        for (int jt = 0; jt < nt; ++jt) {
            const f32x16 st = mm_rows_regs(Ks + (jt * 32 + l31) * LDW + HF * h, qf);
            const f32x16 dp = mm_rows_regs(Vs + (jt * 32 + l31) * LDW + HF * h, df);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int jl = jt * 32 + rowof(e, h), j = k0 + jl;
                const float pr = j < n ? expf(st[e] - lse_i) : 0.f;
                float g = dp[e];
                if (p.thresh) g = wf3d_keep(seed, (uint32_t)((r0 + i) * p.heads + head), (uint32_t)j, p.thresh) ? g * p.dscale : 0.f;
                const float ds = pr * (g - delta);
                const float* kr = Ks + jl * LDW + l31;
#pragma unroll
                for (int dt = 0; dt < NO; ++dt)
                    dq[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[32 * dt], ds, dq[dt], 0, 0, 0);
            }
        }
    }
    if (iok) store_tile_row_wide<P>(p.dqkv + (size_t)(r0 + i) * E3 + head * hd, dq, h, hd, p.scale);
}

// backward sweep 2: a wave owns a key block, scaled Q / dO (+ lse, delta) are walked in tiles -> dK, dV
template <int P>
__global__ __launch_bounds__(256, 1) void attn_bwd_wide_dkv_kernel(const AttnArgs p) {
    constexpr int LDW = P + 4, HF = P / 2, NO = P / 32, KTW = KTW_OF<P>;
    const uint32_t seed = p.thresh ? wf3d_seed_load(p.seed) : 0u;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int head = blockIdx.x, s = blockIdx.y, j0 = blockIdx.z * QG;
    const int r0 = p.voff[s], n = p.voff[s + 1] - r0;
    if (n <= 0 || j0 >= n) return;
    const int E3 = 3 * p.E, hd = p.hd;
    const float* ctx = p.ctx;
    float* Qs = sm;                                        // scaled Q tile
    float* Gs = sm + KTW * LDW;                            // dO tile
    float* dl = Gs + KTW * LDW;                            // [KTW] delta_i
    float* ls = dl + KTW;                                  // [KTW] lse_i (+inf for padded queries)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const bool live = j0 + wave * 32 < n;
    const int j = j0 + wave * 32 + l31;                    // this lane's key
    const bool jok = j < n;
    float kf[HF], vf[HF];
    load_half_row_wide<P>(kf, p.qkv + (size_t)(r0 + j) * E3 + p.E + head * hd + HF * h, HF * h, hd, jok, 1.0f);
    load_half_row_wide<P>(vf, p.qkv + (size_t)(r0 + j) * E3 + 2 * p.E + head * hd + HF * h, HF * h, hd, jok, 1.0f);
    f32x16 dk[NO], dv[NO];
#pragma unroll
    for (int dt = 0; dt < NO; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) { dk[dt][e] = 0.f; dv[dt][e] = 0.f; }
    for (int i0 = 0; i0 < n; i0 += KTW) {
        const int tn = min(KTW, n - i0), tpad = (tn + 31) & ~31, nt = tpad >> 5;
        if (i0) __syncthreads();
        stage_wide<P>(Qs, p.qkv, E3, r0 + i0, tn, tpad, head * hd, hd, p.scale);
        // dO rows, and delta_i from the 32 lanes that hold a row (tpad * 32 is a multiple of the block: no lane idles)
        for (int idx = threadIdx.x; idx < tpad * 32; idx += blockDim.x) {
            const int r = idx >> 5, c = (idx & 31) * 4;
            f32x4 g = {0.f, 0.f, 0.f, 0.f};
            float d = 0.f;
            if (r < tn && c < hd) {
                const size_t at = (size_t)(r0 + i0 + r) * p.E + head * hd + c;
                g = *reinterpret_cast<const f32x4*>(p.dctx + at);
                const f32x4 ov = *reinterpret_cast<const f32x4*>(ctx + at);
                d = g[0] * ov[0] + g[1] * ov[1] + g[2] * ov[2] + g[3] * ov[3];
            }
            if (c < P) *reinterpret_cast<f32x4*>(Gs + r * LDW + c) = g;
#pragma unroll
            for (int x = 16; x > 0; x >>= 1) d += __shfl_xor(d, x, 64);
            if ((idx & 31) == 0) {
                dl[r] = d;
                ls[r] = r < tn ? p.lse[(size_t)(r0 + i0 + r) * p.heads + head] : INFINITY;
            }
        }
        __syncthreads();
        if (!live) continue;
        for (int it = 0; it < nt; ++it) {
            const f32x16 sc = mm_rows_regs(Qs + (it * 32 + l31) * LDW + HF * h, kf);     // S[i][j], rows = queries
            const f32x16 dp = mm_rows_regs(Gs + (it * 32 + l31) * LDW + HF * h, vf);     // dP[i][j]
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int il = it * 32 + rowof(e, h);
                const float pr = expf(sc[e] - ls[il]);                                   // 0 for padded queries
                float mk = 1.0f;
                if (p.thresh) mk = wf3d_keep(seed, (uint32_t)((r0 + i0 + il) * p.heads + head), (uint32_t)j, p.thresh) ? p.dscale : 0.f;
                const float ds = pr * (dp[e] * mk - dl[il]);
                const float pt = pr * mk;
                const float* qr = Qs + il * LDW + l31;
                const float* gr = Gs + il * LDW + l31;
#pragma unroll
                for (int dt = 0; dt < NO; ++dt) {
                    dk[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(qr[32 * dt], ds, dk[dt], 0, 0, 0);
                    dv[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(gr[32 * dt], pt, dv[dt], 0, 0, 0);
                }
            }
        }
    }
    if (jok) {
        store_tile_row_wide<P>(p.dqkv + (size_t)(r0 + j) * E3 + p.E + head * hd, dk, h, hd, 1.0f);
        store_tile_row_wide<P>(p.dqkv + (size_t)(r0 + j) * E3 + 2 * p.E + head * hd, dv, h, hd, 1.0f);
    }
}

// the wide kernels' launches at padded width P: LDS sized from this instantiation's row length and tile rows
template <int P>
int launch_wide(AttnArgs p, const char* who, bool backward, int S, int vmax, hipStream_t stream) {
    constexpr int KTW = KTW_OF<P>;
    static_assert(KTW % 32 == 0 && KTW <= QG, "whole 32-row blocks, and dl / ls hold a tile's rows");
    p.rows = KTW;
    const dim3 grid(p.heads, S, wf3d_cdiv(vmax, QG));
    const size_t tiles = (size_t)2 * KTW * (P + 4) * sizeof(float);
    if (!backward) return wf3d_attn_launch(who, attn_fwd_wide_kernel<P>, grid, tiles, p, stream);
    int rc = wf3d_attn_launch(who, attn_bwd_wide_dq_kernel<P>, grid, tiles, p, stream);
    if (rc) return rc;
    return wf3d_attn_launch(who, attn_bwd_wide_dkv_kernel<P>, grid, tiles + 2 * KTW * sizeof(float), p, stream);
}

}  // namespace

int wf3d_attn_mfma_launch(AttnArgs p, int family, bool backward, int S, int vmax, hipStream_t stream) {
    const char* who = backward ? "wf3d_attn_bwd" : "wf3d_attn_fwd";
    WF3D_CHECK(p.hd == HD || (family == 2 && p.hd > HD && p.hd <= 128 && p.hd % 4 == 0), WF3D_ERR_UNSUPPORTED,
               "%s: no MFMA kernel for head_dim %d in family %d", who, p.hd, family);
    if (family == 1) {                                     // resident: K / V (or Q / dO) of the padded sample, + lse, delta
        p.rows = (vmax + 31) & ~31;
        const dim3 grid(p.heads, S);
        const size_t rows = (size_t)2 * p.rows * LDR * sizeof(float);
        if (!backward) return wf3d_attn_launch(who, attn_fwd_mfma_kernel, grid, rows, p, stream);
        return wf3d_attn_launch(who, attn_bwd_mfma_kernel, grid, rows + 2 * p.rows * sizeof(float), p, stream);
    }
    static_assert(QG == KT, "a workgroup owns 128 rows at every width: one grid rule");
    WF3D_CHECK(wf3d_cdiv(vmax, KT) <= 65535, WF3D_ERR_UNSUPPORTED, "%s: vmax %d too large", who, vmax);
    if (p.hd != HD) {                                      // 64 < hd <= 128 (attn_family): the smallest padded width
        return p.hd <= 96 ? launch_wide<96>(p, who, backward, S, vmax, stream)
                          : launch_wide<128>(p, who, backward, S, vmax, stream);
    }
    p.rows = KT;
    const dim3 grid(p.heads, S, wf3d_cdiv(vmax, KT));
    const size_t tiles = (size_t)2 * KT * LDR * sizeof(float);
    if (!backward) return wf3d_attn_launch(who, attn_fwd_tiled_kernel, grid, tiles, p, stream);
    int rc = wf3d_attn_launch(who, attn_bwd_tiled_dq_kernel, grid, tiles, p, stream);
    if (rc) return rc;
    return wf3d_attn_launch(who, attn_bwd_tiled_dkv_kernel, grid, tiles + 2 * KT * sizeof(float), p, stream);
}
