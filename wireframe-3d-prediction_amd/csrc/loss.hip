// Row f-1: the device side of losses/WireframeLoss.py — the caller of backward.
//
// The reference builds one [V, V] Hungarian cost matrix per sample with torch ops and a
// `.cpu().numpy()` sync PER SAMPLE (WireframeLoss.py:130-236), then evaluates SmoothL1 / BCE with
// a dozen more launches.  Here: one kernel writes all B cost matrices (one device->host copy for
// the whole batch; the assignment itself stays scipy on the host, as in the reference), and one
// kernel evaluates the three loss terms AND their gradients w.r.t. the model outputs — which are
// exactly the cotangents entering the hot path's backward.
#include <cfloat>

#include "lsa_solve.h"
#include "wf3d_common.h"

namespace {

// cost[b,p,t] = sum_k |v[b,p,k] - tv[b,t,k]| + |e[b,p] - 1|   for t < count[b]   (real targets)
//             = e[b,p]                                         for t >= count[b]  (dummy columns)
__global__ __launch_bounds__(256) void loss_cost_kernel(const float* __restrict__ verts, long vs_b, long vs_v,
                                                         const float* __restrict__ exist,
                                                         const float* __restrict__ tverts, int Vt,
                                                         const int64_t* __restrict__ counts, int V,
                                                         float* __restrict__ cost) {
    const int b = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= V * V) return;
    const int p = idx / V, t = idx % V;
    const int cnt = (int)counts[b];
    const float e = exist[(size_t)b * V + p];
    float c = e;
    if (t < cnt) {
        const float* v = verts + (size_t)b * vs_b + (size_t)p * vs_v;
        const float* w = tverts + ((size_t)b * Vt + t) * 3;
        c = (fabsf(v[0] - w[0]) + fabsf(v[1] - w[1]) + fabsf(v[2] - w[2])) + fabsf(e - 1.0f);
    }
    cost[(size_t)b * V * V + idx] = c;
}

__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wf3d_wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// nn.BCELoss element: -(t*max(log p, -100) + (1-t)*max(log(1-p), -100)); grad (p-t)/max(p(1-p), 1e-12)
__device__ __forceinline__ float bce(float p, float t, float& g) {
    g = (p - t) / fmaxf(p * (1.0f - p), 1e-12f);
    return -(t * fmaxf(logf(p), -100.0f) + (1.0f - t) * fmaxf(log1pf(-p), -100.0f));
}

// One side of the class-balanced edge element: v = x^gamma * max(log y, -100) with x = 1 - y (ly = log y as formed by the
// caller), and dv/dy in dy.  x^(gamma - 1) is formed as x^gamma / x; at x = 0 that factor meets ly = log 1 = 0 and the
// product's limit is 0, which is what is returned there instead of inf * 0.
__device__ __forceinline__ float focal_side(float y, float x, float ly, float gamma, float& dy) {
    const float xg = gamma > 0.f ? powf(x, gamma) : 1.0f;
    const float l = fmaxf(ly, -100.0f);
    dy = (ly > -100.0f ? xg / y : 0.f) - (gamma > 0.f && x > 0.f ? gamma * (xg / x) * l : 0.f);
    return xg * l;
}

// The balanced / focal edge element (WireframeLoss(edge_pos_weight = w, edge_focal_gamma = gamma)):
//   L = -(w t (1-p)^gamma max(log p, -100) + (1-t) p^gamma max(log1p(-p), -100)),  g = dL/dp of that expression
// (the clamps have derivative 0 where they bind).  A side whose coefficient t or 1-t is exactly 0 is not evaluated, and a
// probability that equals a hard label exactly (p = t = 0 or 1: the padded columns of a ragged batch) gives 0 and
// gradient 0 at every gamma, as bce() does there.
__device__ __forceinline__ float bce_bal(float p, float t, float w, float gamma, float& g) {
    g = 0.f;
    if (p == t && (t == 0.f || t == 1.f)) return 0.f;
    float s = 0.f, d;
    if (t != 0.f) {
        s = w * t * focal_side(p, 1.0f - p, logf(p), gamma, d);
        g = w * t * d;
    }
    if (t != 1.0f) {
        s += (1.0f - t) * focal_side(1.0f - p, p, log1pf(-p), gamma, d);
        g -= (1.0f - t) * d;                   // d/dp of a function of y = 1 - p
    }
    g = -g;
    return -s;
}

// One workgroup per sample: partial sums of the three terms + all gradients.  The forms differ in the vertex term only:
//   ASSIGNED = false  matches from host lists (the scipy path): m_a = m_pred, with m_tgt and m_off; gv = weight / normaliser
//   ASSIGNED = true   the device assignment m_a = col4row: prediction p of sample b is matched iff col4row[b,p] < counts[b];
//                     gv arrives as the vertex weight and is normalised here by the matches the counts add up to
// The edge term runs over the common width min_e with the gradient scale gd (weight / normaliser, like ge); ewidth
// non-NULL: the prediction width comes from the device, and min_e and gd are formed here from it and the edge weight we.
// BAL: the edge element is bce_bal(pos_w, gamma) instead of bce(); the two arguments are not read otherwise.
template <bool ASSIGNED, bool BAL = false>
__global__ __launch_bounds__(256) void loss_terms_kernel(const float* __restrict__ verts, long vs_b, long vs_v,
                                                          const float* __restrict__ exist,
                                                          const float* __restrict__ edge, int Ep,
                                                          const float* __restrict__ tverts, int Vt,
                                                          const float* __restrict__ texist,
                                                          const float* __restrict__ tlabel, int Et, int min_e,
                                                          const int32_t* __restrict__ m_a,
                                                          const int32_t* __restrict__ m_tgt,
                                                          const int32_t* __restrict__ m_off,
                                                          const int64_t* __restrict__ counts, int V, int B,
                                                          float gv, float ge, float gd,
                                                          float* __restrict__ dverts, float* __restrict__ dexist,
                                                          float* __restrict__ dedge, float* __restrict__ part,
                                                          const int64_t* __restrict__ ewidth, float we, float pos_w,
                                                          float gamma) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (ewidth) {
        min_e = edge_common_width(*ewidth, Ep, Et);
        gd = min_e ? we / ((float)B * min_e) : 0.f;
    }
    // vertex term: SmoothL1 (beta = 1) over the Hungarian-matched pairs
    float sv = 0.f;
    if (ASSIGNED) {
        long nm = 0;
        for (int s = 0; s < B; ++s) nm += min((long)counts[s], (long)V);        // total matches = sum of real targets
        gv = nm > 0 ? gv / (3.0f * (float)nm) : 0.f;
        const int cnt = (int)counts[b];
        for (int p = tid; p < V; p += 256) {
            const int t = m_a[(size_t)b * V + p];
            const bool m = t < cnt;
            const float* vp = verts + (size_t)b * vs_b + (size_t)p * vs_v;
            const float* w = tverts + ((size_t)b * Vt + (m ? t : 0)) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float g = 0.f;
                if (m) {
                    const float d = vp[k] - w[k], a = fabsf(d);
                    sv += a < 1.0f ? 0.5f * d * d : a - 0.5f;
                    g = gv * (a < 1.0f ? d : (d > 0.f ? 1.0f : -1.0f));
                }
                dverts[((size_t)b * V + p) * 3 + k] = g;
            }
        }
    } else {
        for (int i = tid; i < V * 3; i += 256) dverts[(size_t)b * V * 3 + i] = 0.f;
        __syncthreads();
        for (int m = m_off[b] + tid; m < m_off[b + 1]; m += 256) {
            const int p = m_a[m], t = m_tgt[m];
            const float* v = verts + (size_t)b * vs_b + (size_t)p * vs_v;
            const float* w = tverts + ((size_t)b * Vt + t) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float d = v[k] - w[k], a = fabsf(d);
                sv += a < 1.0f ? 0.5f * d * d : a - 0.5f;
                dverts[((size_t)b * V + p) * 3 + k] = gv * (a < 1.0f ? d : (d > 0.f ? 1.0f : -1.0f));   // p unique per match
            }
        }
    }
    // existence term
    float se = 0.f;
    for (int i = tid; i < V; i += 256) {
        float g;
        se += bce(exist[(size_t)b * V + i], texist[(size_t)b * V + i], g);
        dexist[(size_t)b * V + i] = ge * g;
    }
    // edge term over the common width
    float sd = 0.f;
    for (int i = tid; i < Ep; i += 256) {
        float g = 0.f;
        if (i < min_e) {
            const float p = edge[(size_t)b * Ep + i], t = tlabel[(size_t)b * Et + i];
            sd += BAL ? bce_bal(p, t, pos_w, gamma, g) : bce(p, t, g);
        }
        dedge[(size_t)b * Ep + i] = gd * g;
    }
    sv = block_sum(sv, red); se = block_sum(se, red); sd = block_sum(sd, red);
    if (tid == 0) { part[b * 3] = sv; part[b * 3 + 1] = se; part[b * 3 + 2] = sd; }
}

// COUNTS (the device assignment): the match count, so the vertex normaliser nv, is formed here from counts (a template
// argument: the one thread's loop waits for no second load where there are no counts); ewidth non-NULL: so is the edge
// normaliser nd
template <bool COUNTS>
__global__ void loss_final_kernel(const float* __restrict__ part, const int64_t* __restrict__ counts, int B, int V, float nv,
                                  float ne, float nd, float wv, float we, float wd, float* __restrict__ out,
                                  const int64_t* __restrict__ ewidth, int Ep, int Et) {
    if (ewidth) nd = (float)B * edge_common_width(*ewidth, Ep, Et);
    float sv = 0.f, se = 0.f, sd = 0.f;
    long nm = 0;
    for (int b = 0; b < B; ++b) {
        sv += part[b * 3]; se += part[b * 3 + 1]; sd += part[b * 3 + 2];
        if (COUNTS) nm += min((long)counts[b], (long)V);
    }
    if (COUNTS) nv = 3.0f * (float)nm;
    const float lv = nv > 0.f ? sv / nv : 0.f, le = ne > 0.f ? se / ne : 0.f, ld = nd > 0.f ? sd / nd : 0.f;
    out[0] = lv; out[1] = le; out[2] = ld; out[3] = wv * lv + we * le + wd * ld;
}


// ---------------------------------------------------------------------------
// Linear sum assignment on the device: shortest-augmenting-path (Jonker-Volgenant, the
// algorithm behind scipy.optimize.linear_sum_assignment) on a square [V, V] cost matrix, one
// wave64 per sample, lanes = columns (V <= 256: up to 4 columns per lane), dual variables and
// path costs in fp64 like scipy.  Removes the loss's only device->host sync: with it the
// whole train step is asynchronous.  Output col4row[b, p] = column assigned to prediction p.
// Ties: a lane-order rule (unassigned column first, then lowest index); the dummy columns of
// the wireframe cost are identical, so only assignments to real targets are meaningful and
// those are unique whenever the optimum is.  tests/lsa_model.py states algorithm and tie rule in numpy; the kernels'
// col4row equals it element for element (only additions and subtractions here: nothing contracts to an FMA).
//
// Non-finite costs.  All three kernels read the cost matrix clamped: NaN and +inf become FLT_MAX, -inf becomes
// -FLT_MAX, a finite value is unchanged (lsa_cost here, lsa_cost64 in lsa_solve.h: the same function of a float).  That
// is what makes them terminate on any input; lsa_solve.h gives the argument.  The result is always a permutation; a NaN
// in the model outputs then reaches the loss through the term kernels, as it would in torch.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float lsa_cost(float c) {
    return c < FLT_MAX ? (c > -FLT_MAX ? c : -FLT_MAX) : FLT_MAX;       // NaN fails the first comparison
}

// V > 64: the solver of lsa_solve.h on the square problem, state in LDS.  wf3d_loss_assign has no status output: the
// solver's is dropped, and its guards are compiled out (lsa_solve.h says what they cost here).
__global__ __launch_bounds__(64) void lsa_kernel(const float* __restrict__ cost, int V, int32_t* __restrict__ col4row_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    const int b = blockIdx.x;
    lsa_rect_solve<float, true, false>(lsm, nullptr, cost + (size_t)b * V * V, V, V, V, 1, col4row_out + (size_t)b * V);
}

// V <= 64: the whole solver state lives in registers — lane j owns column j (v_j, shortest-path cost, predecessor,
// row4col_j, visited flag) and row j (u_j, col4row_j); a uniform row/column index is read with v_readlane, the
// arg-min is one fp64 wave minimum plus two ballots, and the cost matrix sits in LDS (<= 16 KB) instead of being
// re-read from L2 once per path step.  Same algorithm, same tie rule as lsa_kernel.
__device__ __forceinline__ double lane_read_f64(double x, int lane_uniform) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)b, lane_uniform);
    const unsigned hi = __builtin_amdgcn_readlane((unsigned)(b >> 32), lane_uniform);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// RECT (counts given): the wireframe cost has V - count identical dummy columns (cost e_p for prediction p), so the
// square problem equals the rectangular one "assign each of the count real targets to a distinct prediction, cost
// c[p,t] - e_p" (+ a constant): rows = targets, lane = prediction, only `count` augmentations instead of V (the
// dataset's counts are 4..38 of 64).  Unmatched predictions get the dummy columns count, count+1, ... in lane order.
// counts[b] is clamped to 0..V: a negative count is 0 (nothing matched), one above V is V.
template <bool RECT>
__global__ __launch_bounds__(64) void lsa64_kernel(const float* __restrict__ cost, const int64_t* __restrict__ counts, int V,
                                                    int32_t* __restrict__ col4row_out) {
    __shared__ float Cs[64 * 64];
    const int lane = threadIdx.x, b = blockIdx.x;
    const float* C = cost + (size_t)b * V * V;
    const int nrow = RECT ? (int)min(max(counts[b], (int64_t)0), (int64_t)V) : V;
    const bool col_ok = lane < V;
    double ep = 0.0;
    if (RECT) {
        for (int idx = lane; idx < nrow * V; idx += 64) Cs[idx] = lsa_cost(C[(size_t)(idx % V) * V + idx / V]);      // Cs[t][p] = cost[p][t]
        if (col_ok && nrow < V) ep = (double)lsa_cost(C[(size_t)lane * V + V - 1]);
    } else {
        for (int idx = lane; idx < V * V; idx += 64) Cs[idx] = lsa_cost(C[idx]);
    }
    __syncthreads();
    double u = 0.0, v = 0.0;
    int row4col = -1, col4row = -1;
    for (int cur = 0; cur < nrow; ++cur) {
        double spc = INFINITY;
        bool in_sc = !col_ok;
        int path = -1;
        int i = cur, sink = -1;
        double min_val = 0.0;
        unsigned long long sr_mask = 0ull;
        while (sink < 0) {
            sr_mask |= 1ull << i;
            const double ui = lane_read_f64(u, i);
            if (!in_sc) {
                const double r = min_val + ((double)Cs[i * V + lane] - ep) - ui - v;
                if (r < spc) { spc = r; path = i; }
            }
            double m = in_sc ? INFINITY : spc;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmin(m, __shfl_xor(m, o, 64));
            const unsigned long long cand = __ballot(!in_sc && spc == m);
            const unsigned long long fr = cand & __ballot(row4col < 0);
            const int pick = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(fr ? fr : cand));
            min_val = m;
            if (lane == pick) in_sc = true;
            const int r4c = __builtin_amdgcn_readlane(row4col, pick);
            if (r4c < 0) sink = pick; else i = __builtin_amdgcn_readfirstlane(r4c);
        }
        // dual update: rows in SR (lane = row), columns in SC (lane = column)
        {
            const int c = col4row < 0 ? 0 : col4row;
            const double spc_c = __shfl(spc, c, 64);
            if ((sr_mask >> lane) & 1ull) u += (lane == cur) ? min_val : min_val - spc_c;
            if (in_sc && col_ok) v -= min_val - spc;
        }
        // augment along the path (wave-uniform walk)
        int j = sink;
        while (true) {
            const int r = __builtin_amdgcn_readlane(path, j);
            if (lane == j) row4col = r;
            const int prev = __builtin_amdgcn_readlane(col4row, r);
            if (lane == r) col4row = j;
            if (r == cur) break;
            j = __builtin_amdgcn_readfirstlane(prev);
        }
    }
    if (RECT) {
        // lane = prediction: its target, or the next free dummy column
        const unsigned long long un = __ballot(col_ok && row4col < 0);
        const int rank = __builtin_popcountll(un & ((1ull << lane) - 1ull));
        if (col_ok) col4row_out[(size_t)b * V + lane] = row4col >= 0 ? row4col : nrow + rank;
    } else if (col_ok) {
        col4row_out[(size_t)b * V + lane] = col4row;
    }
}

}  // namespace

extern "C" int wf3d_loss_cost_matrix(const float* verts, long sample_stride, long vertex_stride, const float* exist,
                                     const float* tverts, int Vt, const int64_t* counts, int B, int V, float* cost,
                                     void* stream) {
    WF3D_CHECK(B >= 0 && V > 0 && Vt > 0, WF3D_ERR_ARG, "wf3d_loss_cost_matrix: bad dims");
    if (B == 0) return WF3D_OK;
    WF3D_CHECK(verts && exist && tverts && counts && cost, WF3D_ERR_ARG, "wf3d_loss_cost_matrix: null pointer");
    WF3D_CHECK(B <= 65535, WF3D_ERR_UNSUPPORTED, "wf3d_loss_cost_matrix: B > 65535");
    hipLaunchKernelGGL(loss_cost_kernel, dim3(wf3d_cdiv((long)V * V, 256), B), dim3(256), 0, (hipStream_t)stream, verts,
                       sample_stride, vertex_stride, exist, tverts, Vt, counts, V, cost);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

namespace {
// where a term launch takes its matches from: host lists (the scipy path), or a device assignment (counts non-NULL),
// which may come with a device edge width
struct LossMatch {
    const int32_t *m_pred, *m_tgt, *m_off;
    int n_match;
    const int32_t* col4row;
    const int64_t *counts, *ewidth;
    float pos_w = 1.0f, gamma = 0.0f;      // the edge element: (1, 0) is bce(), anything else bce_bal() (device assignment only)
};
}  // namespace

// The shared checks and the two launches of the three term entry points.  own_ptrs: the entry's own pointers are there.
static int loss_terms_run(const char* fn, const LossMatch& ms, bool own_ptrs, const float* verts, long sample_stride,
                          long vertex_stride, const float* exist, const float* edge, int Ep, const float* tverts, int Vt,
                          const float* texist, const float* tlabel, int Et, int B, int V, float w_vertex, float w_exist,
                          float w_edge, float* dverts, float* dexist, float* dedge, float* losses, void* ws, size_t ws_bytes,
                          void* stream) {
    WF3D_CHECK(B > 0 && V > 0 && Ep >= 0 && Et >= 0, WF3D_ERR_ARG, "%s: bad dims", fn);
    WF3D_CHECK(own_ptrs && verts && exist && tverts && texist && dverts && dexist && losses, WF3D_ERR_ARG, "%s: null pointer", fn);
    WF3D_CHECK(Ep == 0 || (edge && dedge), WF3D_ERR_ARG, "%s: null edge tensors", fn);
    WF3D_CHECK(ws && ws_bytes >= (size_t)B * 3 * sizeof(float), WF3D_ERR_WS, "%s: workspace too small", fn);
    // with a device edge width the common width, its gradient scale and its normaliser are formed on the device
    const int min_e = (!ms.ewidth && Ep > 0 && Et > 0 && tlabel) ? (Ep < Et ? Ep : Et) : 0;
    const float nv = 3.0f * (float)ms.n_match, ne = (float)B * V, nd = (float)B * min_e;
    // the vertex gradient scale: the lists' is formed here, the assignment's on the device from the weight
    const float gv = ms.counts ? w_vertex : (ms.n_match ? w_vertex / nv : 0.f);
    hipStream_t st = (hipStream_t)stream;
    const bool bal = ms.pos_w != 1.0f || ms.gamma != 0.0f;
    auto terms = bal ? &loss_terms_kernel<true, true> : ms.counts ? &loss_terms_kernel<true> : &loss_terms_kernel<false>;
    hipLaunchKernelGGL(terms, dim3(B), dim3(256), 0, st, verts, sample_stride, vertex_stride, exist, edge, Ep, tverts, Vt,
                       texist, tlabel, Et, min_e, ms.counts ? ms.col4row : ms.m_pred, ms.m_tgt, ms.m_off, ms.counts, V, B, gv,
                       w_exist / ne, min_e ? w_edge / nd : 0.f, dverts, dexist, dedge, (float*)ws, ms.ewidth, w_edge,
                       ms.pos_w, ms.gamma);
    WF3D_LAUNCH_CHECK();
    auto fin = ms.counts ? &loss_final_kernel<true> : &loss_final_kernel<false>;
    hipLaunchKernelGGL(fin, dim3(1), dim3(1), 0, st, (const float*)ws, ms.counts, B, V, nv, ne, nd, w_vertex,
                       w_exist, w_edge, losses, ms.ewidth, Ep, Et);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" int wf3d_loss_terms(const float* verts, long sample_stride, long vertex_stride, const float* exist,
                               const float* edge, int Ep, const float* tverts, int Vt, const float* texist,
                               const float* tlabel, int Et, const int32_t* m_pred, const int32_t* m_tgt,
                               const int32_t* m_off, int n_match, int B, int V, float w_vertex, float w_exist,
                               float w_edge, float* dverts, float* dexist, float* dedge, float* losses, void* ws,
                               size_t ws_bytes, void* stream) {
    WF3D_CHECK(n_match >= 0, WF3D_ERR_ARG, "wf3d_loss_terms: bad dims");
    return loss_terms_run("wf3d_loss_terms", LossMatch{m_pred, m_tgt, m_off, n_match, nullptr, nullptr, nullptr}, m_off != nullptr,
                          verts, sample_stride, vertex_stride, exist, edge, Ep, tverts, Vt, texist, tlabel, Et, B, V, w_vertex,
                          w_exist, w_edge, dverts, dexist, dedge, losses, ws, ws_bytes, stream);
}

extern "C" int wf3d_loss_terms_assigned(const float* verts, long sample_stride, long vertex_stride, const float* exist,
                                        const float* edge, int Ep, const float* tverts, int Vt, const float* texist,
                                        const float* tlabel, int Et, const int32_t* col4row, const int64_t* counts,
                                        int B, int V, float w_vertex, float w_exist, float w_edge, float* dverts,
                                        float* dexist, float* dedge, float* losses, void* ws, size_t ws_bytes,
                                        void* stream) {
    return loss_terms_run("wf3d_loss_terms_assigned", LossMatch{nullptr, nullptr, nullptr, 0, col4row, counts, nullptr},
                          col4row && counts, verts, sample_stride, vertex_stride, exist, edge, Ep, tverts, Vt, texist, tlabel, Et,
                          B, V, w_vertex, w_exist, w_edge, dverts, dexist, dedge, losses, ws, ws_bytes, stream);
}

extern "C" int wf3d_loss_terms_assigned_ew(const float* verts, long sample_stride, long vertex_stride, const float* exist,
                                           const float* edge, int Ep, const float* tverts, int Vt, const float* texist,
                                           const float* tlabel, int Et, const int64_t* edge_width, const int32_t* col4row,
                                           const int64_t* counts, int B, int V, float w_vertex, float w_exist, float w_edge,
                                           float* dverts, float* dexist, float* dedge, float* losses, void* ws,
                                           size_t ws_bytes, void* stream) {
    // the other entries read a null tlabel as width 0; here the width is the device's to say
    WF3D_CHECK(Et <= 0 || tlabel, WF3D_ERR_ARG, "wf3d_loss_terms_assigned_ew: null edge labels");
    return loss_terms_run("wf3d_loss_terms_assigned_ew", LossMatch{nullptr, nullptr, nullptr, 0, col4row, counts, edge_width},
                          col4row && counts && edge_width, verts, sample_stride, vertex_stride, exist, edge, Ep, tverts, Vt, texist,
                          tlabel, Et, B, V, w_vertex, w_exist, w_edge, dverts, dexist, dedge, losses, ws, ws_bytes, stream);
}

extern "C" int wf3d_loss_terms_assigned_bal(const float* verts, long sample_stride, long vertex_stride, const float* exist,
                                            const float* edge, int Ep, const float* tverts, int Vt, const float* texist,
                                            const float* tlabel, int Et, const int64_t* edge_width, const int32_t* col4row,
                                            const int64_t* counts, int B, int V, float w_vertex, float w_exist, float w_edge,
                                            float edge_pos_weight, float edge_focal_gamma, float* dverts, float* dexist,
                                            float* dedge, float* losses, void* ws, size_t ws_bytes, void* stream) {
    // negated comparisons: NaN is refused too
    WF3D_CHECK(edge_pos_weight > 0.f && edge_pos_weight <= FLT_MAX && edge_focal_gamma >= 0.f && edge_focal_gamma <= FLT_MAX,
               WF3D_ERR_ARG, "wf3d_loss_terms_assigned_bal: edge_pos_weight must be a finite number > 0 and edge_focal_gamma one >= 0");
    WF3D_CHECK(!edge_width || Et <= 0 || tlabel, WF3D_ERR_ARG, "wf3d_loss_terms_assigned_bal: null edge labels");
    return loss_terms_run("wf3d_loss_terms_assigned_bal",
                          LossMatch{nullptr, nullptr, nullptr, 0, col4row, counts, edge_width, edge_pos_weight, edge_focal_gamma},
                          col4row && counts, verts, sample_stride, vertex_stride, exist, edge, Ep, tverts, Vt, texist, tlabel, Et,
                          B, V, w_vertex, w_exist, w_edge, dverts, dexist, dedge, losses, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------------------
// Matched edge labels (WireframeLoss(edge_targets="matched")).  Column k of a prediction row is the pair (p, q) of
// predicted SLOTS; the labels arrive per pair (i, j) of ground-truth vertices.  out[b, k] = the label of the pair of
// targets that slots p and q are matched to, 0 where either is unmatched; wf3d.targets.matched_edge_labels states it in
// numpy and the kernel equals it element for element.  Grid (column chunks, B): a sample's row is cut into chunks of
// ELM_COLS columns, each workgroup stages the sample's assignment row in LDS (<= 4 KiB) and writes its chunk once.
// ---------------------------------------------------------------------------
namespace {
constexpr int ELM_COLS = 512;      // columns per workgroup, two per thread

// pair k of the pairs i < j < d in lexicographic order, 0 <= k < d(d-1)/2, d <= 1024: (2d-1)^2 - 8k is an integer in
// 1 .. 2^24, so its fp32 square root is off by less than one unit and one integer step either way mends the estimate
__device__ __forceinline__ void pair_unrank(int k, int d, int& p, int& q) {
    const int b = 2 * d - 1;
    int i = (int)(((float)b - sqrtf((float)(b * b - 8 * k))) * 0.5f);
    i = max(0, min(i, d - 2));
    if (edge_offset(i + 1, d) <= k) ++i;
    else if (edge_offset(i, d) > k) --i;
    p = i;
    q = k - edge_offset(i, d) + i + 1;
}

__global__ __launch_bounds__(256) void edge_labels_matched_kernel(const float* __restrict__ tlabel, int Et,
                                                                   const int32_t* __restrict__ col4row,
                                                                   const int64_t* __restrict__ counts,
                                                                   const int64_t* __restrict__ pair_counts, int V, int Ep,
                                                                   float* __restrict__ out) {
    __shared__ int32_t tgt[1024];      // slot -> matched target, -1 for none
    const int b = blockIdx.y, tid = threadIdx.x;
    const int c = (int)min(max(counts[b], (int64_t)0), (int64_t)V);
    const int d = pair_counts ? (int)min(max(pair_counts[b], (int64_t)0), (int64_t)V) : c;
    for (int p = tid; p < d; p += 256) {
        const int t = col4row[(size_t)b * V + p];
        tgt[p] = t >= 0 && t < c ? t : -1;
    }
    __syncthreads();
    const int npair = d * (d - 1) / 2;
    const float* tl = tlabel + (size_t)b * Et;
    const long k0 = (long)blockIdx.x * ELM_COLS;
#pragma unroll
    for (int it = 0; it < ELM_COLS / 256; ++it) {
        const long k = k0 + it * 256 + tid;
        if (k >= Ep) break;
        float v = 0.f;
        if (k < npair) {
            int p, q;
            pair_unrank((int)k, d, p, q);
            const int tp = tgt[p], tq = tgt[q];
            if (tp >= 0 && tq >= 0 && tp != tq) {
                const int lo = min(tp, tq), hi = max(tp, tq);
                const int idx = edge_offset(lo, c) + (hi - lo - 1);
                if (idx < Et) v = tl[idx];
            }
        }
        out[(size_t)b * Ep + k] = v;
    }
}
}  // namespace

extern "C" int wf3d_edge_labels_matched(const float* tlabel, int Et, const int32_t* col4row, const int64_t* counts,
                                        const int64_t* pair_counts, int B, int V, int Ep, float* out, void* stream) {
    WF3D_CHECK(B >= 0 && V > 0 && Ep >= 0 && Et >= 0, WF3D_ERR_ARG,
               "wf3d_edge_labels_matched: bad dims (B %d, V %d, Ep %d, Et %d)", B, V, Ep, Et);
    WF3D_CHECK(V <= 1024, WF3D_ERR_UNSUPPORTED, "wf3d_edge_labels_matched: V > 1024 (got %d)", V);
    WF3D_CHECK(B <= 65535, WF3D_ERR_UNSUPPORTED, "wf3d_edge_labels_matched: B > 65535 (got %d)", B);
    WF3D_CHECK((long)B * Ep < (1L << 31) && (long)B * Et < (1L << 31), WF3D_ERR_UNSUPPORTED,
               "wf3d_edge_labels_matched: B * Ep or B * Et >= 2^31 (B %d, Ep %d, Et %d)", B, Ep, Et);
    if (B == 0 || Ep == 0) return WF3D_OK;
    WF3D_CHECK(col4row && counts && out && (Et == 0 || tlabel), WF3D_ERR_ARG, "wf3d_edge_labels_matched: null pointer");
    hipLaunchKernelGGL(edge_labels_matched_kernel, dim3(wf3d_cdiv(Ep, ELM_COLS), B), dim3(256), 0, (hipStream_t)stream, tlabel,
                       Et, col4row, counts, pair_counts, V, Ep, out);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" int wf3d_loss_assign(const float* cost, int B, int V, int32_t* col4row, void* stream) {
    WF3D_CHECK(B >= 0 && V > 0, WF3D_ERR_ARG, "wf3d_loss_assign: bad dims");
    WF3D_CHECK(V <= 1024, WF3D_ERR_UNSUPPORTED, "wf3d_loss_assign: V > 1024");
    if (B == 0) return WF3D_OK;
    WF3D_CHECK(cost && col4row, WF3D_ERR_ARG, "wf3d_loss_assign: null pointer");
    if (V <= 64) {
        hipLaunchKernelGGL(lsa64_kernel<false>, dim3(B), dim3(64), 0, (hipStream_t)stream, cost, (const int64_t*)nullptr, V, col4row);
    } else {
        hipLaunchKernelGGL(lsa_kernel, dim3(B), dim3(64), lsa_state_bytes(V), (hipStream_t)stream, cost, V, col4row);
    }
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" int wf3d_loss_assign_counts(const float* cost, const int64_t* counts, int B, int V, int32_t* col4row, void* stream) {
    WF3D_CHECK(B >= 0 && V > 0, WF3D_ERR_ARG, "wf3d_loss_assign_counts: bad dims");
    if (B == 0) return WF3D_OK;
    WF3D_CHECK(cost && counts && col4row, WF3D_ERR_ARG, "wf3d_loss_assign_counts: null pointer");
    if (V > 64) return wf3d_loss_assign(cost, B, V, col4row, stream);       // general kernel: square problem
    hipLaunchKernelGGL(lsa64_kernel<true>, dim3(B), dim3(64), 0, (hipStream_t)stream, cost, counts, V, col4row);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

// ---------------------------------------------------------------------------
// Training-step meter (train.py:145-157): the reference reads total_loss.item() twice and copies sample 0's vertices to
// the host EVERY step to track loss history, best loss and a monitoring RMSE.  Here one small launch per step folds
// those into a device-resident record that the loop reads back whenever it logs (one copy per k steps, no per-step sync).
//   state[0] = steps recorded, [1] = best total loss, [2] = best vertex RMSE, [3..7] = last total / vertex / existence /
//   edge loss and RMSE, [8 .. 8 + capacity) = ring of the last `capacity` total losses (step t at 8 + t % capacity).
//   RMSE = sqrt(mean((pred - target)^2)) over the first counts[0] vertices x 3 coordinates of sample 0 (train.py:148-150).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void meter_update_kernel(const float* __restrict__ total, const float* __restrict__ lv,
                                                            const float* __restrict__ le, const float* __restrict__ ld,
                                                            const float* __restrict__ pred, long pstride,
                                                            const float* __restrict__ tgt, long tstride,
                                                            const int64_t* __restrict__ count0, int max_v,
                                                            float* __restrict__ state, int capacity) {
    __shared__ float red[4];
    long c = count0 ? count0[0] : (long)max_v;
    c = c < 0 ? 0 : (c > max_v ? max_v : c);
    float s = 0.f;
    for (long i = threadIdx.x; i < c * 3; i += 256) {
        const float d = pred[(i / 3) * pstride + i % 3] - tgt[(i / 3) * tstride + i % 3];
        s += d * d;
    }
    s = wf3d_wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float sq = (red[0] + red[1]) + (red[2] + red[3]);
        const float rmse = c > 0 ? sqrtf(sq / (float)(c * 3)) : 0.f;
        const float t = total[0];
        const long step = (long)state[0];
        state[1] = step == 0 ? t : fminf(state[1], t);
        state[2] = step == 0 ? rmse : fminf(state[2], rmse);
        state[3] = t; state[4] = lv ? lv[0] : 0.f; state[5] = le ? le[0] : 0.f; state[6] = ld ? ld[0] : 0.f; state[7] = rmse;
        if (capacity > 0) state[8 + step % capacity] = t;
        state[0] = (float)(step + 1);
    }
}

extern "C" int wf3d_meter_update(const float* total, const float* vertex_loss, const float* existence_loss, const float* edge_loss,
                                 const float* pred_vertices, long pred_stride, const float* target_vertices, long target_stride,
                                 const int64_t* count0, int max_v, float* state, int capacity, void* stream) {
    WF3D_CHECK(max_v >= 0 && capacity >= 0, WF3D_ERR_ARG, "wf3d_meter_update: bad dims");
    WF3D_CHECK(total && state && (max_v == 0 || (pred_vertices && target_vertices)), WF3D_ERR_ARG, "wf3d_meter_update: null pointer");
    hipLaunchKernelGGL(meter_update_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, total, vertex_loss, existence_loss, edge_loss,
                       pred_vertices, pred_stride, target_vertices, target_stride, count0, max_v, state, capacity);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}
