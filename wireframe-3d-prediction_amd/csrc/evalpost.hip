// Row f-4: what follows the hot path at evaluation time — evaluate.py:74-110 and the Hausdorff line
// distance of eval/ap_calculator.py:8-36.
//
//   edge_endpoints_kernel   every candidate edge (i < j) of every sample in one launch: keep = prob > threshold (:79),
//                           end points gathered from the predicted vertices with the HIGHER-z vertex first (:88-89:
//                           flip of an ascending argsort over z; on equal z the second vertex comes first) -> the
//                           [B, max_e, 2, 3] / [B, max_e] arrays the host compacts after ONE device->host copy (the
//                           reference copies and loops per sample).
//   hausdorff_lines_kernel  [N, M] symmetric Hausdorff distance between N predicted and M labelled segments, each sampled
//                           at S <= 32 points: one thread per pair, the S x S point distances stay in registers (the
//                           reference materialises a (20 N) x (20 M) cdist matrix: 310 MB at N = 2016, M = 48).  float64,
//                           sample points a + w_k * (b - a) with numpy's linspace weights.
//   compact_{count,scan,place}_kernel   the same selection as a stable stream compaction (wf3d_edge_compact): kept count per
//                           256-candidate chunk, one exclusive scan over all chunk counts (which also yields the per-sample
//                           offsets), placement by wave-ballot rank.  The host then reads B + 1 offsets and K packed rows
//                           instead of B * max_e of them, and never needs the (i, j) index lists.
//   hausdorff_lines_batch_kernel   every sample's [n_s, m_s] matrix in one launch, from the packed float32 segments that are
//                           already on the device; the per-pair arithmetic is hausdorff_pair, shared with the kernel above.
//   decode_{,count_,place_}kernel   wireframe decoding (wf3d_wireframe_decode; specification wf3d/decode.py): per sample the
//                           slots that exist, greedy vertex merging, the edges re-indexed onto the surviving vertices and
//                           packed by the scan above.  The reference has no such step: it evaluates all V slots.
#include "wf3d_common.h"

namespace {

__device__ __forceinline__ int eo(int i, int nv) { return i * nv - (i * (i + 1)) / 2; }     // edges before row i

__global__ __launch_bounds__(256) void edge_endpoints_kernel(const float* __restrict__ verts, long sstride, long vstride,
                                                              const int32_t* __restrict__ counts, const float* __restrict__ probs,
                                                              int max_e, int V, float thr, float* __restrict__ ev,
                                                              unsigned char* __restrict__ keep) {
    const int s = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int nv = counts[s];
    if (idx >= V * V) return;
    const int i = idx / V, j = idx - i * V;
    if (!(i < j && j < nv)) return;
    const int e = eo(i, nv) + (j - i - 1);
    if (e >= max_e) return;
    const float* vi = verts + s * sstride + i * vstride;
    const float* vj = verts + s * sstride + j * vstride;
    const bool i_first = vi[2] > vj[2];
    const float* a = i_first ? vi : vj;
    const float* b = i_first ? vj : vi;
    float* o = ev + ((size_t)s * max_e + e) * 6;
    o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = b[0]; o[4] = b[1]; o[5] = b[2];
    keep[(size_t)s * max_e + e] = probs[(size_t)s * max_e + e] > thr ? 1 : 0;
}

// One (query, target) pair: segments a + w * d and b + w * e sampled at S <= SMAX points each; the S x S point distances
// stay in registers.  Shared by the single-matrix and the batched kernel: the arithmetic is written once.
template <int SMAX>
__device__ __forceinline__ double hausdorff_pair(double ax, double ay, double az, double dx, double dy, double dz, double bx,
                                                 double by, double bz, double ex, double ey, double ez, int S) {
    const double step = S > 1 ? 1.0 / (double)(S - 1) : 0.0;
    double tmin[SMAX];
#pragma unroll
    for (int j = 0; j < SMAX; ++j) tmin[j] = INFINITY;
    double h_pt = 0.0;
    for (int i = 0; i < S; ++i) {
        const double wi = i == S - 1 && S > 1 ? 1.0 : (double)i * step;
        const double px = ax + wi * dx, py = ay + wi * dy, pz = az + wi * dz;
        double rmin = INFINITY;
#pragma unroll
        for (int j = 0; j < SMAX; ++j) {
            if (j < S) {
                const double wj = j == S - 1 && S > 1 ? 1.0 : (double)j * step;
                const double qx = bx + wj * ex - px, qy = by + wj * ey - py, qz = bz + wj * ez - pz;
                const double d = sqrt(qx * qx + qy * qy + qz * qz);
                rmin = fmin(rmin, d);
                tmin[j] = fmin(tmin[j], d);
            }
        }
        h_pt = fmax(h_pt, rmin);
    }
    double h_tp = 0.0;
#pragma unroll
    for (int j = 0; j < SMAX; ++j)
        if (j < S) h_tp = fmax(h_tp, tmin[j]);
    return fmax(h_pt, h_tp);
}

template <int SMAX>
__global__ __launch_bounds__(256) void hausdorff_lines_kernel(const double* __restrict__ pa, const double* __restrict__ pd,
                                                               const double* __restrict__ ta, const double* __restrict__ td,
                                                               int N, int M, int S, double* __restrict__ out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)N * M) return;
    const int n = (int)(idx / M), m = (int)(idx - (long)n * M);
    out[idx] = hausdorff_pair<SMAX>(pa[n * 3], pa[n * 3 + 1], pa[n * 3 + 2], pd[n * 3], pd[n * 3 + 1], pd[n * 3 + 2], ta[m * 3],
                                    ta[m * 3 + 1], ta[m * 3 + 2], td[m * 3], td[m * 3 + 1], td[m * 3 + 2], S);
}

// blockIdx.y = sample, blockIdx.x over the largest n_s * m_s of the batch; float32 end points, direction = an fp32
// subtraction widened afterwards (what numpy's concatenate-then-subtract gives for float32 predictions and labels).
template <int SMAX>
__global__ __launch_bounds__(256) void hausdorff_lines_batch_kernel(const float* __restrict__ seg, const int32_t* __restrict__ koff,
                                                                     const float* __restrict__ lseg, const int32_t* __restrict__ loff,
                                                                     const int64_t* __restrict__ ooff, int S, double* __restrict__ out) {
    const int s = blockIdx.y;
    const int k0 = koff[s], l0 = loff[s];
    const long N = koff[s + 1] - k0, M = loff[s + 1] - l0;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (N <= 0 || M <= 0 || idx >= N * M) return;
    const long n = idx / M, m = idx - n * M;
    const float* p = seg + (k0 + n) * 6;
    const float* t = lseg + (l0 + m) * 6;
    const float dx = p[3] - p[0], dy = p[4] - p[1], dz = p[5] - p[2];
    const float ex = t[3] - t[0], ey = t[4] - t[1], ez = t[5] - t[2];
    out[ooff[s] + idx] = hausdorff_pair<SMAX>((double)p[0], (double)p[1], (double)p[2], (double)dx, (double)dy, (double)dz,
                                              (double)t[0], (double)t[1], (double)t[2], (double)ex, (double)ey, (double)ez, S);
}

// ---- stable compaction of the kept candidate edges ---------------------------------------------------------------------
// A chunk is the 256 candidates of one workgroup: 4 waves of 64, each lane one candidate.  The kept flag is the same
// expression in the count and in the placement pass.
constexpr int CHUNK = 256, SCAN_TILE = 1024;

__device__ __forceinline__ int clamp_count(int c, int V) { return min(max(c, 0), V); }

__device__ __forceinline__ bool edge_kept(const float* __restrict__ probs, int s, int e, int c, int max_e, float thr) {
    const long E = (long)c * (c - 1) / 2;
    return e < max_e && (long)e < E && probs[(size_t)s * max_e + e] > thr;          // NaN > thr is false
}

// kept lanes of this wave below this lane, and in the whole wave (wave64: the ballot is 64 bits wide)
__device__ __forceinline__ int wave_rank(bool kept, int lane, int& total) {
    const unsigned long long b = __ballot(kept);
    total = __popcll(b);
    return __popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(CHUNK) void compact_count_kernel(const int32_t* __restrict__ counts, const float* __restrict__ probs,
                                                              int max_e, int V, float thr, int32_t* __restrict__ chunk_cnt) {
    __shared__ int wsum[CHUNK / 64];
    const int s = blockIdx.y, e = blockIdx.x * CHUNK + threadIdx.x;
    int total;
    wave_rank(edge_kept(probs, s, e, clamp_count(counts[s], V), max_e, thr), threadIdx.x & 63, total);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = total;
    __syncthreads();
    if (threadIdx.x == 0) chunk_cnt[(size_t)s * gridDim.x + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// One workgroup walks the T = B * nchunk chunk counts in tiles of SCAN_TILE and turns them into their exclusive prefix in
// place; the entry of a sample's first chunk is that sample's koff.
__global__ __launch_bounds__(SCAN_TILE) void compact_scan_kernel(int32_t* __restrict__ chunk, int T, int nchunk, int B,
                                                                 int32_t* __restrict__ koff) {
    __shared__ int wtot[SCAN_TILE / 64];
    __shared__ int carry_s;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < T; base += SCAN_TILE) {
        const int t = base + threadIdx.x;
        const int v = t < T ? chunk[t] : 0;
        int inc = v;                                             // inclusive scan inside the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) wtot[w] = inc;
        const int carry = carry_s;
        __syncthreads();
        int before = 0;                                          // kept edges of this tile's earlier waves
        for (int k = 0; k < w; ++k) before += wtot[k];
        const int excl = carry + before + inc - v;
        if (t < T) {
            chunk[t] = excl;
            if (t % nchunk == 0) koff[t / nchunk] = excl;
        }
        __syncthreads();
        if (threadIdx.x == SCAN_TILE - 1) carry_s = excl + v;
        __syncthreads();
    }
    if (threadIdx.x == 0) koff[B] = carry_s;
}

__global__ __launch_bounds__(CHUNK) void compact_place_kernel(const float* __restrict__ verts, long sstride, long vstride,
                                                              const int32_t* __restrict__ counts, const float* __restrict__ probs,
                                                              int max_e, int V, float thr, const int32_t* __restrict__ chunk_off,
                                                              int32_t* __restrict__ pairs, float* __restrict__ seg,
                                                              float* __restrict__ kprob) {
    __shared__ int wsum[CHUNK / 64];
    const int s = blockIdx.y, e = blockIdx.x * CHUNK + threadIdx.x;
    const int c = clamp_count(counts[s], V);
    const bool kept = edge_kept(probs, s, e, c, max_e, thr);
    int total;
    const int rank = wave_rank(kept, threadIdx.x & 63, total);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = total;
    __syncthreads();
    if (!kept) return;
    int pos = chunk_off[(size_t)s * gridDim.x + blockIdx.x] + rank;
    for (int k = 0; k < (int)(threadIdx.x >> 6); ++k) pos += wsum[k];
    int i, j;
    edge_ij(e, c, i, j);                                         // float estimate, integer fix-up: exact
    const float* vi = verts + s * sstride + i * vstride;
    const float* vj = verts + s * sstride + j * vstride;
    const bool i_first = vi[2] > vj[2];
    const float* a = i_first ? vi : vj;
    const float* b = i_first ? vj : vi;
    float* o = seg + (size_t)pos * 6;
    o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = b[0]; o[4] = b[1]; o[5] = b[2];
    pairs[(size_t)pos * 2] = i;
    pairs[(size_t)pos * 2 + 1] = j;
    kprob[pos] = probs[(size_t)s * max_e + e];
}

// ---- wireframe decoding (wf3d_wireframe_decode; the specification is wf3d/decode.py) -----------------------------------
// decode_kernel, one workgroup per sample, everything per slot in LDS: alive flags, the visiting order as a rank computed
// by counting, greedy suppression in at most V rounds of one barrier ("the next unclaimed slot in order claims every
// later slot within r"), then the surviving candidates' maximum probability per pair of representatives in the caller's
// workspace pmax [B, V, V] (atomicMax on an order-preserving key: a maximum gives the same bits on every run), then the
// output vertices in slot order.  The edges then go through the compaction above: count / scan / place over the
// n (n - 1) / 2 pairs of output vertices.  Every loop is bounded by V or max_e; none ends on a data value.
constexpr int DEC_MAX = 1024, DEC_THREADS = 256;

// a float as an unsigned key of the same order (0.0 above -0.0).  Only a NaN maps to 0: the mark of a pair no candidate reached.
__device__ __forceinline__ unsigned prob_key(float p) {
    const unsigned b = __float_as_uint(p);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_prob(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// (dx dx + dy dy) + dz dz in fp64, each operation rounded on its own: pt_dist of evalmetrics.hip without the root
__device__ __forceinline__ double slot_d2(const float* a, const float* b) {
#pragma clang fp contract(off)
    const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1], dz = (double)a[2] - (double)b[2];
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const double xy = xx + yy;
    return xy + zz;
}

__global__ __launch_bounds__(DEC_THREADS) void decode_kernel(const float* __restrict__ verts, long sstride, long vstride,
                                                             const float* __restrict__ exist, long estride,
                                                             const int32_t* __restrict__ counts, const float* __restrict__ probs,
                                                             int V, int max_e, float ethr, float thr, double r2, int drop,
                                                             int32_t* __restrict__ nverts, float* __restrict__ dverts,
                                                             int32_t* __restrict__ slots, int32_t* __restrict__ status,
                                                             unsigned* __restrict__ pmax_all) {
    __shared__ float Xs[DEC_MAX * 3], Es[DEC_MAX];
    __shared__ int alive_s[DEC_MAX], rank_s[DEC_MAX], order_s[DEC_MAX], rep_s[DEC_MAX], used_s[DEC_MAX];   // rank -1: not alive
    __shared__ int st_s, nalive_s, n_s;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int c = clamp_count(counts[s], V);
    if (tid == 0) { st_s = 0; nalive_s = 0; n_s = 0; }
    __syncthreads();
    // 1. alive slots
    int st = 0;
    for (int i = tid; i < V; i += DEC_THREADS) {
        float x = 0.f, y = 0.f, z = 0.f, e = 0.f;
        bool alive = false;
        if (i < c) {
            const float* p = verts + s * sstride + i * vstride;
            x = p[0]; y = p[1]; z = p[2];
            e = exist[((long)s * V + i) * estride];
            const bool fin = isfinite(x) && isfinite(y) && isfinite(z) && e == e;
            if (!fin) st = WF3D_DECODE_NONFINITE;
            alive = fin && (ethr == -INFINITY || e > ethr);
        }
        Xs[3 * i] = x; Xs[3 * i + 1] = y; Xs[3 * i + 2] = z; Es[i] = e;
        alive_s[i] = alive ? 1 : 0;
        rank_s[i] = -1;
        rep_s[i] = -1;
        used_s[i] = 0;
    }
    if (st) atomicOr(&st_s, st);
    __syncthreads();
    // 2. the visiting order (existence descending, slot ascending) as a rank, by counting
    int mine = 0;
    for (int i = tid; i < V; i += DEC_THREADS) {
        if (!alive_s[i]) continue;
        const float e = Es[i];
        int r = 0;
        for (int k = 0; k < V; ++k) r += (alive_s[k] && (Es[k] > e || (Es[k] == e && k < i))) ? 1 : 0;
        rank_s[i] = r;
        order_s[r] = i;
        ++mine;
    }
    if (mine) atomicAdd(&nalive_s, mine);
    __syncthreads();
    const int nalive = nalive_s;
    // greedy suppression: rep < 0 = unclaimed.  Round t: the t-th slot in order, if still unclaimed, is a representative
    // and claims every later unclaimed slot within the radius; an earlier representative has claimed first.  rep[i] is
    // written by the thread that owns slot i alone, and rep[order[t]] not after round t - 1.
    if (r2 >= 0.0) {
        for (int t = 0; t < nalive; ++t) {
            const int o = order_s[t];
            if (rep_s[o] < 0) {
                for (int i = tid; i < V; i += DEC_THREADS)
                    if (rank_s[i] > t && rep_s[i] < 0 && slot_d2(Xs + 3 * i, Xs + 3 * o) <= r2) rep_s[i] = o;
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < V; i += DEC_THREADS)
        if (rank_s[i] >= 0 && rep_s[i] < 0) rep_s[i] = i;
    // 3. the maximum probability per pair of representatives (slot indices, lower first)
    if (pmax_all) {
        unsigned* pmax = pmax_all + (size_t)s * V * V;
        for (int idx = tid; idx < c * c; idx += DEC_THREADS) pmax[(size_t)(idx / c) * V + idx % c] = 0u;
        __threadfence();
        __syncthreads();
        const long E = (long)c * (c - 1) / 2;
        const int ne = (int)(E < (long)max_e ? E : (long)max_e);
        for (int e = tid; e < ne; e += DEC_THREADS) {
            const float p = probs[(size_t)s * max_e + e];
            if (!(p > thr)) continue;                                    // NaN and equality do not pass
            int i, j;
            edge_ij(e, c, i, j);
            if (rank_s[i] < 0 || rank_s[j] < 0) continue;
            const int a = rep_s[i], b = rep_s[j];
            if (a == b) continue;
            const int lo = a < b ? a : b, hi = a < b ? b : a;
            atomicMax(&pmax[(size_t)lo * V + hi], prob_key(p));
            atomicOr(&used_s[lo], 1);
            atomicOr(&used_s[hi], 1);
        }
        __threadfence();
    }
    __syncthreads();
    // 4. the output vertices: the kept representatives in slot order (order_s now holds the keep flags)
    for (int i = tid; i < V; i += DEC_THREADS) order_s[i] = (rank_s[i] >= 0 && rep_s[i] == i && (!drop || used_s[i])) ? 1 : 0;
    __syncthreads();
    mine = 0;
    for (int i = tid; i < V; i += DEC_THREADS) {
        if (!order_s[i]) continue;
        int n = 0;
        for (int k = 0; k < i; ++k) n += order_s[k];
        slots[(size_t)s * V + n] = i;
        float* o = dverts + ((size_t)s * V + n) * 3;
        o[0] = Xs[3 * i]; o[1] = Xs[3 * i + 1]; o[2] = Xs[3 * i + 2];
        ++mine;
    }
    if (mine) atomicAdd(&n_s, mine);
    __syncthreads();
    const int n = n_s;
    for (int k = n + tid; k < V; k += DEC_THREADS) {
        slots[(size_t)s * V + k] = -1;
        float* o = dverts + ((size_t)s * V + k) * 3;
        o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
    }
    if (tid == 0) { nverts[s] = n; status[s] = st_s; }
}

// The key of pair t = (p, q), p < q < n_s, of sample s's output vertices in lexicographic order; 0: no edge.
__device__ __forceinline__ unsigned decoded_pair(const unsigned* __restrict__ pmax_all, const int32_t* __restrict__ nverts,
                                                 const int32_t* __restrict__ slots, int s, int t, int V, int& p, int& q) {
    const int n = clamp_count(nverts[s], V);
    if ((long)t >= (long)n * (n - 1) / 2) return 0u;
    edge_ij(t, n, p, q);
    const int a = slots[(size_t)s * V + p], b = slots[(size_t)s * V + q];
    if (a < 0 || b < 0 || a >= V || b >= V) return 0u;
    return pmax_all[(size_t)s * V * V + (size_t)a * V + b];
}

__global__ __launch_bounds__(CHUNK) void decode_count_kernel(const unsigned* __restrict__ pmax_all, const int32_t* __restrict__ nverts,
                                                             const int32_t* __restrict__ slots, int V,
                                                             int32_t* __restrict__ chunk_cnt) {
    __shared__ int wsum[CHUNK / 64];
    const int s = blockIdx.y, t = blockIdx.x * CHUNK + threadIdx.x;
    int p, q, total;
    wave_rank(decoded_pair(pmax_all, nverts, slots, s, t, V, p, q) != 0u, threadIdx.x & 63, total);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = total;
    __syncthreads();
    if (threadIdx.x == 0) chunk_cnt[(size_t)s * gridDim.x + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(CHUNK) void decode_place_kernel(const unsigned* __restrict__ pmax_all, const int32_t* __restrict__ nverts,
                                                             const int32_t* __restrict__ slots, const float* __restrict__ dverts,
                                                             int V, const int32_t* __restrict__ chunk_off,
                                                             int32_t* __restrict__ pairs, float* __restrict__ seg,
                                                             float* __restrict__ kprob) {
    __shared__ int wsum[CHUNK / 64];
    const int s = blockIdx.y, t = blockIdx.x * CHUNK + threadIdx.x;
    int p = 0, q = 0, total;
    const unsigned key = decoded_pair(pmax_all, nverts, slots, s, t, V, p, q);
    const int rank = wave_rank(key != 0u, threadIdx.x & 63, total);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = total;
    __syncthreads();
    if (key == 0u) return;
    int pos = chunk_off[(size_t)s * gridDim.x + blockIdx.x] + rank;
    for (int k = 0; k < (int)(threadIdx.x >> 6); ++k) pos += wsum[k];
    const float* vp = dverts + ((size_t)s * V + p) * 3;
    const float* vq = dverts + ((size_t)s * V + q) * 3;
    const bool p_first = vp[2] > vq[2];                          // equal z: vertex q first, as in compact_place_kernel
    const float* a = p_first ? vp : vq;
    const float* b = p_first ? vq : vp;
    float* o = seg + (size_t)pos * 6;
    o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = b[0]; o[4] = b[1]; o[5] = b[2];
    pairs[(size_t)pos * 2] = p;
    pairs[(size_t)pos * 2 + 1] = q;
    kprob[pos] = key_prob(key);
}

}  // namespace

extern "C" int wf3d_edge_endpoints(const float* verts, long sample_stride, long vertex_stride, const int32_t* counts,
                                   const float* probs, int B, int V, int max_e, float threshold, float* edge_vertices,
                                   unsigned char* keep, void* stream) {
    WF3D_CHECK(B >= 0 && V >= 0 && max_e >= 0, WF3D_ERR_ARG, "wf3d_edge_endpoints: bad dims");
    if (B == 0 || V < 2 || max_e == 0) return WF3D_OK;
    WF3D_CHECK(verts && counts && probs && edge_vertices && keep, WF3D_ERR_ARG, "wf3d_edge_endpoints: null pointer");
    WF3D_CHECK(B <= 65535, WF3D_ERR_UNSUPPORTED, "wf3d_edge_endpoints: B > 65535");
    hipLaunchKernelGGL(edge_endpoints_kernel, dim3(wf3d_cdiv((long)V * V, 256), B), dim3(256), 0, (hipStream_t)stream, verts,
                       sample_stride, vertex_stride, counts, probs, max_e, V, threshold, edge_vertices, keep);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" int wf3d_hausdorff_lines(const double* p_start, const double* p_diff, const double* t_start, const double* t_diff,
                                    int N, int M, int sample_points, double* out, void* stream) {
    WF3D_CHECK(N >= 0 && M >= 0 && sample_points >= 1 && sample_points <= 32, WF3D_ERR_UNSUPPORTED,
               "wf3d_hausdorff_lines: 1..32 sample points per segment (got %d)", sample_points);
    if (N == 0 || M == 0) return WF3D_OK;
    WF3D_CHECK(p_start && p_diff && t_start && t_diff && out, WF3D_ERR_ARG, "wf3d_hausdorff_lines: null pointer");
    hipLaunchKernelGGL(hausdorff_lines_kernel<32>, dim3(wf3d_cdiv((long)N * M, 256)), dim3(256), 0, (hipStream_t)stream, p_start,
                       p_diff, t_start, t_diff, N, M, sample_points, out);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" size_t wf3d_edge_compact_ws_bytes(int B, int max_e) {
    if (B <= 0 || max_e <= 0) return 0;
    return (size_t)B * (size_t)wf3d_cdiv(max_e, CHUNK) * sizeof(int32_t);
}

extern "C" int wf3d_edge_compact(const float* verts, long sample_stride, long vertex_stride, const int32_t* counts,
                                 const float* probs, int B, int V, int max_e, float threshold, int32_t* koff, int32_t* pairs,
                                 float* seg, float* kprob, void* ws, size_t ws_bytes, void* stream) {
    WF3D_CHECK(B >= 0 && V >= 0 && max_e >= 0, WF3D_ERR_ARG, "wf3d_edge_compact: bad dims");
    WF3D_CHECK(koff, WF3D_ERR_ARG, "wf3d_edge_compact: null koff");
    WF3D_CHECK(B <= 65535, WF3D_ERR_UNSUPPORTED, "wf3d_edge_compact: B > 65535 (got %d)", B);
    WF3D_CHECK((long)B * max_e < (1L << 31), WF3D_ERR_UNSUPPORTED, "wf3d_edge_compact: B * max_e >= 2^31 (B %d, max_e %d)", B,
               max_e);
    hipStream_t st = (hipStream_t)stream;
    if (B == 0 || V < 2 || max_e == 0) {
        if (hipMemsetAsync(koff, 0, (size_t)(B + 1) * sizeof(int32_t), st) != hipSuccess) {
            (void)hipGetLastError();
            WF3D_CHECK(false, WF3D_ERR_LAUNCH, "wf3d_edge_compact: clearing koff failed");
        }
        return WF3D_OK;
    }
    WF3D_CHECK(verts && counts && probs && pairs && seg && kprob, WF3D_ERR_ARG, "wf3d_edge_compact: null pointer");
    WF3D_CHECK(ws && ws_bytes >= wf3d_edge_compact_ws_bytes(B, max_e), WF3D_ERR_ARG,
               "wf3d_edge_compact: workspace of %zu bytes, %zu needed", ws_bytes, wf3d_edge_compact_ws_bytes(B, max_e));
    const int nchunk = wf3d_cdiv(max_e, CHUNK);
    int32_t* chunk = (int32_t*)ws;
    hipLaunchKernelGGL(compact_count_kernel, dim3(nchunk, B), dim3(CHUNK), 0, st, counts, probs, max_e, V, threshold, chunk);
    WF3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(SCAN_TILE), 0, st, chunk, B * nchunk, nchunk, B, koff);
    WF3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(compact_place_kernel, dim3(nchunk, B), dim3(CHUNK), 0, st, verts, sample_stride, vertex_stride, counts,
                       probs, max_e, V, threshold, chunk, pairs, seg, kprob);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

extern "C" int wf3d_hausdorff_lines_batch(const float* seg, const int32_t* koff, const float* lseg, const int32_t* loff,
                                          const int64_t* ooff, int B, long max_pairs, int sample_points, double* out,
                                          void* stream) {
    WF3D_CHECK(sample_points >= 1 && sample_points <= 32, WF3D_ERR_UNSUPPORTED,
               "wf3d_hausdorff_lines_batch: 1..32 sample points per segment (got %d)", sample_points);
    WF3D_CHECK(B >= 0 && max_pairs >= 0, WF3D_ERR_ARG, "wf3d_hausdorff_lines_batch: bad dims");
    WF3D_CHECK(B <= 65535, WF3D_ERR_UNSUPPORTED, "wf3d_hausdorff_lines_batch: B > 65535 (got %d)", B);
    WF3D_CHECK((max_pairs + 255) / 256 < (1L << 31), WF3D_ERR_UNSUPPORTED, "wf3d_hausdorff_lines_batch: max_pairs %ld too large",
               max_pairs);
    if (B == 0 || max_pairs == 0) return WF3D_OK;
    WF3D_CHECK(seg && koff && lseg && loff && ooff && out, WF3D_ERR_ARG, "wf3d_hausdorff_lines_batch: null pointer");
    hipLaunchKernelGGL(hausdorff_lines_batch_kernel<32>, dim3(wf3d_cdiv(max_pairs, 256), B), dim3(256), 0, (hipStream_t)stream,
                       seg, koff, lseg, loff, ooff, sample_points, out);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}

static size_t decode_pmax_bytes(int B, int V) { return ((size_t)B * V * V * sizeof(uint32_t) + 15) / 16 * 16; }
static int decode_nchunk(int V) { return wf3d_cdiv((long)V * (V - 1) / 2, CHUNK); }

extern "C" size_t wf3d_wireframe_decode_ws_bytes(int B, int V, int max_e) {
    if (B <= 0 || V < 2 || max_e <= 0) return 0;                 // no candidate pair: the vertices need no workspace
    return decode_pmax_bytes(B, V) + (size_t)B * (size_t)decode_nchunk(V) * sizeof(int32_t);
}

extern "C" int wf3d_wireframe_decode(const float* verts, long sample_stride, long vertex_stride, const float* exist,
                                     long exist_stride, const int32_t* counts, const float* probs, int B, int V, int max_e,
                                     float exist_threshold, float edge_threshold, double merge_radius, int drop_isolated,
                                     int32_t* nverts, float* dverts, int32_t* slots, int32_t* koff, int32_t* pairs, float* seg,
                                     float* kprob, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    WF3D_CHECK(B >= 0 && V >= 0 && max_e >= 0, WF3D_ERR_ARG, "wf3d_wireframe_decode: bad dims");
    WF3D_CHECK(exist_threshold == exist_threshold && edge_threshold == edge_threshold && merge_radius == merge_radius,
               WF3D_ERR_ARG, "wf3d_wireframe_decode: a threshold or the merge radius is NaN");
    WF3D_CHECK(V <= DEC_MAX, WF3D_ERR_UNSUPPORTED, "wf3d_wireframe_decode: at most 1024 vertex slots per sample (V %d)", V);
    WF3D_CHECK(B <= 65535, WF3D_ERR_UNSUPPORTED, "wf3d_wireframe_decode: B > 65535 (got %d)", B);
    WF3D_CHECK((long)B * max_e < (1L << 31), WF3D_ERR_UNSUPPORTED, "wf3d_wireframe_decode: B * max_e >= 2^31 (B %d, max_e %d)", B,
               max_e);
    if (B == 0) return WF3D_OK;
    const size_t need = wf3d_wireframe_decode_ws_bytes(B, V, max_e);
    WF3D_CHECK(need == 0 || (ws && ws_bytes >= need), WF3D_ERR_WS, "wf3d_wireframe_decode: workspace of %zu bytes, %zu needed",
               ws_bytes, need);
    WF3D_CHECK(counts && nverts && koff && status, WF3D_ERR_ARG, "wf3d_wireframe_decode: null pointer");
    WF3D_CHECK(V == 0 || (verts && exist && dverts && slots), WF3D_ERR_ARG, "wf3d_wireframe_decode: null vertex pointer");
    WF3D_CHECK(need == 0 || (probs && pairs && seg && kprob), WF3D_ERR_ARG, "wf3d_wireframe_decode: null edge pointer");
    hipStream_t st = (hipStream_t)stream;
    unsigned* pmax = need ? (unsigned*)ws : nullptr;
    const double r2 = merge_radius < 0.0 ? -1.0 : merge_radius * merge_radius;
    hipLaunchKernelGGL(decode_kernel, dim3(B), dim3(DEC_THREADS), 0, st, verts, sample_stride, vertex_stride, exist, exist_stride,
                       counts, probs, V, max_e, exist_threshold, edge_threshold, r2, drop_isolated ? 1 : 0, nverts, dverts, slots,
                       status, pmax);
    WF3D_LAUNCH_CHECK();
    if (!need) {
        if (hipMemsetAsync(koff, 0, (size_t)(B + 1) * sizeof(int32_t), st) != hipSuccess) {
            (void)hipGetLastError();
            WF3D_CHECK(false, WF3D_ERR_LAUNCH, "wf3d_wireframe_decode: clearing koff failed");
        }
        return WF3D_OK;
    }
    const int nchunk = decode_nchunk(V);
    int32_t* chunk = (int32_t*)((unsigned char*)ws + decode_pmax_bytes(B, V));
    hipLaunchKernelGGL(decode_count_kernel, dim3(nchunk, B), dim3(CHUNK), 0, st, pmax, nverts, slots, V, chunk);
    WF3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(SCAN_TILE), 0, st, chunk, B * nchunk, nchunk, B, koff);
    WF3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(decode_place_kernel, dim3(nchunk, B), dim3(CHUNK), 0, st, pmax, nverts, slots, dverts, V, chunk, pairs, seg,
                       kprob);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}
