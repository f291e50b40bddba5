// Device-side dropout seeds (wf3d.random.DropoutGenerator): a generator whose state lives in device memory and a
// per-thread seed source for the mask kernels, so that a captured training step draws fresh masks on every replay.
//
//   wf3d_dropout_draw            one thread: s = hash(key, counter); words[k] = s + k * 0x9E3779B9 (k = 0..4), the
//                                per-site derivation of EdgeFn.forward; then counter += 1
//   wf3d_set_dropout_seed_words  while non-NULL, the drop_seed of every mask launch on this thread is an index into
//                                these words, loaded by the kernel itself (wf3d_seed_t, wf3d_common.h)
//   wf3d_set_live_rows           while non-NULL, the edge-row launches on this thread stop at the 256-row boundary above
//                                the int32 this points to (wf3d_live_extent, wf3d_common.h)
#include "wf3d_common.h"

static thread_local const uint32_t* g_seed_words = nullptr;

wf3d_seed_t wf3d_seed_arg(float drop_p, uint32_t drop_seed) {
    return wf3d_seed_t{drop_seed, drop_p > 0.f ? g_seed_words : nullptr};
}

extern "C" int wf3d_set_dropout_seed_words(const uint32_t* words) {
    g_seed_words = words;
    return WF3D_OK;
}

// The live-row count of the calling thread (include/wf3d.h, "LIVE ROW COUNT"): a device pointer that is handed to the
// kernels and never dereferenced on the host.
static thread_local const int32_t* g_live_rows = nullptr;

const int32_t* wf3d_live_rows() { return g_live_rows; }

extern "C" int wf3d_set_live_rows(const int32_t* rows) {
    g_live_rows = rows;
    return WF3D_OK;
}

namespace {

// state = {key, counter}.  The seed of draw number `counter` is splitmix64 (Steele, Lea, Flood 2014) at that position
// of the key's stream, low 32 bits:
//   z = key + (counter + 1) * 0x9E3779B97F4A7C15
//   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31
//   s = z mod 2^32
__global__ __launch_bounds__(64) void dropout_draw_kernel(uint64_t* __restrict__ state, uint32_t* __restrict__ words) {
    if (threadIdx.x != 0) return;
    const uint64_t key = state[0], ctr = state[1];
    uint64_t z = key + (ctr + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const uint32_t s = (uint32_t)z;
#pragma unroll
    for (int k = 0; k < 5; ++k) words[k] = s + 0x9E3779B9u * (uint32_t)k;
    state[1] = ctr + 1;
}

}  // namespace

extern "C" int wf3d_dropout_draw(uint64_t* state, uint32_t* words, void* stream) {
    WF3D_CHECK(state && words, WF3D_ERR_ARG, "wf3d_dropout_draw: null pointer");
    hipLaunchKernelGGL(dropout_draw_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, words);
    WF3D_LAUNCH_CHECK();
    return WF3D_OK;
}
