// Client-drift correction in the local step: FedProx's proximal pull towards the round's starting
// point and SCAFFOLD's control variates, as ONE elementwise launch over the flat gradient buffer between the backward pass and
// the optimizer launch.  All float32: no `dtype` argument, no half twin.
#include "common.h"

namespace {

constexpr int kThreads = 256;            // four waves
constexpr int kMaxBlocks = 2048;         // grid cap of the elementwise passes (as elem_blocks of dp.hip)
constexpr int64_t kMaxN = (int64_t)1 << 34;   // the size limit of dp.hip

inline int elem_blocks(int64_t n) {
    const int64_t b = ((n + 3) / 4 + kThreads - 1) / kThreads;
    return (int)(b > kMaxBlocks ? kMaxBlocks : b);
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Elements 4q .. 4q+3 of p (load4 / store4 of dp.hip): one 16-byte access where the caller found every pointer aligned and
// the group lies inside the buffer, otherwise element by element - the same values either way.
__device__ __forceinline__ void load4(const float* p, int64_t i0, int64_t n, bool vec, float v[4]) {
    if (vec && i0 + 4 <= n) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p + i0);
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i0 + j < n ? p[i0 + j] : 0.f;
    }
}
__device__ __forceinline__ void store4(float* p, int64_t i0, int64_t n, bool vec, const float v[4]) {
    if (vec && i0 + 4 <= n) {
        f32x4 a;
        a[0] = v[0]; a[1] = v[1]; a[2] = v[2]; a[3] = v[3];
        *reinterpret_cast<f32x4*>(p + i0) = a;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < n) p[i0 + j] = v[j];
    }
}

// gsum += g (the raw gradient, before anything is added to it); g += mu * (p - anchor); g += c_diff - each an operand that
// may be absent (uniform over the grid), every operation rounded on its own and in this order.  st: the fp16 gradient-scale
// state; an overflowed step (st[2] == 0) changes nothing here, as it changes nothing in the gated optimizer launch behind.
__global__ __launch_bounds__(kThreads) void drift_kernel(float* g, const float* __restrict__ p,
                                                         const float* __restrict__ anchor, float mu,
                                                         const float* __restrict__ c_diff, float* gsum, int64_t* count,
                                                         const float* __restrict__ st, int64_t n, int vec) {
#pragma clang fp contract(off)
    if (st && st[2] == 0.0f) return;
    if (count && blockIdx.x == 0 && threadIdx.x == 0) *count = *count + 1;
    const int64_t groups = (n + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < groups; q += (int64_t)gridDim.x * kThreads) {
        float x[4];
        load4(g, 4 * q, n, vec, x);
        if (gsum) {
            float s[4];
            load4(gsum, 4 * q, n, vec, s);
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] = s[j] + x[j];
            store4(gsum, 4 * q, n, vec, s);
        }
        if (anchor) {
            float a[4], b[4];
            load4(p, 4 * q, n, vec, a);
            load4(anchor, 4 * q, n, vec, b);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = a[j] - b[j];
                const float t = mu * d;
                x[j] = x[j] + t;
            }
        }
        if (c_diff) {
            float c[4];
            load4(c_diff, 4 * q, n, vec, c);
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = x[j] + c[j];
        }
        if (anchor || c_diff) store4(g, 4 * q, n, vec, x);     // (with neither, g[i] = raw is what g already holds)
    }
}

}  // namespace

extern "C" int ffm_drift_correct(float* g, const float* p, const float* anchor, float mu, const float* c_diff, float* gsum,
                                 int64_t* count, const float* scale_state, int64_t n, void* stream) {
    if (!g || n <= 0 || !(fabsf(mu) <= 3.4028234663852886e38f)) return FFM_EINVAL;
    if ((anchor && !p) || (mu != 0.f && !anchor) || (!gsum != !count)) return FFM_EINVAL;
    if (!anchor && !c_diff && !gsum) return FFM_EINVAL;        // nothing to do
    if (n > kMaxN) return FFM_EUNSUP;
    const int vec = aligned16(g) && (!anchor || (aligned16(p) && aligned16(anchor))) && (!c_diff || aligned16(c_diff)) &&
                    (!gsum || aligned16(gsum));
    hipLaunchKernelGGL(drift_kernel, dim3(elem_blocks(n)), dim3(kThreads), 0, (hipStream_t)stream, g, anchor ? p : nullptr,
                       anchor, mu, c_diff, gsum, count, scale_state, n, vec);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}
