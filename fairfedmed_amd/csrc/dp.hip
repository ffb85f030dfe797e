// Client-level differential privacy at the FedAvg round boundary: the L2 norm of a client's update
// theta - g over the flat trainable buffer, and the clipped, weighted and noised contribution c_k of that client to the
// round's sum.  Two launches per client; the clip factor is formed on the device and never read back.
#include "common.h"
#include "philox.h"

namespace {

constexpr int kThreads = 256;            // four waves
constexpr int kMaxPartials = 256;        // one fp64 partial per block of the norm pass: re-summed by one block-wide tree
constexpr int kMaxBlocks = 2048;         // elementwise passes (as grid_for of optim.hip)
constexpr int64_t kMaxN = (int64_t)1 << 34;   // the Philox counter word holds i >> 2

inline int norm_blocks(int64_t n) {
    const int64_t b = ((n + 3) / 4 + kThreads - 1) / kThreads;
    return (int)(b > kMaxPartials ? kMaxPartials : b);
}
inline int elem_blocks(int64_t n) {
    const int64_t b = ((n + 3) / 4 + kThreads - 1) / kThreads;
    return (int)(b > kMaxBlocks ? kMaxBlocks : b);
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The four standard normals of group q (elements 4q .. 4q+3 counted from the pointer passed in): counter (q, t, k, 0), key the
// two halves of the seed (low word first); u_j = ((x_j >> 9) + 0.5) 2^-23 is exact in fp32 and strictly inside (0, 1);
// Box-Muller in fp32 on the pairs (u0, u1) and (u2, u3).
__device__ __forceinline__ void gauss4(uint32_t q, uint32_t t, uint32_t k, uint32_t k0, uint32_t k1, float z[4]) {
    uint32_t x[4];
    philox4x32_10(q, t, k, 0u, k0, k1, x);
    float u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = ((float)(x[j] >> 9) + 0.5f) * 1.1920928955078125e-07f;
#pragma unroll
    for (int j = 0; j < 4; j += 2) {
        const float r = sqrtf(-2.0f * logf(u[j]));
        float sn, cs;
        sincosf(6.283185307179586f * u[j + 1], &sn, &cs);
        z[j] = r * cs;
        z[j + 1] = r * sn;
    }
}

// Elements 4q .. 4q+3 of p: one 16-byte load where the caller found every pointer aligned and the group lies inside the
// buffer, otherwise element by element with `fill` behind the end - the same values either way.
__device__ __forceinline__ void load4(const float* p, int64_t i0, int64_t n, bool vec, float fill, float v[4]) {
    if (vec && i0 + 4 <= n) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p + i0);
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i0 + j < n ? p[i0 + j] : fill;
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

// Fixed-order sum over the block: wave64 shuffle tree, then the four wave totals through LDS, added in wave order.  Every
// thread returns the same value.
__device__ __forceinline__ double block_sum(double v, double* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = lds[0];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) s += lds[w];
    __syncthreads();
    return s;
}

// part[block] = sum of (theta - g)^2 over the block's groups: the difference in fp32, squares (exact in fp64) and sums in
// fp64, each thread over its groups in index order.  The order depends on n alone, not on the alignment.
__global__ __launch_bounds__(kThreads) void dp_norm_kernel(const float* __restrict__ theta, const float* __restrict__ g,
                                                           int64_t n, int vec, double* __restrict__ part) {
    __shared__ double lds[kThreads / 64];
    const int64_t groups = (n + 3) / 4;
    double acc = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < groups; q += (int64_t)gridDim.x * kThreads) {
        float a[4], b[4];
        load4(theta, 4 * q, n, vec, 0.f, a);
        load4(g, 4 * q, n, vec, 0.f, b);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double d = (double)(a[j] - b[j]);
            acc += d * d;
        }
    }
    const double s = block_sum(acc, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// out (+)= c_k.  Every block re-sums the norm pass's partials in the same fixed order, so all of them hold the same clip
// factor s: 1 (not clipped: w * theta, the product of ffm_scale_by), C / norm (clipped: w * (g + s * (theta - g))) or 0 (a
// norm that is not finite: w * g, theta does not enter).  Products and sums round separately, as in ffm_scale_acc.
__global__ __launch_bounds__(kThreads) void dp_privatise_kernel(const float* __restrict__ theta, const float* __restrict__ g,
                                                                const float* __restrict__ w, float* out, int64_t n, int vec,
                                                                const double* __restrict__ part, int n_part, float clip,
                                                                float sigma, uint32_t k0, uint32_t k1, uint32_t t, uint32_t k,
                                                                int accumulate, float* __restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ double lds[kThreads / 64];
    const double nu = sqrt(block_sum((int)threadIdx.x < n_part ? part[threadIdx.x] : 0.0, lds));
    float s;
    if (!(nu <= 1.7976931348623157e308)) s = 0.f;          // NaN or Inf
    else if (nu <= (double)clip) s = 1.f;
    else s = (float)((double)clip / nu);
    if (stats && blockIdx.x == 0 && threadIdx.x == 0) {
        stats[0] = (float)nu;
        stats[1] = s;
    }
    const bool whole = s == 1.f, none = s == 0.f;
    const int64_t groups = (n + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < groups; q += (int64_t)gridDim.x * kThreads) {
        float a[4], b[4], ww[4], c[4];
        load4(w, 4 * q, n, vec, 0.f, ww);
        if (!whole) load4(g, 4 * q, n, vec, 0.f, b);
        if (!none) load4(theta, 4 * q, n, vec, 0.f, a);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x;
            if (whole) x = a[j];
            else if (none) x = b[j];
            else {
                const float d = a[j] - b[j];
                const float sd = s * d;
                x = b[j] + sd;
            }
            c[j] = ww[j] * x;
        }
        if (sigma > 0.f) {
            float z[4];
            gauss4((uint32_t)q, t, k, k0, k1, z);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float e = sigma * z[j];
                c[j] = c[j] + e;
            }
        }
        if (accumulate) {
            float o[4];
            load4(out, 4 * q, n, vec, 0.f, o);
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] = o[j] + c[j];
        }
        store4(out, 4 * q, n, vec, c);
    }
}

__global__ __launch_bounds__(kThreads) void dp_noise_kernel(float* __restrict__ out, int64_t n, int vec, float sigma,
                                                            uint32_t k0, uint32_t k1, uint32_t t, uint32_t k) {
#pragma clang fp contract(off)
    const int64_t groups = (n + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < groups; q += (int64_t)gridDim.x * kThreads) {
        float z[4];
        gauss4((uint32_t)q, t, k, k0, k1, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = sigma * z[j];
        store4(out, 4 * q, n, vec, z);
    }
}

// word j = lane j & 3 of Philox4x32-10(counter (c0 + (j >> 2), c1, c2, c3), key)
__global__ __launch_bounds__(kThreads) void dp_philox_kernel(int32_t* __restrict__ out, int64_t n, uint32_t k0, uint32_t k1,
                                                             uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    const int64_t groups = (n + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < groups; q += (int64_t)gridDim.x * kThreads) {
        uint32_t x[4];
        philox4x32_10(c0 + (uint32_t)q, c1, c2, c3, k0, k1, x);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * q + j < n) out[4 * q + j] = (int32_t)x[j];
    }
}

}  // namespace

extern "C" int64_t ffm_dp_norm_ws_bytes(int64_t n) {
    if (n <= 0 || n > kMaxN) return FFM_EINVAL;
    return (int64_t)norm_blocks(n) * (int64_t)sizeof(double);
}

extern "C" int ffm_dp_norm(const float* theta, const float* g, int64_t n, void* scratch, void* stream) {
    if (!theta || !g || !scratch || n <= 0 || ((uintptr_t)scratch & 7)) return FFM_EINVAL;
    if (n > kMaxN) return FFM_EUNSUP;
    const int vec = aligned16(theta) && aligned16(g);
    hipLaunchKernelGGL(dp_norm_kernel, dim3(norm_blocks(n)), dim3(kThreads), 0, (hipStream_t)stream, theta, g, n, vec,
                       (double*)scratch);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}

extern "C" int ffm_dp_privatise(const float* theta, const float* g, const float* w, float* out, int64_t n,
                                const void* scratch, float clip, float sigma, int64_t seed, int round, int client,
                                int accumulate, float* stats, void* stream) {
    if (!theta || !g || !w || !out || !scratch || n <= 0 || ((uintptr_t)scratch & 7)) return FFM_EINVAL;
    if (!(clip > 0.f) || !(sigma >= 0.f) || !(sigma <= 3.4028234663852886e38f)) return FFM_EINVAL;
    if (n > kMaxN) return FFM_EUNSUP;
    const int vec = aligned16(theta) && aligned16(g) && aligned16(w) && aligned16(out);
    hipLaunchKernelGGL(dp_privatise_kernel, dim3(elem_blocks(n)), dim3(kThreads), 0, (hipStream_t)stream, theta, g, w, out, n,
                       vec, (const double*)scratch, norm_blocks(n), clip, sigma, (uint32_t)(uint64_t)seed,
                       (uint32_t)((uint64_t)seed >> 32), (uint32_t)round, (uint32_t)client, accumulate, stats);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}

extern "C" int ffm_dp_noise(float* out, int64_t n, float sigma, int64_t seed, int round, int client, void* stream) {
    if (!out || n <= 0 || !(sigma >= 0.f) || !(sigma <= 3.4028234663852886e38f)) return FFM_EINVAL;
    if (n > kMaxN) return FFM_EUNSUP;
    hipLaunchKernelGGL(dp_noise_kernel, dim3(elem_blocks(n)), dim3(kThreads), 0, (hipStream_t)stream, out, n,
                       (int)aligned16(out), sigma, (uint32_t)(uint64_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint32_t)round,
                       (uint32_t)client);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}

extern "C" int ffm_dp_philox(int32_t* out, int64_t n, int64_t seed, int64_t c0, int64_t c1, int64_t c2, int64_t c3,
                             void* stream) {
    if (!out || n <= 0) return FFM_EINVAL;
    if (n > kMaxN) return FFM_EUNSUP;
    hipLaunchKernelGGL(dp_philox_kernel, dim3(elem_blocks(n)), dim3(kThreads), 0, (hipStream_t)stream, out, n,
                       (uint32_t)(uint64_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint32_t)(uint64_t)c0,
                       (uint32_t)(uint64_t)c1, (uint32_t)(uint64_t)c2, (uint32_t)(uint64_t)c3);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}
