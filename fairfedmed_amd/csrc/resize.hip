// Native-size uint8 transport: the datasets resize every sample whose stored height
// is not INPUT.SIZE with skimage.transform.resize on the host (utils/data_utils.py:640-646, 662-667) and ship the float
// result.  That resize is linear and separable apart from its final clip,
//     out = clip(A_y X A_x^T, min X, max X),
// with one short contiguous run of non-zero taps per row of A (fairfedmed_amd/data.py: resize_taps), so the loader ships
// the stored bytes of a ragged batch with the tap tables of its distinct geometries and this kernel leaves the float32
// [B, C1*rep, R, R] batch the engines consume.
#include "common.h"

namespace {

constexpr int kStrips = 8;      // blocks per plane: each takes ceil(R / 8) output rows

// One block = one plane and one strip of its output rows.  The block first reduces the plane's minimum and maximum (every
// strip of a plane repeats that over the same bytes, from L2: the call allocates nothing and needs no second launch), then
// each thread forms 4 adjacent output columns of one row: per horizontal tap the vertical taps in ascending order, then the
// horizontal taps in ascending order - the two-pass sums, element by element, without the intermediate image.
__global__ __launch_bounds__(256) void resize_u8_kernel(const uint8_t* __restrict__ pix, const int32_t* __restrict__ geom,
                                                        const int32_t* __restrict__ tab_start, const float* __restrict__ tab_w,
                                                        float* __restrict__ dst, int C1, int rep, int R, int T) {
    __shared__ int s_lo[4], s_hi[4];
    const int plane = blockIdx.x / kStrips, strip = blockIdx.x % kStrips;
    const int b = plane / C1, ch = plane % C1;
    const int off = geom[4 * b], H = geom[4 * b + 1], W = geom[4 * b + 2], tab = geom[4 * b + 3];
    if (off < 0 || H <= 0 || W <= 0 || tab < 0) return;                  // (uniform over the block)
    const int n = H * W;
    const uint8_t* src = pix + (size_t)off + (size_t)ch * n;

    // ---- the plane's range: bytes up to the first 4-byte boundary, aligned words, the bytes left over
    int lo = 255, hi = 0;
    int head = (int)((4 - ((uintptr_t)src & 3)) & 3);
    if (head > n) head = n;
    const int words = (n - head) >> 2;
    if ((int)threadIdx.x < head) {
        const int v = src[threadIdx.x];
        lo = min(lo, v), hi = max(hi, v);
    }
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src + head);
    for (int i = threadIdx.x; i < words; i += 256) {
        const uint32_t v = s4[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = (int)((v >> (8 * k)) & 255u);
            lo = min(lo, e), hi = max(hi, e);
        }
    }
    for (int i = head + 4 * words + threadIdx.x; i < n; i += 256) {
        const int v = src[i];
        lo = min(lo, v), hi = max(hi, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, 64));
        hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) s_lo[threadIdx.x >> 6] = lo, s_hi[threadIdx.x >> 6] = hi;
    __syncthreads();
    const float flo = (float)min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3]));
    const float fhi = (float)max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3]));

    // ---- the strip's outputs
    const int rows = (R + kStrips - 1) / kStrips;
    const int r0 = strip * rows, r1 = min(R, r0 + rows);
    const int q4 = R >> 2;
    const int32_t* sy = tab_start + (size_t)(2 * tab) * R;
    const int32_t* sx = sy + R;
    const float* wy = tab_w + (size_t)(2 * tab) * R * T;
    const float* wx = wy + (size_t)R * T;
    float* out = dst + (size_t)plane * rep * R * R;
    for (int q = threadIdx.x; q < (r1 - r0) * q4; q += 256) {
        const int r = r0 + q / q4, c = (q % q4) * 4;
        const int y0 = sy[r];
        const float* wyr = wy + (size_t)r * T;
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x0 = sx[c + j];
            const float* wxr = wx + (size_t)(c + j) * T;
            float acc = 0.f;
            for (int tx = 0; tx < T; ++tx) {
                const float wh = wxr[tx];
                if (wh == 0.f) continue;                                 // (padding: adds an exact zero)
                const int x = min(max(x0 + tx, 0), W - 1);
                float v = 0.f;
                for (int ty = 0; ty < T; ++ty) {
                    const int y = min(max(y0 + ty, 0), H - 1);
                    v += wyr[ty] * (float)src[y * W + x];
                }
                acc += wh * v;
            }
            o[j] = fminf(fmaxf(acc, flo), fhi);
        }
        float* p = out + (size_t)r * R + c;
        for (int k = 0; k < rep; ++k) *reinterpret_cast<f32x4*>(p + (size_t)k * R * R) = o;
    }
}

}  // namespace

extern "C" int ffm_resize_u8(const uint8_t* pix, const int32_t* geom, const int32_t* tab_start, const float* tab_w, float* dst,
                             int B, int C1, int rep, int R, int T, void* stream) {
    if (!pix || !geom || !tab_start || !tab_w || !dst || B <= 0 || C1 <= 0 || rep <= 0 || R <= 0 || T <= 0) return FFM_EINVAL;
    if (((uintptr_t)geom & 3) || ((uintptr_t)tab_start & 3) || ((uintptr_t)tab_w & 3) || ((uintptr_t)dst & 15)) return FFM_EINVAL;
    if (R % 4 || T > FFM_RESIZE_MAX_TAPS || (long long)B * C1 > (1ll << 27)) return FFM_EUNSUP;
    hipLaunchKernelGGL(resize_u8_kernel, dim3((unsigned)(B * C1 * kStrips)), dim3(256), 0, (hipStream_t)stream, pix, geom,
                       tab_start, tab_w, dst, C1, rep, R, T);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}
