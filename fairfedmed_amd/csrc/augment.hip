// Train-time augmentation on the stored bytes: torchvision's RandomResizedCrop and RandomHorizontalFlip
// on a PIL image - crop, then Pillow's antialiased resize - for a ragged data.NativeBatch.  Every sample is its own geometry, so
// nothing is tabulated on the host: ffm_augment_boxes draws each sample's box and flip from the counter-based generator
// (philox.h, keyed by seed / epoch / sample id), and ffm_crop_resize_u8 builds that sample's filter taps in LDS and resamples
// box -> R x R in one pass, leaving the float32 [B, C1*rep, R, R] batch the engines consume.
#include "common.h"
#include "philox.h"

namespace {

constexpr int kStrips = 8;              // blocks per plane: each takes ceil(R / 8) output rows (resize.hip)
constexpr uint32_t kTag = 0x4D475541u;  // fourth counter word of every augmentation draw
constexpr int kAttempts = 10;

__device__ __forceinline__ double unit(uint32_t x) { return ((double)(x >> 9) + 0.5) * 0x1p-23; }

// One thread = one sample: the ten attempts of RandomResizedCrop.get_params, its central fallback, and the flip.
__global__ __launch_bounds__(64) void augment_boxes_kernel(const int32_t* __restrict__ geom, const int32_t* __restrict__ ids,
                                                           int B, uint32_t k0, uint32_t k1, uint32_t epoch, int crop, int flip,
                                                           double s0, double s1, double r0, double r1,
                                                           int32_t* __restrict__ boxes) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int H = geom[4 * b + 1], W = geom[4 * b + 2];
    const uint32_t id = (uint32_t)ids[b];
    int top = 0, left = 0, h = H, w = W, att = -1;
    uint32_t x[4];
    if (crop && H > 0 && W > 0) {
        const double l0 = log(r0), l1 = log(r1);
        for (att = 0; att < kAttempts; ++att) {
            philox4x32_10(id, epoch, (uint32_t)att, kTag, k0, k1, x);
            const double area = (double)H * (double)W * (s0 + unit(x[0]) * (s1 - s0));
            const double asp = exp(l0 + unit(x[1]) * (l1 - l0));
            const double wd = floor(sqrt(area * asp) + 0.5), hd = floor(sqrt(area / asp) + 0.5);
            if (wd > 0.0 && wd <= (double)W && hd > 0.0 && hd <= (double)H) {
                w = (int)wd, h = (int)hd;
                top = min((int)floor(unit(x[2]) * (double)(H - h + 1)), H - h);
                left = min((int)floor(unit(x[3]) * (double)(W - w + 1)), W - w);
                break;
            }
        }
        if (att == kAttempts) {                                          // the central fallback
            const double ratio = (double)W / (double)H;
            if (ratio < r0) w = W, h = (int)floor((double)w / r0 + 0.5);
            else if (ratio > r1) h = H, w = (int)floor((double)h * r1 + 0.5);
            else h = H, w = W;
            h = min(max(h, 1), H), w = min(max(w, 1), W);
            top = (H - h) / 2, left = (W - w) / 2;
        }
    }
    int f = 0;
    if (flip) {
        philox4x32_10(id, epoch, (uint32_t)kAttempts, kTag, k0, k1, x);
        f = unit(x[0]) < 0.5;
    }
    int32_t* o = boxes + 8 * (size_t)b;
    o[0] = top, o[1] = left, o[2] = h, o[3] = w, o[4] = f, o[5] = att, o[6] = 0, o[7] = 0;
}

// Pillow's two filters (src/libImaging/Resample.c): the triangle, and Keys' cubic with a = -0.5
__host__ __device__ __forceinline__ double filter_w(double x, int cubic) {
    x = fabs(x);
    if (!cubic) return x < 1.0 ? 1.0 - x : 0.0;
    if (x < 1.0) return ((-0.5 + 2.0) * x - (-0.5 + 3.0)) * x * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5;
    return 0.0;
}

// Taps one output of an axis of extent n can have: Pillow's ksize, 2 ceil(support) + 1.  Monotone in n.
__host__ __device__ __forceinline__ int tap_bound(int n, int R, int cubic) {
    const double scale = (double)n / (double)R;
    const double half = ceil((cubic ? 2.0 : 1.0) * (scale > 1.0 ? scale : 1.0));
    return half < 1e6 ? 2 * (int)half + 1 : 2000001;
}

// Output o of an axis box extent n -> R: first tap, and the weights (evaluated and normalised in double, rounded once)
// zero-padded to `taps`, stored `stride` floats apart.
__device__ __forceinline__ int build_taps(int o, int n, int R, int cubic, int taps, float* w, int stride) {
    const double scale = (double)n / (double)R, fs = scale > 1.0 ? scale : 1.0, support = (cubic ? 2.0 : 1.0) * fs;
    const double c = ((double)o + 0.5) * scale;
    const int x0 = max(0, (int)(c - support + 0.5));
    const int cnt = min(min(n, (int)(c + support + 0.5)) - x0, taps);
    double sum = 0.0;
    for (int k = 0; k < cnt; ++k) sum += filter_w(((double)(x0 + k) + 0.5 - c) / fs, cubic);
    const double inv = sum != 0.0 ? 1.0 / sum : 1.0;
    for (int k = 0; k < taps; ++k)
        w[(size_t)k * stride] = k < cnt ? (float)(filter_w(((double)(x0 + k) + 0.5 - c) / fs, cubic) * inv) : 0.f;
    return x0;
}

// One block = one plane and one strip of its output rows.  The block builds the horizontal table of its sample's box (all R
// columns, tap-major so that a thread's four columns are one 16-byte LDS read) and the vertical table of its own rows, then
// each thread forms 4 adjacent output columns of one row: per source row the horizontal taps in ascending order, then the
// vertical taps in ascending order - Pillow's two passes, element by element, without the intermediate image.  A padded tap
// has weight zero and a clamped source index: it adds an exact zero.  A box that is not inside its plane, or that needs more
// than T taps, is never resampled: its outputs are NaN.
__global__ __launch_bounds__(256) void crop_resize_u8_kernel(const uint8_t* __restrict__ pix, const int32_t* __restrict__ geom,
                                                             const int32_t* __restrict__ boxes, float* __restrict__ dst, int C1,
                                                             int rep, int R, int cubic, int T) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int plane = blockIdx.x / kStrips, strip = blockIdx.x % kStrips;
    const int b = plane / C1, ch = plane % C1;
    const int off = geom[4 * b], H = geom[4 * b + 1], W = geom[4 * b + 2];
    const int32_t* box = boxes + 8 * (size_t)b;
    const int top = box[0], left = box[1], h = box[2], w = box[3], flip = box[4];
    const int rows = (R + kStrips - 1) / kStrips;
    const int r0 = strip * rows, r1 = min(R, r0 + rows);
    const int q4 = R >> 2;
    float* out = dst + (size_t)plane * rep * R * R;

    bool ok = off >= 0 && H > 0 && W > 0 && top >= 0 && left >= 0 && h > 0 && w > 0 && h <= H - top && w <= W - left;
    const int Ty = ok ? tap_bound(h, R, cubic) : 0, Tx = ok ? tap_bound(w, R, cubic) : 0;
    ok = ok && Ty <= T && Tx <= T;                                       // (uniform over the block)
    if (!ok) {
        const float nan = __builtin_nanf("");
        const f32x4 o = {nan, nan, nan, nan};
        for (int q = threadIdx.x; q < (r1 - r0) * q4; q += 256) {
            float* p = out + (size_t)(r0 + q / q4) * R + (q % q4) * 4;
            for (int k = 0; k < rep; ++k) *reinterpret_cast<f32x4*>(p + (size_t)k * R * R) = o;
        }
        return;
    }

    int32_t* sx = reinterpret_cast<int32_t*>(smem);                      // [R]
    float* wx = reinterpret_cast<float*>(smem) + R;                      // [Tx][R]
    int32_t* sy = reinterpret_cast<int32_t*>(wx + (size_t)T * R);        // [rows]
    float* wy = reinterpret_cast<float*>(sy + rows);                     // [rows][Ty]
    for (int i = threadIdx.x; i < R + (r1 - r0); i += 256) {
        if (i < R) sx[i] = build_taps(i, w, R, cubic, Tx, wx + i, R);
        else sy[i - R] = build_taps(r0 + i - R, h, R, cubic, Ty, wy + (size_t)(i - R) * Ty, 1);
    }
    __syncthreads();

    const uint8_t* src = pix + (size_t)off + (size_t)ch * H * W + (size_t)top * W + left;
    for (int q = threadIdx.x; q < (r1 - r0) * q4; q += 256) {
        const int rr = q / q4, c = (q % q4) * 4;
        const int cs = flip ? R - 4 - c : c;                             // the four unflipped columns, ascending
        const int y0 = sy[rr];
        const float* wyr = wy + (size_t)rr * Ty;
        int x0[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) x0[j] = sx[cs + j];
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int ty = 0; ty < Ty; ++ty) {
            const uint8_t* row = src + (size_t)min(y0 + ty, h - 1) * W;
            f32x4 hs = {0.f, 0.f, 0.f, 0.f};
            for (int tx = 0; tx < Tx; ++tx) {
                const f32x4 w4 = *reinterpret_cast<const f32x4*>(wx + (size_t)tx * R + cs);
#pragma unroll
                for (int j = 0; j < 4; ++j) hs[j] += w4[j] * (float)row[min(x0[j] + tx, w - 1)];
            }
            const float wv = wyr[ty];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += wv * hs[j];
        }
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fminf(fmaxf(flip ? acc[3 - j] : acc[j], 0.f), 255.f);
        float* p = out + (size_t)(r0 + rr) * R + c;
        for (int k = 0; k < rep; ++k) *reinterpret_cast<f32x4*>(p + (size_t)k * R * R) = o;
    }
}

// bytes of the two tables of a block at T taps
inline long long table_bytes(int R, int T) { return 4ll * (R + (R + kStrips - 1) / kStrips) * (T + 1); }

}  // namespace

extern "C" int ffm_augment_taps(int n, int R, int filter) {
    if (n <= 0 || R <= 0 || (filter != FFM_FILTER_BILINEAR && filter != FFM_FILTER_BICUBIC)) return FFM_EINVAL;
    const int T = tap_bound(n, R, filter == FFM_FILTER_BICUBIC);
    if (T > FFM_AUGMENT_MAX_TAPS || table_bytes(R, T) > FFM_AUGMENT_MAX_LDS) return FFM_EUNSUP;
    return T;
}

extern "C" int ffm_augment_boxes(const int32_t* geom, const int32_t* ids, int B, int64_t seed, int epoch, int crop, int flip,
                                 const double* range, int32_t* boxes, void* stream) {
    if (!geom || !ids || !range || !boxes || B <= 0 || epoch < 0) return FFM_EINVAL;
    if (((uintptr_t)geom & 3) || ((uintptr_t)ids & 3) || ((uintptr_t)boxes & 3)) return FFM_EINVAL;
    const double s0 = range[0], s1 = range[1], r0 = range[2], r1 = range[3];
    if (!(0.0 < s0 && s0 <= s1 && s1 <= 1.0) || !(0.0 < r0 && r0 <= r1) || !(r1 < 1e300)) return FFM_EINVAL;
    hipLaunchKernelGGL(augment_boxes_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, geom, ids, B,
                       (uint32_t)(uint64_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint32_t)epoch, crop != 0, flip != 0, s0, s1,
                       r0, r1, boxes);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}

extern "C" int ffm_crop_resize_u8(const uint8_t* pix, const int32_t* geom, const int32_t* boxes, float* dst, int B, int C1,
                                  int rep, int R, int filter, int max_extent, void* stream) {
    if (!pix || !geom || !boxes || !dst || B <= 0 || C1 <= 0 || rep <= 0 || R <= 0 || max_extent <= 0) return FFM_EINVAL;
    if (filter != FFM_FILTER_BILINEAR && filter != FFM_FILTER_BICUBIC) return FFM_EINVAL;
    if (((uintptr_t)geom & 3) || ((uintptr_t)boxes & 3) || ((uintptr_t)dst & 15)) return FFM_EINVAL;
    if (R % 4 || (long long)B * C1 > (1ll << 27)) return FFM_EUNSUP;
    const int T = ffm_augment_taps(max_extent, R, filter);
    if (T < 0) return FFM_EUNSUP;
    hipLaunchKernelGGL(crop_resize_u8_kernel, dim3((unsigned)(B * C1 * kStrips)), dim3(256), (size_t)table_bytes(R, T),
                       (hipStream_t)stream, pix, geom, boxes, dst, C1, rep, R, filter == FFM_FILTER_BICUBIC, T);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}
