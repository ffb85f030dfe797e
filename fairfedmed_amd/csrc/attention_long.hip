// Multi-head self-attention for sequences beyond one LDS image (L > 256), head_dim 64, MFMA 16x16: the key range is
// STREAMED through LDS in tiles of 64 keys, so LDS use does not depend on L.  fp32, bf16 and IEEE half storage from one
// template (no twin), with and without the causal mask.
//
// Orientation and fragment maps are those of the first-generation kernels (attention.hip): scores are computed
// transposed, S^T = K Q^T, a lane holds one query column (q = lane & 15) and 4 consecutive keys per 16-key fragment
// (key = 16 f + 4 (lane >> 4) + e), and that accumulator is directly the B operand of the next product, so P and dS never
// go through LDS.  The A side of those products needs the key (or query) index contiguous per lane: V / K / Q / dO are
// staged TRANSPOSED in LDS ([64 d][64 tokens], rows padded) next to the row-major swizzled images the score products read.
//
//   forward : one block per (b, h, 64-query tile), a wave per 16 queries.  Online softmax: running maximum m and running
//             sum l per query, the O accumulator rescaled by exp(m_old - m_new) whenever a tile raises the maximum.
//   backward: dQ kernel - one block per (b, h, 64-query tile), sweeps the key tiles; writes delta = rowsum(dO * O);
//             dK/dV kernel - one block per (b, h, 64-key tile), sweeps the query tiles; reads delta back.
//             P is recomputed from lse.  Every output element is summed by ONE wave in tile order: no sum across
//             workgroups, no atomics, no hand-off - the bits do not depend on the grid or on the batch size.
//
// Tiles are register-staged: the global loads of tile t + 1 are issued before the products of tile t and land in LDS
// behind the next barrier; the compiler places the waits.  Under the causal mask tiles wholly above the diagonal are
// never loaded (the 64-query and 64-key tiles are aligned: query tile j meets key tiles 0..j).
// Rows >= L of every tile are staged as zeros: finite, and always multiplied by an exactly zero probability.
#include "common.h"
#include <type_traits>

namespace {

constexpr int HD = 64;
constexpr int KT = 64;               // keys (or queries) per streamed tile
constexpr int NW = 4;                // waves per block, 16 resident queries (keys) each
constexpr int QT = 16 * NW;          // resident tile of a block; == KT (the causal tile bounds rely on it)
constexpr int NTH = 64 * NW;
static_assert(QT == KT, "causal tile skipping assumes aligned square tiles");

template <typename T> struct AL;     // per-dtype helpers
#define FFM_AL16(T16, X8, X4, MFMA)                                                                                   \
    template <> struct AL<T16> {                                                                                      \
        typedef X8 frag_t;                                                                                            \
        static constexpr int ES = 2, ROWB = 128, NCH = 8, ND = 2, CE = 8;                                             \
        static constexpr int FPK = 2; /* 16-token fragments per second-product k-step */                              \
        static __device__ __forceinline__ void mma(f32x4& acc, const frag_t& a, const frag_t& b) {                    \
            acc = MFMA(a, b, acc, 0, 0, 0);                                                                           \
        }                                                                                                             \
        static __device__ __forceinline__ frag_t pack(const f32x4* p) {                                               \
            const f32x4 a = p[0], b = p[1];                                                                           \
            frag_t r = {(T16)a[0], (T16)a[1], (T16)a[2], (T16)a[3], (T16)b[0], (T16)b[1], (T16)b[2], (T16)b[3]};      \
            return r;                                                                                                 \
        }                                                                                                             \
        /* A fragment of a transposed tile Xt[d][token] for k-step s: tokens 32 s + 16 (j >> 2) + 4 g + (j & 3) */    \
        static __device__ __forceinline__ frag_t tfrag(const T16* xt, int ts, int d, int s, int g) {                  \
            const X4 lo = *reinterpret_cast<const X4*>(xt + d * ts + 32 * s + 4 * g);                                 \
            const X4 hi = *reinterpret_cast<const X4*>(xt + d * ts + 32 * s + 16 + 4 * g);                            \
            frag_t r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};                                      \
            return r;                                                                                                 \
        }                                                                                                             \
        static __device__ __forceinline__ void store4(T16* p, f32x4 v) {                                              \
            X4 r = {(T16)v[0], (T16)v[1], (T16)v[2], (T16)v[3]};                                                      \
            *reinterpret_cast<X4*>(p) = r;                                                                            \
        }                                                                                                             \
    };
FFM_AL16(bf16_t, bf16x8, bf16x4, __builtin_amdgcn_mfma_f32_16x16x32_bf16)
FFM_AL16(f16_t, f16x8, f16x4, __builtin_amdgcn_mfma_f32_16x16x32_f16)
#undef FFM_AL16
template <> struct AL<float> {
    typedef f32x4 frag_t;
    static constexpr int ES = 4, ROWB = 256, NCH = 16, ND = 4, CE = 4;
    static constexpr int FPK = 1;
    // MFMA number e consumes element e of both lanes' fragments: which physical k that is does not matter (common.h)
    static __device__ __forceinline__ void mma(f32x4& acc, const frag_t& a, const frag_t& b) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], acc, 0, 0, 0);
    }
    static __device__ __forceinline__ frag_t pack(const f32x4* p) { return p[0]; }
    static __device__ __forceinline__ frag_t tfrag(const float* xt, int ts, int d, int s, int g) {
        return *reinterpret_cast<const f32x4*>(xt + d * ts + 16 * s + 4 * g);
    }
    static __device__ __forceinline__ void store4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
};

// element stride of a transposed tile row: 64 tokens + 16 B (rows 16 B apart modulo 32 B keep the 16-row fragment
// reads off each other's banks)
template <typename T> constexpr int tstride() { return (KT * AL<T>::ES + 16) / AL<T>::ES; }
template <typename T> constexpr int rm_bytes() { return KT * AL<T>::ROWB; }                 // row-major image
template <typename T> constexpr int tr_bytes() { return HD * tstride<T>() * AL<T>::ES; }    // transposed image

// swizzled byte offset of 16-B chunk `c` of row `row` in a row-major [64][64] LDS tile
template <typename T> __device__ __forceinline__ int rm_off(int row, int c) {
    return row * AL<T>::ROWB + ((c ^ (row & (AL<T>::NCH - 1))) << 4);
}

// One 64-token tile on its way global -> registers -> LDS.  Two thread maps:
//   rows  : consecutive threads take the chunks of one row (whole 128 / 256 B rows per 8 / 16 lanes) - row-major image only
//   tokens: consecutive threads take consecutive tokens, chunks outer - conflict-free 2- and 4-byte stores into the
//           transposed image; the same registers also feed the row-major image where a kernel needs both
template <typename T> struct Tile {
    typedef typename AL<T>::frag_t frag_t;
    static constexpr int TOTAL = KT * AL<T>::NCH, NIT = TOTAL / NTH;
    static_assert(TOTAL % NTH == 0, "whole passes");
    frag_t buf[NIT];

    template <bool BY_TOKEN> static __device__ __forceinline__ void where(int idx, int& row, int& c) {
        if (BY_TOKEN) { c = idx / KT; row = idx % KT; }
        else { row = idx / AL<T>::NCH; c = idx % AL<T>::NCH; }
    }
    // rows [0, nvalid) of src (first row of the tile, row stride ld); the others are zero
    template <bool BY_TOKEN> __device__ __forceinline__ void load(const T* __restrict__ src, int ld, int nvalid, int tid) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            int row, c;
            where<BY_TOKEN>(tid + it * NTH, row, c);
#pragma unroll
            for (int e = 0; e < AL<T>::CE; ++e) buf[it][e] = (T)0.f;
            if (row < nvalid) buf[it] = *reinterpret_cast<const frag_t*>(src + (size_t)row * ld + c * AL<T>::CE);
        }
    }
    template <bool BY_TOKEN> __device__ __forceinline__ void store_rowmajor(char* dst, int tid) const {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            int row, c;
            where<BY_TOKEN>(tid + it * NTH, row, c);
            *reinterpret_cast<frag_t*>(dst + rm_off<T>(row, c)) = buf[it];
        }
    }
    __device__ __forceinline__ void store_transposed(T* dst, int tid) const {     // token map only
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            int row, c;
            where<true>(tid + it * NTH, row, c);
#pragma unroll
            for (int e = 0; e < AL<T>::CE; ++e) dst[(c * AL<T>::CE + e) * tstride<T>() + row] = buf[it][e];
        }
    }
};

// 16-B operand fragment of row `row` (clamped to the sequence) straight from global memory
template <typename T>
__device__ __forceinline__ typename AL<T>::frag_t gfrag(const T* __restrict__ src, int ld, int row, int L, int ks, int g) {
    const int r = row < L ? row : L - 1;
    return *reinterpret_cast<const typename AL<T>::frag_t*>(src + (size_t)r * ld + (ks * 4 + g) * AL<T>::CE);
}
template <typename T>
__device__ __forceinline__ typename AL<T>::frag_t lfrag(const char* tile, int row, int ks, int g) {
    return *reinterpret_cast<const typename AL<T>::frag_t*>(tile + rm_off<T>(row, ks * 4 + g));
}

__device__ __forceinline__ float group4_max(float v) {   // lanes l, l^16, l^32, l^48 share a column
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
// IEEE half only (docs/experiments.md E15).  dS = P (dP - delta) / 8 goes to the matrix cores rounded to the storage type; it
// is linear in the incoming gradient and carries P ~ 1 / L, so in half it is subnormal from |dO| ~ 2^-12 down (fp16 mode:
// dO sits at 2^-10 rms at the default scale).  The wave's N fragments of one product step are scaled by the power of two that
// puts their largest |.| into [2^4, 2^5) - returned; `inv` its inverse, which the product's fp32 result takes.  Exact both
// ways; the exponent is clamped so that both factors are normal floats whatever the maximum is (0, infinite, subnormal).
template <int N> __device__ __forceinline__ float wave_pow2(const f32x4* d, float& inv) {
    float m = 0.f;
#pragma unroll
    for (int ff = 0; ff < N; ++ff)
#pragma unroll
        for (int e = 0; e < 4; ++e) m = fmaxf(m, fabsf(d[ff][e]));
#pragma unroll
    for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    int ex = m > 0.f ? ilogbf(m) : 0;
    ex = ex < -100 ? -100 : ex > 100 ? 100 : ex;
    inv = ldexpf(1.f, ex - 4);
    return ldexpf(1.f, 4 - ex);
}

__device__ __forceinline__ float group4_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// (b, h) pair and tile of a block; tiles of one pair are consecutive block ids
struct Unit { int b, h, tile; };
__device__ __forceinline__ Unit unit_of_block(int ntiles, int heads) {
    const int bid = blockIdx.x, bh = bid / ntiles;
    return {bh / heads, bh % heads, bid % ntiles};
}
// streamed tiles [first, end) that a resident tile meets (aligned 64-token tiles)
__device__ __forceinline__ int ntiles_of(int L) { return (L + KT - 1) / KT; }

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(NTH) void al_fwd_kernel(const T* __restrict__ qkv, T* __restrict__ out, float* __restrict__ lse, int L,
                                                     int heads, int causal) {
    typedef typename AL<T>::frag_t frag_t;
    extern __shared__ __attribute__((aligned(128))) char smem[];
    char* Ks = smem;                                              // [64][64] swizzled
    T* Vt = reinterpret_cast<T*>(smem + rm_bytes<T>());           // [64 d][ts]
    constexpr int ts = tstride<T>();

    const Unit u = unit_of_block(ntiles_of(L), heads);
    const int E = heads * HD, ld = 3 * E;
    const T* base = qkv + (size_t)u.b * L * ld + u.h * HD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int q0 = u.tile * QT, qw = q0 + wave * 16, q = qw + col;
    const int nkt = causal ? u.tile + 1 : ntiles_of(L);           // key tiles wholly above the diagonal are skipped

    frag_t qf[AL<T>::ND];
#pragma unroll
    for (int ks = 0; ks < AL<T>::ND; ++ks) qf[ks] = gfrag<T>(base, ld, q, L, ks, g);

    float m = -INFINITY, l = 0.f;                                 // running maximum and sum of this lane's query
    f32x4 o[4];
#pragma unroll
    for (int fd = 0; fd < 4; ++fd) o[fd] = (f32x4){0.f, 0.f, 0.f, 0.f};

    Tile<T> kr, vr;
    kr.template load<false>(base + E, ld, L, tid);
    vr.template load<true>(base + 2 * E, ld, L, tid);
    for (int kt = 0; kt < nkt; ++kt) {
        const int k0 = kt * KT;
        __syncthreads();                                          // the previous tile's readers are done
        kr.template store_rowmajor<false>(Ks, tid);
        vr.store_transposed(Vt, tid);
        __syncthreads();
        if (kt + 1 < nkt) {                                       // in flight while this tile multiplies
            kr.template load<false>(base + E + (size_t)(k0 + KT) * ld, ld, L - k0 - KT, tid);
            vr.template load<true>(base + 2 * E + (size_t)(k0 + KT) * ld, ld, L - k0 - KT, tid);
        }
        // a wave whose queries all lie beyond L, or (mask) all before this tile's first key, has nothing to add
        if (qw >= L || (causal && k0 > qw + 15)) continue;

        f32x4 s[4];
        float mx = -INFINITY;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < AL<T>::ND; ++ks) AL<T>::mma(acc, lfrag<T>(Ks, f * 16 + col, ks, g), qf[ks]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int key = k0 + f * 16 + g * 4 + e;
                float v = acc[e] * 0.125f;
                if (key >= L || (causal && key > q)) v = -INFINITY;
                acc[e] = v;
                mx = fmaxf(mx, v);
            }
            s[f] = acc;
        }
        // every processed tile holds an unmasked key for every live query (tile 0 holds key 0), so mn is finite from the
        // first tile on and alpha = exp(-inf) = 0 exactly there
        const float mn = fmaxf(m, group4_max(mx));
        const float alpha = fast_expf(m - mn);
        m = mn;
        float sum = 0.f;
#pragma unroll
        for (int f = 0; f < 4; ++f)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float p = fast_expf(s[f][e] - mn);
                s[f][e] = p;
                sum += p;
            }
        l = l * alpha + group4_sum(sum);
#pragma unroll
        for (int fd = 0; fd < 4; ++fd)
#pragma unroll
            for (int e = 0; e < 4; ++e) o[fd][e] *= alpha;
        constexpr int FPK = AL<T>::FPK;
#pragma unroll
        for (int st = 0; st < 4 / FPK; ++st) {
            const frag_t pf = AL<T>::pack(s + st * FPK);
#pragma unroll
            for (int fd = 0; fd < 4; ++fd) AL<T>::mma(o[fd], AL<T>::tfrag(Vt, ts, fd * 16 + col, st, g), pf);
        }
    }
    if (q < L) {
        const float inv = 1.0f / l;
        T* orow = out + ((size_t)u.b * L + q) * E + u.h * HD;
#pragma unroll
        for (int fd = 0; fd < 4; ++fd) {
            f32x4 v = o[fd];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= inv;
            AL<T>::store4(orow + fd * 16 + g * 4, v);
        }
        if (g == 0 && lse) lse[((size_t)u.b * heads + u.h) * L + q] = m + __logf(l);
    }
}

// ---------------------------------------------------------------------------
// backward, dQ: dS^T[key][q] = P^T * (dP^T - delta[q]) * scale,  dQ^T[d][q] = sum_key Kt[d][key] dS^T[key][q].
// Also writes delta[q] = sum_d dO[q][d] O[q][d] for the dK/dV kernel.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(NTH) void al_bwd_dq_kernel(const T* __restrict__ qkv, const T* __restrict__ d_o,
                                                        const float* __restrict__ lse, const T* __restrict__ o_fwd,
                                                        T* __restrict__ dqkv, float* __restrict__ delta, int L, int heads,
                                                        int causal) {
    typedef typename AL<T>::frag_t frag_t;
    extern __shared__ __attribute__((aligned(128))) char smem[];
    T* Kt = reinterpret_cast<T*>(smem);                           // [64 d][ts]
    char* Ks = smem + tr_bytes<T>();                              // [64][64] swizzled
    char* Vs = Ks + rm_bytes<T>();
    constexpr int ts = tstride<T>();

    const Unit u = unit_of_block(ntiles_of(L), heads);
    const int E = heads * HD, ld = 3 * E;
    const T* base = qkv + (size_t)u.b * L * ld + u.h * HD;
    const T* dob = d_o + (size_t)u.b * L * E + u.h * HD;
    const T* ob = o_fwd + (size_t)u.b * L * E + u.h * HD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int q0 = u.tile * QT, qw = q0 + wave * 16, q = qw + col;
    const int nkt = causal ? u.tile + 1 : ntiles_of(L);

    frag_t qf[AL<T>::ND], dof[AL<T>::ND];
    float dl = 0.f;
#pragma unroll
    for (int ks = 0; ks < AL<T>::ND; ++ks) {
        qf[ks] = gfrag<T>(base, ld, q, L, ks, g);
        dof[ks] = gfrag<T>(dob, E, q, L, ks, g);
        // the lane holds 16 of the 64 dO values of its query; the four lane groups of the column cover the row
        const frag_t of = gfrag<T>(ob, E, q, L, ks, g);
#pragma unroll
        for (int e = 0; e < AL<T>::CE; ++e) dl += (float)of[e] * (float)dof[ks][e];
    }
    dl = group4_sum(dl);
    const size_t rowc = ((size_t)u.b * heads + u.h) * L;
    const float lq = lse[rowc + (q < L ? q : L - 1)];
    if (g == 0 && q < L) delta[rowc + q] = dl;

    f32x4 dq[4];
#pragma unroll
    for (int fd = 0; fd < 4; ++fd) dq[fd] = (f32x4){0.f, 0.f, 0.f, 0.f};

    Tile<T> kr, vr;
    kr.template load<true>(base + E, ld, L, tid);
    vr.template load<false>(base + 2 * E, ld, L, tid);
    for (int kt = 0; kt < nkt; ++kt) {
        const int k0 = kt * KT;
        __syncthreads();
        kr.store_transposed(Kt, tid);
        kr.template store_rowmajor<true>(Ks, tid);
        vr.template store_rowmajor<false>(Vs, tid);
        __syncthreads();
        if (kt + 1 < nkt) {
            kr.template load<true>(base + E + (size_t)(k0 + KT) * ld, ld, L - k0 - KT, tid);
            vr.template load<false>(base + 2 * E + (size_t)(k0 + KT) * ld, ld, L - k0 - KT, tid);
        }
        if (qw >= L || (causal && k0 > qw + 15)) continue;

        constexpr int FPK = AL<T>::FPK;
#pragma unroll
        for (int st = 0; st < 4 / FPK; ++st) {
            f32x4 d2[FPK];
#pragma unroll
            for (int ff = 0; ff < FPK; ++ff) {
                const int f = st * FPK + ff;
                f32x4 sa = {0.f, 0.f, 0.f, 0.f}, pa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < AL<T>::ND; ++ks) {
                    AL<T>::mma(sa, lfrag<T>(Ks, f * 16 + col, ks, g), qf[ks]);
                    AL<T>::mma(pa, lfrag<T>(Vs, f * 16 + col, ks, g), dof[ks]);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int key = k0 + f * 16 + g * 4 + e;
                    float v = 0.f;
                    if (key < L && !(causal && key > q)) {
                        const float p = fast_expf(sa[e] * 0.125f - lq);
                        v = p * (pa[e] - dl) * 0.125f;
                    }
                    sa[e] = v;
                }
                d2[ff] = sa;
            }
            if constexpr (std::is_same<T, f16_t>::value) {
                float inv;
                const float up = wave_pow2<FPK>(d2, inv);
#pragma unroll
                for (int ff = 0; ff < FPK; ++ff)
#pragma unroll
                    for (int e = 0; e < 4; ++e) d2[ff][e] *= up;
                const frag_t df = AL<T>::pack(d2);
#pragma unroll
                for (int fd = 0; fd < 4; ++fd) {
                    f32x4 part = {0.f, 0.f, 0.f, 0.f};
                    AL<T>::mma(part, AL<T>::tfrag(Kt, ts, fd * 16 + col, st, g), df);
#pragma unroll
                    for (int e = 0; e < 4; ++e) dq[fd][e] += part[e] * inv;
                }
            } else {
            const frag_t df = AL<T>::pack(d2);
#pragma unroll
            for (int fd = 0; fd < 4; ++fd) AL<T>::mma(dq[fd], AL<T>::tfrag(Kt, ts, fd * 16 + col, st, g), df);
            }
        }
    }
    if (q < L) {
        T* drow = dqkv + ((size_t)u.b * L + q) * ld + u.h * HD;
#pragma unroll
        for (int fd = 0; fd < 4; ++fd) AL<T>::store4(drow + fd * 16 + g * 4, dq[fd]);
    }
}

// ---------------------------------------------------------------------------
// backward, dK/dV: waves own 16 keys; a lane holds key = lane & 15 and 4 consecutive queries per fragment.
// S[q][key] = Q K^T (A = Q rows), dP[q][key] = dO V^T,
// dV^T[d][key] = sum_q dOt[d][q] P[q][key],  dK^T[d][key] = sum_q Qt[d][q] dS[q][key].
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(NTH) void al_bwd_dkv_kernel(const T* __restrict__ qkv, const T* __restrict__ d_o,
                                                         const float* __restrict__ lse, const float* __restrict__ delta,
                                                         T* __restrict__ dqkv, int L, int heads, int causal) {
    typedef typename AL<T>::frag_t frag_t;
    extern __shared__ __attribute__((aligned(128))) char smem[];
    T* Qt = reinterpret_cast<T*>(smem);                           // [64 d][ts]
    T* dOt = reinterpret_cast<T*>(smem + tr_bytes<T>());
    char* Qs = smem + 2 * tr_bytes<T>();                          // [64][64] swizzled
    char* dOs = Qs + rm_bytes<T>();
    float* lse_s = reinterpret_cast<float*>(dOs + rm_bytes<T>()); // [64]
    float* del_s = lse_s + KT;                                    // [64]
    constexpr int ts = tstride<T>();

    const int nqt = ntiles_of(L);
    const Unit u = unit_of_block(nqt, heads);
    const int E = heads * HD, ld = 3 * E;
    const T* base = qkv + (size_t)u.b * L * ld + u.h * HD;
    const T* dob = d_o + (size_t)u.b * L * E + u.h * HD;
    const size_t rowc = ((size_t)u.b * heads + u.h) * L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int kw = u.tile * KT + wave * 16, key = kw + col;
    const int qt0 = causal ? u.tile : 0;                          // query tiles wholly before the key tile are skipped

    frag_t kf[AL<T>::ND], vf[AL<T>::ND];
#pragma unroll
    for (int ks = 0; ks < AL<T>::ND; ++ks) {
        kf[ks] = gfrag<T>(base + E, ld, key, L, ks, g);
        vf[ks] = gfrag<T>(base + 2 * E, ld, key, L, ks, g);
    }
    f32x4 dv[4], dk[4];
#pragma unroll
    for (int fd = 0; fd < 4; ++fd) { dv[fd] = (f32x4){0.f, 0.f, 0.f, 0.f}; dk[fd] = (f32x4){0.f, 0.f, 0.f, 0.f}; }

    Tile<T> qr, dr;
    float lr = 0.f, er = 0.f;                                     // row constants of the tile (threads 0..63)
    auto load_tile = [&](int r0) {
        qr.template load<true>(base + (size_t)r0 * ld, ld, L - r0, tid);
        dr.template load<true>(dob + (size_t)r0 * E, E, L - r0, tid);
        lr = 0.f;
        er = 0.f;
        if (tid < KT && r0 + tid < L) {
            lr = lse[rowc + r0 + tid];
            er = delta[rowc + r0 + tid];
        }
    };
    load_tile(qt0 * KT);
    for (int qt = qt0; qt < nqt; ++qt) {
        const int r0 = qt * KT;
        __syncthreads();
        qr.store_transposed(Qt, tid);
        qr.template store_rowmajor<true>(Qs, tid);
        dr.store_transposed(dOt, tid);
        dr.template store_rowmajor<true>(dOs, tid);
        if (tid < KT) { lse_s[tid] = lr; del_s[tid] = er; }
        __syncthreads();
        if (qt + 1 < nqt) load_tile(r0 + KT);
        if (kw >= L) continue;                                    // (every query of a later tile is past a live key: no mask skip)

        constexpr int FPK = AL<T>::FPK;
#pragma unroll
        for (int st = 0; st < 4 / FPK; ++st) {
            f32x4 p2[FPK], d2[FPK];
#pragma unroll
            for (int ff = 0; ff < FPK; ++ff) {
                const int f = st * FPK + ff;
                f32x4 sa = {0.f, 0.f, 0.f, 0.f}, pa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < AL<T>::ND; ++ks) {
                    AL<T>::mma(sa, lfrag<T>(Qs, f * 16 + col, ks, g), kf[ks]);
                    AL<T>::mma(pa, lfrag<T>(dOs, f * 16 + col, ks, g), vf[ks]);
                }
                const int qb = f * 16 + g * 4;                    // this lane's 4 consecutive queries of the tile
                const f32x4 l4 = *reinterpret_cast<const f32x4*>(&lse_s[qb]);
                const f32x4 d4 = *reinterpret_cast<const f32x4*>(&del_s[qb]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int qq = r0 + qb + e;
                    float p = 0.f, d = 0.f;
                    if (qq < L && key < L && !(causal && key > qq)) {
                        p = fast_expf(sa[e] * 0.125f - l4[e]);
                        d = p * (pa[e] - d4[e]) * 0.125f;
                    }
                    sa[e] = p;
                    pa[e] = d;
                }
                p2[ff] = sa;
                d2[ff] = pa;
            }
            const frag_t pf = AL<T>::pack(p2);
            if constexpr (std::is_same<T, f16_t>::value) {
                float inv;
                const float up = wave_pow2<FPK>(d2, inv);
#pragma unroll
                for (int ff = 0; ff < FPK; ++ff)
#pragma unroll
                    for (int e = 0; e < 4; ++e) d2[ff][e] *= up;
                const frag_t df = AL<T>::pack(d2);
#pragma unroll
                for (int fd = 0; fd < 4; ++fd) {
                    AL<T>::mma(dv[fd], AL<T>::tfrag(dOt, ts, fd * 16 + col, st, g), pf);
                    f32x4 part = {0.f, 0.f, 0.f, 0.f};
                    AL<T>::mma(part, AL<T>::tfrag(Qt, ts, fd * 16 + col, st, g), df);
#pragma unroll
                    for (int e = 0; e < 4; ++e) dk[fd][e] += part[e] * inv;
                }
            } else {
            const frag_t df = AL<T>::pack(d2);
#pragma unroll
            for (int fd = 0; fd < 4; ++fd) {
                AL<T>::mma(dv[fd], AL<T>::tfrag(dOt, ts, fd * 16 + col, st, g), pf);
                AL<T>::mma(dk[fd], AL<T>::tfrag(Qt, ts, fd * 16 + col, st, g), df);
            }
            }
        }
    }
    if (key < L) {
        T* drow = dqkv + ((size_t)u.b * L + key) * ld + u.h * HD;
#pragma unroll
        for (int fd = 0; fd < 4; ++fd) {
            AL<T>::store4(drow + E + fd * 16 + g * 4, dk[fd]);
            AL<T>::store4(drow + 2 * E + fd * 16 + g * 4, dv[fd]);
        }
    }
}

template <typename T> constexpr int lds_fwd() { return rm_bytes<T>() + tr_bytes<T>(); }
template <typename T> constexpr int lds_dq() { return tr_bytes<T>() + 2 * rm_bytes<T>(); }
template <typename T> constexpr int lds_dkv() { return 2 * tr_bytes<T>() + 2 * rm_bytes<T>() + 2 * KT * 4; }

// one block per (b, h, tile): FFM_EUNSUP when the grid's thread count does not fit 32 bits (HIP's limit per dimension)
inline bool grid_of(int B, int L, int heads, unsigned& blocks) {
    const long long n = (long long)B * heads * ((L + KT - 1) / KT);
    blocks = (unsigned)n;
    return n * NTH <= 0xffffffffLL;
}

template <typename T>
int run_fwd(const void* qkv, void* out, float* lse, int B, int L, int heads, int causal, hipStream_t s) {
    unsigned blocks;
    if (!grid_of(B, L, heads, blocks)) return FFM_EUNSUP;
    hipLaunchKernelGGL((al_fwd_kernel<T>), dim3(blocks), dim3(NTH), lds_fwd<T>(), s, (const T*)qkv, (T*)out, lse, L, heads, causal);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}
template <typename T>
int run_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv, int B, int L, int heads,
            int causal, hipStream_t s) {
    unsigned blocks;
    if (!grid_of(B, L, heads, blocks)) return FFM_EUNSUP;
    const int e = ffm_set_max_lds(al_bwd_dkv_kernel<T>, lds_dkv<T>());    // fp32: 68 096 B
    if (e) return e;
    hipLaunchKernelGGL((al_bwd_dq_kernel<T>), dim3(blocks), dim3(NTH), lds_dq<T>(), s, (const T*)qkv, (const T*)dout, lse, (const T*)out,
                       (T*)dqkv, delta, L, heads, causal);
    FFM_CHECK_LAUNCH();
    hipLaunchKernelGGL((al_bwd_dkv_kernel<T>), dim3(blocks), dim3(NTH), lds_dkv<T>(), s, (const T*)qkv, (const T*)dout, lse,
                       (const float*)delta, (T*)dqkv, L, heads, causal);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}

}  // namespace

// Entry points for attention.hip's dispatcher (same library, not part of the C ABI).  `dtype` is the caller's real code:
// this file is compiled once and serves the IEEE-half twin of the dispatcher too.
int ffm_attn_long_fwd(const void* qkv, void* out, float* lse, int B, int L, int heads, int causal, int dtype, hipStream_t s) {
    if (dtype == FFM_BF16) return run_fwd<bf16_t>(qkv, out, lse, B, L, heads, causal, s);
    if (dtype == FFM_F16) return run_fwd<f16_t>(qkv, out, lse, B, L, heads, causal, s);
    if (dtype == FFM_F32) return run_fwd<float>(qkv, out, lse, B, L, heads, causal, s);
    return FFM_EINVAL;
}
int ffm_attn_long_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv, int B, int L,
                      int heads, int causal, int dtype, hipStream_t s) {
    if (dtype == FFM_BF16) return run_bwd<bf16_t>(qkv, out, dout, lse, delta, dqkv, B, L, heads, causal, s);
    if (dtype == FFM_F16) return run_bwd<f16_t>(qkv, out, dout, lse, delta, dqkv, B, L, heads, causal, s);
    if (dtype == FFM_F32) return run_bwd<float>(qkv, out, dout, lse, delta, dqkv, B, L, heads, causal, s);
    return FFM_EINVAL;
}
