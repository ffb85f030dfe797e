// Pieces the evaluator files share (evalsort.hip, evalboot.hip): the slot layout of the count table, the order-preserving
// image of a score and the row a sample's attribute value selects.
#pragma once
#include "common.h"

namespace {

constexpr int EV_NPOS = 0, EV_NNEG = 1, EV_WIN1 = 2, EV_TIE1 = 3, EV_WIN0 = 4, EV_TIE0 = 5, EV_TP = 6, EV_FP = 7, EV_TN = 8,
              EV_FN = 9;
constexpr int EV_SLOTS = FFM_EVAL_SLOTS;
typedef unsigned long long u64;

__device__ __forceinline__ uint32_t order_key(float f) {          // a < b  <=>  key(a) < key(b)  (no NaNs, no -0)
    const uint32_t u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ int group_slot(const int64_t* attr, int i, int G) {
    const int64_t a = attr ? attr[i] : -1;
    return (a >= 0 && a < G) ? (int)a : G;
}

// keys of one (column, scope): column c's score, scope group in the high word (0 for the 'all' scope)
__global__ __launch_bounds__(256) void eval_keys_kernel(const float* __restrict__ prob, const int64_t* __restrict__ attr, int N,
                                                        int G, int c, int grouped, u64* __restrict__ keys,
                                                        uint32_t* __restrict__ idx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const u64 hi = grouped ? (u64)group_slot(attr, i, G) : 0ull;
    keys[i] = (hi << 32) | order_key(prob[2 * (size_t)i + c]);
    idx[i] = (uint32_t)i;
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace
