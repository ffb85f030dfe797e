// Bootstrap replicates of the evaluator's count table (ffm_eval_boot_counts): out[r] is the table
// ffm_eval_counts would produce for the test set resampled with replacement by replicate r, integer for integer.
//   once per call:      a code byte per sample (row, label, prediction); per probability column c and scope (all / own
//                       group) the sort of evalsort.hip, and per sorted position of a positive the three positions that
//                       no replicate moves: lower bound, upper bound and segment start of its key;
//   per chunk of replicates:
//     draw kernel       m[r][i] = multiplicity of sample i (Philox4x32-10 draws, integer atomics);
//     count kernel      one block per (replicate, column, scope): E = exclusive prefix of the negatives' multiplicities in
//                       sorted order (block-wide scan, running carry across tiles); a positive at sorted position s adds
//                       m (E[lb] - E[seg]) to its row's wins and m (E[ub] - E[lb]) to its ties.  The (column 1, group
//                       scope) block also sums the sample and confusion counts: its order visits the rows one by one.
// Prefix sums are at most N (32 bits); wins and ties are 64-bit.  Accumulators live in registers, then in LDS, then one
// 64-bit global atomic per block and slot: exact integers, independent of launch geometry and of `chunk`.
// The sort is rocPRIM's, as in evalsort.hip.  The caller provides the workspace (the library allocates nothing).
#include "common.h"
#include "evalkeys.h"
#include "philox.h"
#include <rocprim/device/device_radix_sort.hpp>

namespace {

constexpr int kThreads = 256;                 // four waves
constexpr int kItems = 4;                     // sorted positions per thread and tile of the scan
constexpr int kTile = kThreads * kItems;
constexpr int kMaxChunk = 65535;              // replicates of a chunk ride in gridDim.y
constexpr uint32_t kNegBit = 0x80000000u;     // sorted sample index: bit 31 = negative of this column
constexpr uint32_t kBootWord = 0x544F4F42u;   // fourth counter word of every bootstrap draw
constexpr int CODE_ROW = 15, CODE_IS1 = 16, CODE_IS0 = 32, CODE_PRED1 = 64;

// row | label == 1 | label == 0 | p1 > p0: all a replicate needs of a sample besides its place in the sorted orders
__global__ __launch_bounds__(kThreads) void boot_code_kernel(const float* __restrict__ prob, const int64_t* __restrict__ label,
                                                             const int64_t* __restrict__ attr, int N, int G,
                                                             uint8_t* __restrict__ code) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    const int64_t y = label[i];
    const float p0 = prob[2 * (size_t)i], p1 = prob[2 * (size_t)i + 1];
    code[i] = (uint8_t)(group_slot(attr, i, G) | (y == 1 ? CODE_IS1 : 0) | (y == 0 ? CODE_IS0 : 0) | (p1 > p0 ? CODE_PRED1 : 0));
}

// sorted order of one (column, scope): sample index with the negative flag; for a positive (label == c) the bounds of its
// key and the start of its group's segment (0 in the 'all' scope) - the searches of eval_count_kernel, done once
__global__ __launch_bounds__(kThreads) void boot_bounds_kernel(const u64* __restrict__ skeys, const uint32_t* __restrict__ sidx,
                                                               const uint8_t* __restrict__ code, int N, int c, int grouped,
                                                               uint32_t* __restrict__ sv, uint32_t* __restrict__ lbv,
                                                               uint32_t* __restrict__ ubv, uint32_t* __restrict__ segv) {
    const int s = blockIdx.x * kThreads + threadIdx.x;
    if (s >= N) return;
    const uint32_t i = sidx[s];
    const bool positive = code[i] & (c == 1 ? CODE_IS1 : CODE_IS0);
    sv[s] = i | (positive ? 0u : kNegBit);
    if (!positive) return;
    const u64 k = skeys[s];
    int lo = 0, hi = s;                                            // lower bound lies in [0, s]
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (skeys[mid] < k) lo = mid + 1; else hi = mid;
    }
    const int lb = lo;
    lo = s + 1;                                                    // upper bound lies in (s, N]
    hi = N;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (skeys[mid] <= k) lo = mid + 1; else hi = mid;
    }
    const int ub = lo;
    int a = 0;
    if (grouped) {
        const u64 seg = k & 0xFFFFFFFF00000000ull;
        int b = lb;
        while (a < b) {
            const int mid = a + ((b - a) >> 1);
            if (skeys[mid] < seg) a = mid + 1; else b = mid;
        }
    }
    lbv[s] = (uint32_t)lb;
    ubv[s] = (uint32_t)ub;
    segv[s] = (uint32_t)a;
}

// m[r][idx_k] += 1 for the draws k = 2q, 2q + 1 of replicate r0 + r (gridDim.y = replicates of the chunk)
__global__ __launch_bounds__(kThreads) void boot_draw_kernel(uint32_t* __restrict__ m, int N, uint32_t r0, uint32_t tag,
                                                             uint32_t k0, uint32_t k1) {
    const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= ((uint32_t)N + 1u) / 2u) return;
    uint32_t x[4];
    philox4x32_10(q, r0 + blockIdx.y, tag, kBootWord, k0, k1, x);
    uint32_t* mr = m + (size_t)blockIdx.y * (size_t)N;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (2u * q + h < (uint32_t)N) {
            const u64 x64 = (u64)x[2 * h] | ((u64)x[2 * h + 1] << 32);
            atomicAdd(&mr[__umul64hi(x64, (u64)N)], 1u);           // < N
        }
    }
}

// blockIdx.x = (column, scope): 0 (c = 1, all), 1 (c = 1, group), 2 (c = 0, all), 3 (c = 0, group); blockIdx.y = replicate
__global__ __launch_bounds__(kThreads) void boot_count_kernel(const uint32_t* __restrict__ sv_all, const uint32_t* __restrict__ lb_all,
                                                              const uint32_t* __restrict__ ub_all, const uint32_t* __restrict__ seg_all,
                                                              const uint8_t* __restrict__ code, const uint32_t* __restrict__ m_all,
                                                              uint32_t* E_all, int N, int G, u64* out) {
    __shared__ u64 acc[(FFM_MAX_GROUPS + 2) * EV_SLOTS];
    __shared__ uint32_t wsum[kThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x, c = p < 2 ? 1 : 0, grouped = p & 1;
    const bool basic = p == 1;
    const size_t r = blockIdx.y;
    const uint32_t* sv = sv_all + (size_t)p * N;
    const uint32_t* lbv = lb_all + (size_t)p * N;
    const uint32_t* ubv = ub_all + (size_t)p * N;
    const uint32_t* segv = seg_all + (size_t)p * N;
    const uint32_t* m = m_all + r * (size_t)N;
    uint32_t* E = E_all + (r * 4 + p) * ((size_t)N + 1);
    for (int k = tid; k < (G + 2) * EV_SLOTS; k += kThreads) acc[k] = 0;

    // E[s] = sum of m over the negatives at sorted positions < s; E[N] = all of them
    uint32_t carry = 0;
    for (int64_t base = 0; base < N; base += kTile) {
        const int64_t s0 = base + (int64_t)tid * kItems;
        uint32_t w[kItems], t = 0;
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            w[j] = 0;
            if (s0 + j < N) {
                const uint32_t v = sv[s0 + j];
                if (v & kNegBit) w[j] = m[v & ~kNegBit];
            }
            t += w[j];
        }
        uint32_t incl = t;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kThreads / 64; ++k) {
            if (k < wave) before += wsum[k];
            total += wsum[k];
        }
        uint32_t e = carry + before + incl - t;
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            if (s0 + j < N) E[s0 + j] = e;
            e += w[j];
        }
        carry += total;
        __syncthreads();                                           // wsum is rewritten by the next tile
    }
    if (tid == 0) E[N] = carry;
    __threadfence_block();
    __syncthreads();

    // the sorted order of the group scope visits one row after the other, so a thread keeps the sums of its current row in
    // registers and hands them to LDS when the row changes
    const int wslot = c == 1 ? EV_WIN1 : EV_WIN0;
    int cur = -1;
    u64 win = 0, tie = 0;
    uint32_t npos = 0, nneg = 0, tp = 0, fp = 0, tn = 0, fn = 0;
    auto flush = [&]() {
        if (cur >= 0) {
            u64* a = acc + cur * EV_SLOTS;
            if (win) atomicAdd(&a[wslot], win);
            if (tie) atomicAdd(&a[wslot + 1], tie);
            if (basic) {
                if (npos) atomicAdd(&a[EV_NPOS], (u64)npos);
                if (nneg) atomicAdd(&a[EV_NNEG], (u64)nneg);
                if (tp) atomicAdd(&a[EV_TP], (u64)tp);
                if (fp) atomicAdd(&a[EV_FP], (u64)fp);
                if (tn) atomicAdd(&a[EV_TN], (u64)tn);
                if (fn) atomicAdd(&a[EV_FN], (u64)fn);
            }
        }
        win = tie = 0;
        npos = nneg = tp = fp = tn = fn = 0;
    };
    for (int64_t s = tid; s < N; s += kThreads) {
        const uint32_t v = sv[s], i = v & ~kNegBit, mi = m[i];
        if (!mi) continue;
        const int cd = code[i];
        const int row = grouped ? (cd & CODE_ROW) : G + 1;
        if (row != cur) {
            flush();
            cur = row;
        }
        if (basic) {
            const bool pos = cd & CODE_IS1, pred1 = cd & CODE_PRED1;
            npos += pos ? mi : 0u;
            nneg += pos ? 0u : mi;
            tp += (pos && pred1) ? mi : 0u;
            fn += (pos && !pred1) ? mi : 0u;
            fp += (!pos && pred1) ? mi : 0u;
            tn += (!pos && !pred1) ? mi : 0u;
        }
        if (!(v & kNegBit)) {
            const uint32_t el = E[lbv[s]];
            win += (u64)mi * (u64)(el - E[segv[s]]);
            tie += (u64)mi * (u64)(E[ubv[s]] - el);
        }
    }
    flush();
    __syncthreads();
    if (basic) {                                                   // the 'all' row of the per-sample counts: sum of the rows
        if (tid < EV_SLOTS && (tid < EV_WIN1 || tid >= EV_TP)) {
            u64 t = 0;
            for (int g = 0; g <= G; ++g) t += acc[g * EV_SLOTS + tid];
            acc[(G + 1) * EV_SLOTS + tid] = t;
        }
        __syncthreads();
    }
    u64* o = out + r * (size_t)(G + 2) * EV_SLOTS;
    for (int k = tid; k < (G + 2) * EV_SLOTS; k += kThreads)
        if (acc[k]) atomicAdd(&o[k], acc[k]);
}

struct BootWs {
    u64 *k0, *k1;
    uint32_t *i0, *i1, *sv, *lb, *ub, *seg, *m, *E;
    uint8_t* code;
    void* temp;
    size_t temp_bytes, own, total;
};

// everything but rocPRIM's temporary storage, which comes last: `own` needs no library call
void plan_own(int N, int chunk, char* base, BootWs& w) {
    const size_t n = (size_t)N;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += align256(bytes); return p; };
    w.k0 = (u64*)take(sizeof(u64) * n);
    w.k1 = (u64*)take(sizeof(u64) * n);
    w.i0 = (uint32_t*)take(4 * n);
    w.i1 = (uint32_t*)take(4 * n);
    w.code = (uint8_t*)take(n);
    w.sv = (uint32_t*)take(4 * 4 * n);
    w.lb = (uint32_t*)take(4 * 4 * n);
    w.ub = (uint32_t*)take(4 * 4 * n);
    w.seg = (uint32_t*)take(4 * 4 * n);
    w.m = (uint32_t*)take(4 * (size_t)chunk * n);
    w.E = (uint32_t*)take(4 * (size_t)chunk * 4 * (n + 1));
    w.own = off;
    w.temp = base ? base + off : nullptr;
}

hipError_t plan_sort(int N, BootWs& w) {
    size_t sort_b = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_b, (u64*)nullptr, (u64*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                             (size_t)N, 0u, 36u, (hipStream_t)0);
    if (e != hipSuccess) return e;
    w.temp_bytes = sort_b;
    w.total = w.own + align256(sort_b);
    return hipSuccess;
}

}  // namespace

extern "C" int64_t ffm_eval_boot_ws_bytes(int N, int chunk) {
    if (N <= 0 || chunk <= 0 || chunk > kMaxChunk) return FFM_EINVAL;
    BootWs w;
    plan_own(N, chunk, nullptr, w);
    if (plan_sort(N, w) != hipSuccess) return FFM_EINVAL;
    return (int64_t)w.total;
}

extern "C" int ffm_eval_boot_counts(const float* prob, const int64_t* label, const int64_t* attr, int N, int G, int B, int chunk,
                                    int64_t seed, int tag, uint64_t* out, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
    if (!prob || !label || !out || !workspace || N <= 0 || B <= 0 || chunk <= 0 || G < 0 || G > FFM_MAX_GROUPS) return FFM_EINVAL;
    if (((uintptr_t)workspace & 255) || workspace_bytes <= 0) return FFM_EINVAL;
    if (chunk > kMaxChunk) return FFM_EUNSUP;
    BootWs w;
    plan_own(N, chunk, (char*)workspace, w);
    if ((int64_t)w.own > workspace_bytes) return FFM_EINVAL;       // short already without the sort's share: no library call
    hipError_t e = plan_sort(N, w);
    if (e != hipSuccess) return (int)e;
    if ((int64_t)w.total > workspace_bytes) return FFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const size_t table = (size_t)(G + 2) * EV_SLOTS;
    e = hipMemsetAsync(out, 0, sizeof(uint64_t) * table * (size_t)B, s);
    if (e != hipSuccess) return (int)e;
    const int nb = (int)(((int64_t)N + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(boot_code_kernel, dim3(nb), dim3(kThreads), 0, s, prob, label, attr, N, G, w.code);
    FFM_CHECK_LAUNCH();
    for (int p = 0; p < 4; ++p) {
        const int c = p < 2 ? 1 : 0, grouped = p & 1;
        hipLaunchKernelGGL(eval_keys_kernel, dim3(nb), dim3(256), 0, s, prob, attr, N, G, c, grouped, w.k0, w.i0);
        FFM_CHECK_LAUNCH();
        size_t tb = w.temp_bytes;
        e = rocprim::radix_sort_pairs(w.temp, tb, w.k0, w.k1, w.i0, w.i1, (size_t)N, 0u, grouped ? 36u : 32u, s);
        if (e != hipSuccess) return (int)e;
        const size_t o = (size_t)p * (size_t)N;
        hipLaunchKernelGGL(boot_bounds_kernel, dim3(nb), dim3(kThreads), 0, s, w.k1, w.i1, w.code, N, c, grouped, w.sv + o, w.lb + o,
                           w.ub + o, w.seg + o);
        FFM_CHECK_LAUNCH();
    }
    const uint32_t k0 = (uint32_t)(uint64_t)seed, k1 = (uint32_t)((uint64_t)seed >> 32);
    const int nq = (int)(((int64_t)N + 1) / 2);
    for (int r0 = 0; r0 < B; r0 += chunk) {
        const int nr = B - r0 < chunk ? B - r0 : chunk;
        e = hipMemsetAsync(w.m, 0, 4 * (size_t)nr * (size_t)N, s);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(boot_draw_kernel, dim3((nq + kThreads - 1) / kThreads, nr), dim3(kThreads), 0, s, w.m, N, (uint32_t)r0,
                           (uint32_t)tag, k0, k1);
        FFM_CHECK_LAUNCH();
        hipLaunchKernelGGL(boot_count_kernel, dim3(4, nr), dim3(kThreads), 0, s, w.sv, w.lb, w.ub, w.seg, w.code, w.m, w.E, N, G,
                           (u64*)out + (size_t)r0 * table);
        FFM_CHECK_LAUNCH();
    }
    return FFM_OK;
}
