// Flat-buffer parameter kernels: fused SGD-momentum over all trainable tensors,
// and the FedAvg round-boundary helpers.  All float32: no `dtype` argument, no half twin.
#include "common.h"

namespace {

// torch.optim.SGD, dampening 0, no nesterov (Dassl/dassl/optim/optimizer.py:105-113), `repeats` times on the SAME gradient:
// d = g + wd*p; b = (first application of a first step) ? d : mu*b + d; p -= lr*b.  Every SGD kernel below goes through
// this one function, with the roundings written out: left to contraction, the SLP vectoriser pairs mu*b with wd*p into
// one v_pk_mul_f32 (rounded apart from the adds) in some kernels and some repeats but not in others, and the eager step,
// its recorded plan and the captured graph must agree bit for bit.  The first application fuses both products into their
// sums, the later ones round products and sums separately: what ffm_sgd_momentum / _n / _gated have always computed.
__device__ __forceinline__ void sgd_update(float& pi, float& b, float gi, float lr, float mu, float wd, int first,
                                           int repeats) {
    const float d0 = fmaf(wd, pi, gi);
    b = first ? d0 : fmaf(mu, b, d0);
    pi = fmaf(-lr, b, pi);
    for (int k = 1; k < repeats; ++k) {
#pragma clang fp contract(off)
        const float d = gi + wd * pi;
        b = mu * b + d;
        pi = fmaf(-lr, b, pi);
    }
}

__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ buf, int64_t n, float lr, float mu, float wd,
                                                  int first) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float pi = p[i];
        float b = first ? 0.f : buf[i];
        sgd_update(pi, b, g[i], lr, mu, wd, first, 1);
        buf[i] = b;
        p[i] = pi;
    }
}

// `repeats` applications of the same update on the SAME gradient in one pass over memory: the reference registers
// 'prompt_learner' and 'image_encoder' with ONE optimizer (trainers/GLP_OT_SVLoRA.py:866-870) and Dassl's model_update
// steps every registered name (Dassl/dassl/engine/trainer.py:333-337), so optim.step() runs twice per batch.
__global__ __launch_bounds__(256) void sgd_n_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ buf, int64_t n, float lr, float mu, float wd,
                                                    int first, int repeats) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float pi = p[i];
        float b = first ? 0.f : buf[i];
        sgd_update(pi, b, g[i], lr, mu, wd, first, repeats);
        buf[i] = b;
        p[i] = pi;
    }
}

// same update with the hyper-parameters read from device memory (hp = {lr, momentum, weight_decay}),
// so that a captured hipGraph keeps working when the LR scheduler changes lr.  With a zero-initialised
// momentum buffer the general formula equals torch's first-step rule (mu*0 + d == d exactly).  st (may be NULL): the
// fp16 gradient-scale state; the update is skipped when st[2] == 0, as in sgd_gated_kernel.
__global__ __launch_bounds__(256) void sgd_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                      float* __restrict__ buf, int64_t n,
                                                      const float* __restrict__ hp, int repeats,
                                                      const float* __restrict__ st) {
    if (st && st[2] == 0.0f) return;              // the gradients overflowed: the step is skipped, momentum untouched
    const float lr = hp[0], mu = hp[1], wd = hp[2];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float pi = p[i];
        float b = buf[i];
        sgd_update(pi, b, g[i], lr, mu, wd, 0, repeats);
        buf[i] = b;
        p[i] = pi;
    }
}

__global__ __launch_bounds__(256) void scale_by_kernel(const float* __restrict__ p, const float* __restrict__ w,
                                                       float* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = p[i] * w[i];
}

// a rank that holds several clients of a round: acc += p (.) w, product and sum rounded separately (no FMA), as the
// reference's `w_avg[key] += w[idx][key] * weight` (utils/fed_utils.py:79-86) rounds them
__global__ __launch_bounds__(256) void scale_acc_kernel(const float* __restrict__ p, const float* __restrict__ w,
                                                        float* __restrict__ acc, int64_t n) {
#pragma clang fp contract(off)      // (hipcc contracts a * b + c into an FMA by default, and __fmul_rn is a plain product in HIP)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        acc[i] = acc[i] + p[i] * w[i];
}

// utils/fed_utils.py:88-98: optional shared_half_s, then EMA with the previous global
__global__ __launch_bounds__(256) void shared_half_kernel(float* __restrict__ avg, const int64_t* __restrict__ offs,
                                                          int n_s, int G, int r) {
    const int blk = blockIdx.x;
    if (blk >= n_s) return;
    float* s = avg + offs[blk];
    const int half = r / 2;
    for (int j = threadIdx.x; j < half; j += blockDim.x) {
        float m = 0.f;
        for (int g = 0; g < G; ++g) m += s[g * r + j];
        m /= (float)G;
        for (int g = 0; g < G; ++g) s[g * r + j] = m;
    }
}

// (prev and out may be the same buffer: the aggregator updates its global weights in place)
__global__ __launch_bounds__(256) void ema_kernel(const float* __restrict__ avg, const float* prev, float* out, int64_t n,
                                                  float beta) {
#pragma clang fp contract(off)      // three roundings, as `(1 - b) * avg + b * w_g` has in the reference (utils/fed_utils.py:98)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (1.0f - beta) * avg[i] + beta * prev[i];
}

inline int grid_for(int64_t n) {
    int64_t b = (n + 255) / 256;
    return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

// p *= s in place; *finite_flag = 0 if any product is not finite (the overflow guard of the IEEE-half mode's gradient scale)
__global__ __launch_bounds__(256) void scale_check_kernel(float* __restrict__ p, float sc, int64_t n, int32_t* __restrict__ finite_flag) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = p[i] * sc;
        p[i] = v;
        bad |= !(fabsf(v) <= 3.4028234e38f);
    }
    if (finite_flag && __any(bad) && (threadIdx.x & 63) == 0) *finite_flag = 0;
}

// IEEE-half mode, dynamic gradient scale held in DEVICE memory so that recorded launch plans / captured graphs stay valid
// while it changes: st = {scale, 1/scale, ok, good_run, overflows, max_scale, growth_interval, min_scale} (floats).
// A step is  loss_scale(dlogits) -> backward -> unscale_check(grad) -> sgd_gated -> scale_update.
__global__ __launch_bounds__(256) void loss_scale_kernel(float* __restrict__ p, int64_t n, float* __restrict__ st) {
    const float sc = st[0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] *= sc;
    // (ok is read by kernels behind this one in stream order only; every block has read st[0] from a different word)
    if (blockIdx.x == 0 && threadIdx.x == 0) st[2] = 1.0f;
}

__global__ __launch_bounds__(256) void unscale_check_kernel(float* __restrict__ p, int64_t n, float* __restrict__ st) {
    const float inv = st[1];
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = p[i] * inv;
        p[i] = v;
        bad |= !(fabsf(v) <= 3.4028234e38f);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) st[2] = 0.0f;
}

__global__ __launch_bounds__(256) void sgd_gated_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ buf, int64_t n, float lr, float mu, float wd,
                                                        int first, int repeats, const float* __restrict__ st) {
    if (st[2] == 0.0f) return;                    // the gradients overflowed: the step is skipped, momentum untouched
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float pi = p[i];
        float b = first ? 0.f : buf[i];
        sgd_update(pi, b, g[i], lr, mu, wd, first, repeats);
        buf[i] = b;
        p[i] = pi;
    }
}

__global__ void scale_update_kernel(float* __restrict__ st) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float sc = st[0];
    if (st[2] == 0.0f) {                          // overflow: halve (torch.cuda.amp.GradScaler's backoff), count it
        sc = fmaxf(sc * 0.5f, st[7]);
        st[3] = 0.0f;
        st[4] += 1.0f;
    } else {
        st[3] += 1.0f;
        if (st[6] > 0.0f && st[3] >= st[6] && sc < st[5]) {
            sc = fminf(sc * 2.0f, st[5]);
            st[3] = 0.0f;
        }
    }
    st[0] = sc;
    st[1] = 1.0f / sc;
}

// ---- the optimizers build_optimizer can construct besides SGD (Dassl/dassl/optim/optimizer.py:88-138) ----------------
// One launch over the flat buffer per optimizer step, `repeats` applications on the SAME gradient at the consecutive step
// numbers t+1 .. t+repeats.  The hyper-parameters, the step count t and the running powers beta1^t / beta2^t are doubles
// (ffm_optim_desc): by value for the eager step, in device memory for the captured one - the same kernel either way, so
// the two agree bit for bit.  Application k's scalars are formed once per block, by thread k, in double, and rounded to
// float as torch rounds its Python scalars; the powers advance by one IEEE multiplication per application, as the host's do.
struct OptimApp {
    float a;      // adam*: -lr / (1 - b1^t)        radam: -step_size * lr
    float b;      // adam*: sqrt(1 - b2^t)          radam: -weight_decay * lr
    int rect;     // radam: N_sma >= 5 (the rectified branch)
};

struct OptimConst {
    float lr, b1, omb1, b2, omb2, eps, wd, decay, mu, alpha, omalpha;
};

template <int KIND>
__device__ __forceinline__ void optim_app_scalars(const ffm_optim_desc& d, int k, OptimApp& o) {
#pragma clang fp contract(off)
    double pw1 = d.pow1, pw2 = d.pow2;
    for (int j = 0; j <= k; ++j) {
        pw1 *= d.beta1;
        pw2 *= d.beta2;
    }
    const double t = d.step + (double)(k + 1);
    o.a = o.b = 0.f;
    o.rect = 0;
    if (KIND == FFM_OPTIM_ADAM || KIND == FFM_OPTIM_ADAMW || KIND == FFM_OPTIM_AMSGRAD) {
        // torch/optim/adam.py _single_tensor_adam: step_size = lr / bias_correction1, denom = sqrt(v) / sqrt(bias_correction2) + eps
        o.a = (float)(-(d.lr / (1.0 - pw1)));
        o.b = (float)sqrt(1.0 - pw2);
    } else if (KIND == FFM_OPTIM_RADAM) {
        // Dassl/dassl/optim/radam.py:93-109
        const double nmax = 2.0 / (1.0 - d.beta2) - 1.0;
        const double nsma = nmax - 2.0 * t * pw2 / (1.0 - pw2);
        double step_size;
        if (nsma >= 5.0) {
            step_size = sqrt((1.0 - pw2) * (nsma - 4.0) / (nmax - 4.0) * (nsma - 2.0) / nsma * nmax / (nmax - 2.0)) / (1.0 - pw1);
            o.rect = 1;
        } else {
            step_size = 1.0 / (1.0 - pw1);        // degenerated_to_sgd=True
        }
        o.a = (float)(-step_size * d.lr);
        o.b = (float)(-d.weight_decay * d.lr);
    }
}

// one element through `repeats` applications; s0 / s1 / s2 are its entries of the state rows (see ffm_optim_state_rows)
template <int KIND>
__device__ __forceinline__ void optim_update(float& p, float& s0, float& s1, float& s2, float g, const OptimConst& c,
                                             const OptimApp* app, int repeats, int first) {
    if (KIND == FFM_OPTIM_SGD) {
        sgd_update(p, s0, g, c.lr, c.mu, c.wd, first, repeats);
        return;
    }
    // The float32 association is torch's own, operation for operation (its CPU kernels: `add(alpha)` and `lerp` are one fused
    // multiply-add, `mul_` rounds, `addcmul` is (value * t1) * t2 fused into the sum, `addcdiv` is (value * t1) / t2 then the
    // sum), so that the state rows and the update carry the roundings of the classes the reference constructs.
    for (int k = 0; k < repeats; ++k) {
#pragma clang fp contract(off)
        if (KIND == FFM_OPTIM_ADAM || KIND == FFM_OPTIM_ADAMW || KIND == FFM_OPTIM_AMSGRAD) {
            float gi = g;
            if (KIND == FFM_OPTIM_ADAMW) p = p * c.decay;           // p *= 1 - lr*wd, then Adam without L2
            else gi = fmaf(c.wd, p, g);                             // L2 folded into the gradient
            s0 = fmaf(c.omb1, gi - s0, s0);                         // exp_avg.lerp_(grad, 1 - beta1)
            s1 = fmaf(c.omb2 * gi, gi, s1 * c.b2);                  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
            float v = s1;
            if (KIND == FFM_OPTIM_AMSGRAD) {
                s2 = fmaxf(s2, s1);
                v = s2;
            }
            const float den = sqrtf(v) / app[k].b + c.eps;
            p = p + (app[k].a * s0) / den;                          // param.addcdiv_(exp_avg, denom, value=-step_size)
        } else if (KIND == FFM_OPTIM_RMSPROP) {
            // torch/optim/rmsprop.py _single_tensor_rmsprop, centered=False: s0 the momentum buffer, s1 the square average
            const float gi = fmaf(c.wd, p, g);
            s1 = fmaf(c.omalpha * gi, gi, s1 * c.alpha);
            const float avg = sqrtf(s1) + c.eps;
            if (c.mu > 0.f) {
                s0 = s0 * c.mu + gi / avg;                          // buf.mul_(momentum).addcdiv_(grad, avg)
                p = fmaf(-c.lr, s0, p);
            } else {
                p = p + (-c.lr * gi) / avg;
            }
        } else {                                                    // FFM_OPTIM_RADAM (Dassl/dassl/optim/radam.py:84-128)
            s1 = fmaf(c.omb2 * g, g, s1 * c.b2);
            s0 = fmaf(c.omb1, g, s0 * c.b1);
            p = fmaf(app[k].b, p, p);                               // p += -wd*lr*p
            if (app[k].rect) p = p + (app[k].a * s0) / (sqrtf(s1) + c.eps);
            else p = fmaf(app[k].a, s0, p);
        }
    }
}

// state = [K][n]; vec: 16-byte loads and stores for the first n4 quads (the caller checked the alignment of every row),
// a scalar loop for the rest.  Elementwise: the result does not depend on the launch geometry.
template <int KIND>
__global__ __launch_bounds__(256) void optim_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ state, int64_t n, int64_t n4, ffm_optim_desc hv,
                                                    const ffm_optim_desc* __restrict__ hd, int repeats,
                                                    const float* __restrict__ st) {
#pragma clang fp contract(off)
    if (st && st[2] == 0.0f) return;              // the gradients overflowed: nothing moves (uniform over the grid)
    __shared__ OptimApp app[16];
    const ffm_optim_desc d = hd ? *hd : hv;
    if ((int)threadIdx.x < repeats) optim_app_scalars<KIND>(d, threadIdx.x, app[threadIdx.x]);
    __syncthreads();
    OptimConst c;
    c.lr = (float)d.lr;
    c.b1 = (float)d.beta1;
    c.omb1 = (float)(1.0 - d.beta1);              // formed in double, then rounded: 1.0f - (float)beta is 1e-5 off
    c.b2 = (float)d.beta2;
    c.omb2 = (float)(1.0 - d.beta2);
    c.eps = (float)d.eps;
    c.wd = (float)d.weight_decay;
    c.decay = (float)(1.0 - d.lr * d.weight_decay);
    c.mu = (float)d.momentum;
    c.alpha = (float)d.alpha;
    c.omalpha = (float)(1.0 - d.alpha);
    const int first = d.step == 0.0;
    constexpr int K = KIND == FFM_OPTIM_SGD ? 1 : KIND == FFM_OPTIM_AMSGRAD ? 3 : 2;
    float* r0 = state;
    float* r1 = K > 1 ? state + n : state;
    float* r2 = K > 2 ? state + 2 * n : state;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < n4; i += nthr) {
        float4 pv = reinterpret_cast<float4*>(p)[i];
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 a0 = reinterpret_cast<float4*>(r0)[i], a1 = a0, a2 = a0;
        if (K > 1) a1 = reinterpret_cast<float4*>(r1)[i];
        if (K > 2) a2 = reinterpret_cast<float4*>(r2)[i];
        optim_update<KIND>(pv.x, a0.x, a1.x, a2.x, gv.x, c, app, repeats, first);
        optim_update<KIND>(pv.y, a0.y, a1.y, a2.y, gv.y, c, app, repeats, first);
        optim_update<KIND>(pv.z, a0.z, a1.z, a2.z, gv.z, c, app, repeats, first);
        optim_update<KIND>(pv.w, a0.w, a1.w, a2.w, gv.w, c, app, repeats, first);
        reinterpret_cast<float4*>(p)[i] = pv;
        reinterpret_cast<float4*>(r0)[i] = a0;
        if (K > 1) reinterpret_cast<float4*>(r1)[i] = a1;
        if (K > 2) reinterpret_cast<float4*>(r2)[i] = a2;
    }
    for (int64_t i = n4 * 4 + tid; i < n; i += nthr) {
        float pi = p[i], a0 = r0[i], a1 = K > 1 ? r1[i] : 0.f, a2 = K > 2 ? r2[i] : 0.f;
        optim_update<KIND>(pi, a0, a1, a2, g[i], c, app, repeats, first);
        p[i] = pi;
        r0[i] = a0;
        if (K > 1) r1[i] = a1;
        if (K > 2) r2[i] = a2;
    }
}

// behind optim_kernel on a captured step: the device-resident count and powers move on by `repeats` - unless the step was
// skipped, so that the next good step applies step number t+1
__global__ void optim_advance_kernel(ffm_optim_desc* __restrict__ d, int repeats, const float* __restrict__ st) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (st && st[2] == 0.0f) return;
    double pw1 = d->pow1, pw2 = d->pow2;
    for (int k = 0; k < repeats; ++k) {
        pw1 *= d->beta1;
        pw2 *= d->beta2;
    }
    d->pow1 = pw1;
    d->pow2 = pw2;
    d->step += (double)repeats;
}

int optim_rows(int kind) {
    switch (kind) {
        case FFM_OPTIM_SGD: return 1;
        case FFM_OPTIM_ADAM: case FFM_OPTIM_ADAMW: case FFM_OPTIM_RMSPROP: case FFM_OPTIM_RADAM: return 2;
        case FFM_OPTIM_AMSGRAD: return 3;
        default: return FFM_EINVAL;
    }
}

int optim_launch(float* p, const float* g, float* state, int64_t n, int kind, const ffm_optim_desc& hv,
                 const ffm_optim_desc* hd, int repeats, const float* st, hipStream_t s) {
    const int K = optim_rows(kind);
    // 16-byte accesses when p, g and every state row start on a 16-byte boundary (rows are n floats apart)
    const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)state) & 15) == 0) && (K == 1 || n % 4 == 0);
    const int64_t n4 = vec ? n / 4 : 0;
    const dim3 grid(grid_for(n4 > 0 ? n4 : n)), block(256);
#define FFM_OPTIM_CASE(KIND) \
    case KIND: hipLaunchKernelGGL((optim_kernel<KIND>), grid, block, 0, s, p, g, state, n, n4, hv, hd, repeats, st); break;
    switch (kind) {
        FFM_OPTIM_CASE(FFM_OPTIM_SGD)
        FFM_OPTIM_CASE(FFM_OPTIM_ADAM)
        FFM_OPTIM_CASE(FFM_OPTIM_ADAMW)
        FFM_OPTIM_CASE(FFM_OPTIM_AMSGRAD)
        FFM_OPTIM_CASE(FFM_OPTIM_RMSPROP)
        FFM_OPTIM_CASE(FFM_OPTIM_RADAM)
        default: return FFM_EINVAL;
    }
#undef FFM_OPTIM_CASE
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}

}  // namespace

extern "C" int ffm_optim_state_rows(int kind) { return optim_rows(kind); }

extern "C" int ffm_optim_step(float* p, const float* g, float* state, int64_t n, int kind, const ffm_optim_desc* desc,
                              int repeats, float* scale_state, void* stream) {
    if (!p || !g || !state || !desc || n <= 0 || repeats < 1 || repeats > 16 || optim_rows(kind) < 0) return FFM_EINVAL;
    const int rc = optim_launch(p, g, state, n, kind, *desc, nullptr, repeats, scale_state, (hipStream_t)stream);
    if (rc) return rc;
    if (scale_state) {
        hipLaunchKernelGGL(scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, scale_state);
        FFM_CHECK_LAUNCH();
    }
    return FFM_OK;
}

extern "C" int ffm_optim_step_dev(float* p, const float* g, float* state, int64_t n, int kind, ffm_optim_desc* desc_dev,
                                  int repeats, float* scale_state, void* stream) {
    if (!p || !g || !state || !desc_dev || n <= 0 || repeats < 1 || repeats > 16 || optim_rows(kind) < 0) return FFM_EINVAL;
    const int rc = optim_launch(p, g, state, n, kind, ffm_optim_desc{}, desc_dev, repeats, scale_state, (hipStream_t)stream);
    if (rc) return rc;
    hipLaunchKernelGGL(optim_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, desc_dev, repeats, scale_state);
    FFM_CHECK_LAUNCH();
    if (scale_state) {
        hipLaunchKernelGGL(scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, scale_state);
        FFM_CHECK_LAUNCH();
    }
    return FFM_OK;
}

extern "C" int ffm_abi_version(void) { return FFM_ABI_VERSION; }

extern "C" int ffm_sgd_momentum(float* p, const float* g, float* buf, int64_t n, float lr, float momentum,
                                float weight_decay, int first_step, void* stream) {
    if (!p || !g || !buf || n <= 0) return FFM_EINVAL;
    hipLaunchKernelGGL(sgd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, g, buf, n, lr, momentum,
                       weight_decay, first_step);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}

extern "C" int ffm_sgd_momentum_n(float* p, const float* g, float* buf, int64_t n, float lr, float momentum,
                                  float weight_decay, int first_step, int repeats, void* stream) {
    if (!p || !g || !buf || n <= 0 || repeats < 1 || repeats > 16) return FFM_EINVAL;
    hipLaunchKernelGGL(sgd_n_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, g, buf, n, lr, momentum,
                       weight_decay, first_step, repeats);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}

extern "C" int ffm_sgd_momentum_dev(float* p, const float* g, float* buf, int64_t n, const float* hp, int repeats,
                                    float* state, void* stream) {
    if (!p || !g || !buf || !hp || n <= 0 || repeats < 1 || repeats > 16) return FFM_EINVAL;
    hipLaunchKernelGGL(sgd_dev_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, g, buf, n, hp, repeats,
                       state);
    FFM_CHECK_LAUNCH();
    if (state) {
        hipLaunchKernelGGL(scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state);
        FFM_CHECK_LAUNCH();
    }
    return FFM_OK;
}

extern "C" int ffm_scale_by(const float* p, const float* w, float* out, int64_t n, void* stream) {
    if (!p || !w || !out || n <= 0) return FFM_EINVAL;
    hipLaunchKernelGGL(scale_by_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, w, out, n);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}

extern "C" int ffm_scale_acc(const float* p, const float* w, float* acc, int64_t n, void* stream) {
    if (!p || !w || !acc || n <= 0) return FFM_EINVAL;
    hipLaunchKernelGGL(scale_acc_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, w, acc, n);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}

extern "C" int ffm_scale_check(float* p, float scale, int64_t n, int32_t* finite_flag, void* stream) {
    if (!p || n <= 0) return FFM_EINVAL;
    hipLaunchKernelGGL(scale_check_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, scale, n, finite_flag);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}

extern "C" int ffm_loss_scale(float* p, int64_t n, float* state, void* stream) {
    if (!p || !state || n <= 0) return FFM_EINVAL;
    hipLaunchKernelGGL(loss_scale_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, n, state);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}

extern "C" int ffm_unscale_check(float* g, int64_t n, float* state, void* stream) {
    if (!g || !state || n <= 0) return FFM_EINVAL;
    hipLaunchKernelGGL(unscale_check_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, g, n, state);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}

extern "C" int ffm_sgd_momentum_gated(float* p, const float* g, float* buf, int64_t n, float lr, float momentum,
                                      float weight_decay, int first_step, int repeats, float* state, void* stream) {
    if (!p || !g || !buf || !state || n <= 0 || repeats < 1 || repeats > 16) return FFM_EINVAL;
    hipLaunchKernelGGL(sgd_gated_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, g, buf, n, lr, momentum,
                       weight_decay, first_step, repeats, state);
    FFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}

extern "C" int ffm_fedavg_finish(float* avg, const float* prev, float* out, int64_t n, const int64_t* s_offsets,
                                 int n_s, int G, int r, int shared_half_s, float beta, void* stream) {
    if (!avg || !prev || !out || n <= 0) return FFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (shared_half_s && n_s > 0) {
        if (!s_offsets || G <= 0 || r <= 0) return FFM_EINVAL;
        hipLaunchKernelGGL(shared_half_kernel, dim3(n_s), dim3(64), 0, s, avg, s_offsets, n_s, G, r);
        FFM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ema_kernel, dim3(grid_for(n)), dim3(256), 0, s, avg, prev, out, n, beta);
    FFM_CHECK_LAUNCH();
    return FFM_OK;
}
