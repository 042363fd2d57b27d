// Optimizer step of the training path (trainer.py:116-122: clip_grad_norm_ -> optimizer.step(), Adam as main.py:171-191 builds it):
// global gradient norm, clip coefficient, Adam update and the clipped gradient's write-back in THREE launches over a table of
// parameter segments -- one pass over (p, g, m, v) instead of the library's norm reductions per bucket + a multiply over every
// gradient + the fused Adam's own pass.  Everything the update needs (norm, coefficient, step counters) stays on the device, so
// the step can be captured into a HIP graph.
//
// Arithmetic = torch.optim.Adam (amsgrad = False, maximize = False), per segment:
//     g   = grad * coef                         coef = min(1, max_norm / (inv * ||grad|| + 1e-6)) * inv   (inv = 1 / ranks: the
//                                               gradient arenas hold sums over ranks, cvc.distributed.GradReducer.clip_)
//     g  += weight_decay * p
//     m   = m + (g - m) * (1 - beta1)           v = beta2 * v + (1 - beta2) * g * g
//     p  -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)          t = the segment's step count after this step
// Sums of squares are taken chunk by chunk and combined in chunk order: the norm is the same bits run to run.
//
// The reference's other two optimizers (main.py:182-191: sgd with momentum 0.9, adamax) take the same first two launches and their
// own update kernel in the third (cvc_sgd_clip_step, cvc_adamax_clip_step: building blocks, include/cvc_hip_blocks.h):
//     buf = mom * buf + g                       p -= lr * buf                                    torch.optim.SGD, dampening 0
//     m   = m + (g - m) * (1 - beta1)           u = max(beta2 * u, |g| + eps)    p -= (lr / (1 - beta1^t)) * m / u     torch.optim.Adamax
#include "cvc_common.h"
#include <math.h>

namespace {

constexpr int OPT_WG = 256;
constexpr int OPT_CHUNK = 1 << 16;          // elements per workgroup

struct OptSeg {                             // mirrors cvc_optim_seg (include/cvc_hip.h)
    float* p; float* g; float* m; float* v;
    float* step;                            // this parameter's step count (float32, as torch keeps it on the device)
    long long n;
    float lr, weight_decay;
};

struct OptChunk { int seg; int pad; long long start; };

__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < OPT_WG / 64; ++i) t += red[i];
    }
    return t;                                // valid in thread 0
}

__global__ __launch_bounds__(OPT_WG) void optim_sumsq_kernel(const OptSeg* segs, const OptChunk* chunks, float* partial) {
    __shared__ float red[OPT_WG / 64];
    const OptChunk c = chunks[blockIdx.x];
    const OptSeg s = segs[c.seg];
    const long long end = c.start + OPT_CHUNK < s.n ? c.start + OPT_CHUNK : s.n;
    float acc = 0.f;
    const float* g = s.g;
    if ((((uintptr_t)g) & 15) == 0) {
        long long i = c.start + (long long)threadIdx.x * 4;
        for (; i + 4 <= end; i += OPT_WG * 4) {
            const f32x4 x = ld4(g + i);
            acc += (x.x * x.x + x.y * x.y) + (x.z * x.z + x.w * x.w);
        }
        for (; i < end; ++i) acc += (i < end) ? g[i] * g[i] : 0.f;          // (the tail of the last chunk: < 4 elements of one thread)
    } else {
        for (long long i = c.start + threadIdx.x; i < end; i += OPT_WG) acc += g[i] * g[i];
    }
    const float t = block_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// one workgroup: partial sums in chunk order -> norm, clip coefficient; every segment's step count += 1
__device__ __forceinline__ void optim_finalize(const OptSeg* segs, int nseg, const float* partial, int nchunk, float max_norm, float inv,
                                               float* out /* [0] = norm of the averaged gradient, [1] = coef */, const int* skip) {
    __shared__ float red[OPT_WG / 64];
    if (skip && *skip != 0) {                  // the step is void (a launch of it reported invalid outputs): no step count moves
        if (threadIdx.x == 0) { out[0] = 0.f; out[1] = 0.f; }
        return;
    }
    // fixed assignment (thread t sums partials t, t + 256, ...) and a fixed combine: deterministic
    float acc = 0.f;
    for (int i = threadIdx.x; i < nchunk; i += OPT_WG) acc += partial[i];
    const float t = block_sum(acc, red);
    if (threadIdx.x == 0) {
        const float total = sqrtf(t) * inv;
        out[0] = total;
        // a NaN norm poisons every gradient, as torch's clip_grad_norm_ does (clamp(NaN, max=1) = NaN; fminf would return 1)
        out[1] = max_norm > 0.f ? (total != total ? total : fminf(max_norm / (total + 1e-6f), 1.0f) * inv) : inv;
    }
    // (a rule without a step count -- SGD -- leaves the segment's `step` NULL)
    for (int s = threadIdx.x; s < nseg; s += OPT_WG)
        if (segs[s].step) segs[s].step[0] += 1.0f;
}

__global__ __launch_bounds__(OPT_WG) void optim_finalize_kernel(const OptSeg* segs, int nseg, const float* partial, int nchunk, float max_norm,
                                                                float inv, float* out, const int* skip) {
    optim_finalize(segs, nseg, partial, nchunk, max_norm, inv, out, skip);
}

// ... and, under weight averaging, the effective decay of this step.  ema_state = [averaged (non-void) steps so far, d_eff of the
// current step]: both live on the device, so nothing the host passes changes between replays of a captured step.  A void step is not
// averaged: neither word moves.
__global__ __launch_bounds__(OPT_WG) void optim_finalize_ema_kernel(const OptSeg* segs, int nseg, const float* partial, int nchunk,
                                                                    float max_norm, float inv, float* out, const int* skip,
                                                                    float* ema_state, float decay, int warmup) {
    if (threadIdx.x == 0 && !(skip && *skip != 0)) {
        const float n = ema_state[0];
        // the TensorFlow / timm warm-up: min(d, (1 + n) / (10 + n)), n = the averaged steps BEFORE this one
        ema_state[1] = warmup ? fminf(decay, (1.0f + n) / (10.0f + n)) : decay;
        ema_state[0] = n + 1.0f;
    }
    optim_finalize(segs, nseg, partial, nchunk, max_norm, inv, out, skip);
}

__global__ __launch_bounds__(OPT_WG) void optim_adam_kernel(const OptSeg* segs, const OptChunk* chunks, const float* norm_coef, float beta1,
                                                            float beta2, float eps, int write_grad, const int* skip) {
    const OptChunk c = chunks[blockIdx.x];
    const OptSeg s = segs[c.seg];
    const long long end = c.start + OPT_CHUNK < s.n ? c.start + OPT_CHUNK : s.n;
    if (skip && *skip != 0) {
        // void step: p, m, v stay as they are.  write_grad == 2 promised the caller zeroed gradients (the next step's zero_grad()
        // is folded into this pass): kept -- the void step's gradients are garbage anyway
        if (write_grad == 2)
            for (long long i = c.start + threadIdx.x; i < end; i += OPT_WG) s.g[i] = 0.f;
        return;
    }
    const float coef = norm_coef[1];
    const float t = s.step[0];                                             // already incremented by the finalize launch
    // bias corrections as torch computes them (1 - beta^t in fp32 via pow)
    const float bc1 = 1.0f - powf(beta1, t), bc2 = 1.0f - powf(beta2, t);
    const float step_size = s.lr / bc1, inv_sqrt_bc2 = 1.0f / sqrtf(bc2);
    const float wd = s.weight_decay, omb1 = 1.0f - beta1, omb2 = 1.0f - beta2;
    // Every product-and-sum is an explicit fmaf: left to the compiler's contraction, the float4 loop fused g + wd * p and
    // beta2 * v + ... while the scalar loops (a misaligned operand, the < 4 tail elements of an aligned one) rounded the products
    // first, and the same values gave other bits depending on where the allocator had put them.  These are the float4 loop's bits.
    auto upd = [&](float& p, float& g, float& m, float& v) __attribute__((always_inline)) {
        g *= coef;
        const float ge = wd != 0.f ? fmaf(wd, p, g) : g;
        m = fmaf(ge - m, omb1, m);
        v = fmaf(beta2, v, (omb2 * ge) * ge);
        p = fmaf(-step_size, m / fmaf(sqrtf(v), inv_sqrt_bc2, eps), p);
    };
    const bool al = ((((uintptr_t)s.p) | ((uintptr_t)s.g) | ((uintptr_t)s.m) | ((uintptr_t)s.v)) & 15) == 0;
    if (al) {
        long long i = c.start + (long long)threadIdx.x * 4;
        for (; i + 4 <= end; i += OPT_WG * 4) {
            f32x4 p = ld4(s.p + i), g = ld4(s.g + i), m = ld4(s.m + i), v = ld4(s.v + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = p[e], ge = g[e], me = m[e], ve = v[e];
                upd(pe, ge, me, ve);
                p[e] = pe; g[e] = ge; m[e] = me; v[e] = ve;
            }
            st4(s.p + i, p); st4(s.m + i, m); st4(s.v + i, v);
            if (write_grad == 1) st4(s.g + i, g);
            else if (write_grad == 2) st4(s.g + i, f32x4{0.f, 0.f, 0.f, 0.f});
        }
        for (; i < end; ++i) {
            float p = s.p[i], g = s.g[i], m = s.m[i], v = s.v[i];
            upd(p, g, m, v);
            s.p[i] = p; s.m[i] = m; s.v[i] = v;
            if (write_grad) s.g[i] = write_grad == 2 ? 0.f : g;
        }
    } else {
        for (long long i = c.start + threadIdx.x; i < end; i += OPT_WG) {
            float p = s.p[i], g = s.g[i], m = s.m[i], v = s.v[i];
            upd(p, g, m, v);
            s.p[i] = p; s.m[i] = m; s.v[i] = v;
            if (write_grad) s.g[i] = write_grad == 2 ? 0.f : g;
        }
    }
}

// ---- SGD with momentum and Adamax: the same three launches, another third kernel.  One chunk of one segment under `upd`, with
// NS state arrays next to p and g (0: none, 1: m, 2: m and v): optim_adam_kernel's loops -- float4 when every operand the rule
// has is 16-byte aligned, scalar for the < 4 tail elements and for a misaligned operand -- and its write_grad / void-step rules.
//
// EMA: the weight average rides the same pass.  `ea` is the segment's shadow (never NULL here), `omd` = 1 - d_eff of this step:
//     e = fmaf(p_new - e, omd, e)
// from the p the rule has just produced, still in registers.  The lerp form on purpose: p_new == e leaves e's bits alone (a frozen
// weight's average does not drift), which d e + (1 - d) p does not.  e is loaded with the other operands and counts as one of them
// for the float4 form.  p, g and the state get the bits of the plain form: the rule's arithmetic does not see e.
template <int NS, bool EMA = false, class Upd>
__device__ __forceinline__ void optim_rule_pass(const OptSeg& s, long long start, long long end, int write_grad, bool is_void, Upd upd,
                                                float* ea = nullptr, float omd = 0.f) {
    if (is_void) {                             // p, the state (and the average) stay as they are; write_grad == 2 still leaves the gradients zero
        if (write_grad == 2)
            for (long long i = start + threadIdx.x; i < end; i += OPT_WG) s.g[i] = 0.f;
        return;
    }
    auto one = [&](long long i) __attribute__((always_inline)) {
        float p = s.p[i], g = s.g[i], m = 0.f, v = 0.f, a = 0.f;
        if constexpr (NS >= 1) m = s.m[i];
        if constexpr (NS >= 2) v = s.v[i];
        if constexpr (EMA) a = ea[i];
        upd(p, g, m, v);
        s.p[i] = p;
        if constexpr (NS >= 1) s.m[i] = m;
        if constexpr (NS >= 2) s.v[i] = v;
        if constexpr (EMA) ea[i] = fmaf(p - a, omd, a);
        if (write_grad) s.g[i] = write_grad == 2 ? 0.f : g;
    };
    uintptr_t addr = ((uintptr_t)s.p) | ((uintptr_t)s.g);
    if constexpr (NS >= 1) addr |= (uintptr_t)s.m;
    if constexpr (NS >= 2) addr |= (uintptr_t)s.v;
    if constexpr (EMA) addr |= (uintptr_t)ea;
    if ((addr & 15) == 0) {
        long long i = start + (long long)threadIdx.x * 4;
        for (; i + 4 <= end; i += OPT_WG * 4) {
            f32x4 p = ld4(s.p + i), g = ld4(s.g + i), m = {0.f, 0.f, 0.f, 0.f}, v = {0.f, 0.f, 0.f, 0.f}, a = {0.f, 0.f, 0.f, 0.f};
            if constexpr (NS >= 1) m = ld4(s.m + i);
            if constexpr (NS >= 2) v = ld4(s.v + i);
            if constexpr (EMA) a = ld4(ea + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = p[e], ge = g[e], me = m[e], ve = v[e];
                upd(pe, ge, me, ve);
                p[e] = pe; g[e] = ge; m[e] = me; v[e] = ve;
                if constexpr (EMA) a[e] = fmaf(pe - a[e], omd, a[e]);
            }
            st4(s.p + i, p);
            if constexpr (NS >= 1) st4(s.m + i, m);
            if constexpr (NS >= 2) st4(s.v + i, v);
            if constexpr (EMA) st4(ea + i, a);
            if (write_grad == 1) st4(s.g + i, g);
            else if (write_grad == 2) st4(s.g + i, f32x4{0.f, 0.f, 0.f, 0.f});
        }
        for (; i < end; ++i) one(i);
    } else {
        for (long long i = start + threadIdx.x; i < end; i += OPT_WG) one(i);
    }
}

// torch.optim.SGD (dampening 0, no Nesterov, no maximize).  m = momentum_buffer; a zero buffer gives torch's first step (buf = ge)
// exactly.  A segment whose m is NULL has no buffer (momentum 0, as torch keeps none): p -= lr ge.
__global__ __launch_bounds__(OPT_WG) void optim_sgd_kernel(const OptSeg* segs, const OptChunk* chunks, const float* norm_coef, float mom,
                                                           int write_grad, const int* skip) {
    const OptChunk c = chunks[blockIdx.x];
    const OptSeg s = segs[c.seg];
    const long long end = c.start + OPT_CHUNK < s.n ? c.start + OPT_CHUNK : s.n;
    const bool is_void = skip && *skip != 0;
    const float coef = norm_coef[1], wd = s.weight_decay, nlr = -s.lr;
    // The same bits in every form, as in optim_adam_kernel: contraction is off, so what is fused is what is spelled fmaf.  One
    // operation is deliberately NOT fused, the buffer's update below.
    if (s.m != nullptr) {
        optim_rule_pass<1>(s, c.start, end, write_grad, is_void, [&](float& p, float& g, float& m, float&) __attribute__((always_inline)) {
#pragma clang fp contract(off)
            g *= coef;
            const float ge = wd != 0.f ? fmaf(wd, p, g) : g;
            // Product rounded, then the sum, as torch's buf.mul_(mom).add_(g): where mom buf and g cancel (a buffer of 9, a gradient
            // of -8) an fma differs from torch by an ulp of the PRODUCT, and the buffer is state, so the difference is carried into
            // every later step.  Rounded as torch rounds it, the buffer follows torch's.
            m = mom * m + ge;
            p = fmaf(nlr, m, p);
        });
    } else {
        optim_rule_pass<0>(s, c.start, end, write_grad, is_void, [&](float& p, float& g, float&, float&) __attribute__((always_inline)) {
#pragma clang fp contract(off)
            g *= coef;
            const float ge = wd != 0.f ? fmaf(wd, p, g) : g;
            p = fmaf(nlr, ge, p);
        });
    }
}

// torch.optim.Adamax (no maximize).  m = exp_avg, v = exp_inf, t = the segment's step count after the finalize launch's += 1.
__global__ __launch_bounds__(OPT_WG) void optim_adamax_kernel(const OptSeg* segs, const OptChunk* chunks, const float* norm_coef, float beta1,
                                                              float beta2, float eps, int write_grad, const int* skip) {
    const OptChunk c = chunks[blockIdx.x];
    const OptSeg s = segs[c.seg];
    const long long end = c.start + OPT_CHUNK < s.n ? c.start + OPT_CHUNK : s.n;
    const bool is_void = skip && *skip != 0;
    const float coef = norm_coef[1], wd = s.weight_decay, omb1 = 1.0f - beta1;
    const float nclr = -(s.lr / (1.0f - powf(beta1, s.step[0])));           // bias correction as torch computes it (fp32 pow)
    optim_rule_pass<2>(s, c.start, end, write_grad, is_void, [&](float& p, float& g, float& m, float& u) __attribute__((always_inline)) {
#pragma clang fp contract(off)
        g *= coef;
        const float ge = wd != 0.f ? fmaf(wd, p, g) : g;
        m = fmaf(ge - m, omb1, m);
        // torch.maximum: a NaN on either side is the result (fmaxf would drop it and a NaN gradient would leave no trace in u)
        const float a = beta2 * u, b = fabsf(ge) + eps;
        u = a != a ? a : (b != b ? b : fmaxf(a, b));
        p = fmaf(nclr, m / u, p);
    });
}

// ---- weight averaging (EMA) inside the step: cvc_*_clip_step_ema.  The plain kernels above are what the plain entries launch,
// untouched; these are their rules over optim_rule_pass<NS, true>.  ema[seg] == NULL: the segment has no shadow and takes the plain
// pass.  ema_state = [averaged steps so far, d_eff of the current step], written by optim_finalize_ema_kernel, the second
// launch: three launches, as the plain step.
template <int NS, class Upd>
__device__ __forceinline__ void optim_rule_pass_ema(const OptSeg& s, long long start, long long end, int write_grad, bool is_void, Upd upd,
                                                    float* ea, const float* ema_state) {
    if (ea == nullptr) { optim_rule_pass<NS>(s, start, end, write_grad, is_void, upd); return; }
    const float omd = 1.0f - ema_state[1];       // (a void step never reads it: optim_rule_pass returns first)
    optim_rule_pass<NS, true>(s, start, end, write_grad, is_void, upd, ea, omd);
}

__global__ __launch_bounds__(OPT_WG) void optim_adam_ema_kernel(const OptSeg* segs, const OptChunk* chunks, const float* norm_coef, float beta1,
                                                                float beta2, float eps, int write_grad, const int* skip,
                                                                float* const* ema, const float* ema_state) {
    const OptChunk c = chunks[blockIdx.x];
    const OptSeg s = segs[c.seg];
    const long long end = c.start + OPT_CHUNK < s.n ? c.start + OPT_CHUNK : s.n;
    const bool is_void = skip && *skip != 0;
    const float coef = norm_coef[1];
    const float t = s.step[0];
    // optim_adam_kernel's scalars and its `upd`, operation for operation
    const float bc1 = 1.0f - powf(beta1, t), bc2 = 1.0f - powf(beta2, t);
    const float step_size = s.lr / bc1, inv_sqrt_bc2 = 1.0f / sqrtf(bc2);
    const float wd = s.weight_decay, omb1 = 1.0f - beta1, omb2 = 1.0f - beta2;
    optim_rule_pass_ema<2>(s, c.start, end, write_grad, is_void, [&](float& p, float& g, float& m, float& v) __attribute__((always_inline)) {
#pragma clang fp contract(off)
        g *= coef;
        const float ge = wd != 0.f ? fmaf(wd, p, g) : g;
        m = fmaf(ge - m, omb1, m);
        v = fmaf(beta2, v, (omb2 * ge) * ge);
        p = fmaf(-step_size, m / fmaf(sqrtf(v), inv_sqrt_bc2, eps), p);
    }, ema[c.seg], ema_state);
}

__global__ __launch_bounds__(OPT_WG) void optim_sgd_ema_kernel(const OptSeg* segs, const OptChunk* chunks, const float* norm_coef, float mom,
                                                               int write_grad, const int* skip, float* const* ema, const float* ema_state) {
    const OptChunk c = chunks[blockIdx.x];
    const OptSeg s = segs[c.seg];
    const long long end = c.start + OPT_CHUNK < s.n ? c.start + OPT_CHUNK : s.n;
    const bool is_void = skip && *skip != 0;
    const float coef = norm_coef[1], wd = s.weight_decay, nlr = -s.lr;
    if (s.m != nullptr) {
        optim_rule_pass_ema<1>(s, c.start, end, write_grad, is_void, [&](float& p, float& g, float& m, float&) __attribute__((always_inline)) {
#pragma clang fp contract(off)
            g *= coef;
            const float ge = wd != 0.f ? fmaf(wd, p, g) : g;
            m = mom * m + ge;                    // product rounded, then the sum: see optim_sgd_kernel
            p = fmaf(nlr, m, p);
        }, ema[c.seg], ema_state);
    } else {
        optim_rule_pass_ema<0>(s, c.start, end, write_grad, is_void, [&](float& p, float& g, float&, float&) __attribute__((always_inline)) {
#pragma clang fp contract(off)
            g *= coef;
            const float ge = wd != 0.f ? fmaf(wd, p, g) : g;
            p = fmaf(nlr, ge, p);
        }, ema[c.seg], ema_state);
    }
}

__global__ __launch_bounds__(OPT_WG) void optim_adamax_ema_kernel(const OptSeg* segs, const OptChunk* chunks, const float* norm_coef, float beta1,
                                                                  float beta2, float eps, int write_grad, const int* skip,
                                                                  float* const* ema, const float* ema_state) {
    const OptChunk c = chunks[blockIdx.x];
    const OptSeg s = segs[c.seg];
    const long long end = c.start + OPT_CHUNK < s.n ? c.start + OPT_CHUNK : s.n;
    const bool is_void = skip && *skip != 0;
    const float coef = norm_coef[1], wd = s.weight_decay, omb1 = 1.0f - beta1;
    const float nclr = -(s.lr / (1.0f - powf(beta1, s.step[0])));
    optim_rule_pass_ema<2>(s, c.start, end, write_grad, is_void, [&](float& p, float& g, float& m, float& u) __attribute__((always_inline)) {
#pragma clang fp contract(off)
        g *= coef;
        const float ge = wd != 0.f ? fmaf(wd, p, g) : g;
        m = fmaf(ge - m, omb1, m);
        const float a = beta2 * u, b = fabsf(ge) + eps;
        u = a != a ? a : (b != b ? b : fmaxf(a, b));
        p = fmaf(nclr, m / u, p);
    }, ema[c.seg], ema_state);
}

// p[i] <-> e[i] over the step's tables: the averaged weights go into the parameters' own storage (everything downstream is keyed on
// the parameters' addresses) and come out again bit for bit.  A pure copy: twice is the identity.  A NULL shadow: nothing moves.
__global__ __launch_bounds__(OPT_WG) void ema_swap_kernel(const OptSeg* segs, const OptChunk* chunks, float* const* ema) {
    const OptChunk c = chunks[blockIdx.x];
    const OptSeg s = segs[c.seg];
    float* e = ema[c.seg];
    if (e == nullptr) return;
    const long long end = c.start + OPT_CHUNK < s.n ? c.start + OPT_CHUNK : s.n;
    if (((((uintptr_t)s.p) | ((uintptr_t)e)) & 15) == 0) {
        long long i = c.start + (long long)threadIdx.x * 4;
        for (; i + 4 <= end; i += OPT_WG * 4) {
            const f32x4 a = ld4(s.p + i), b = ld4(e + i);
            st4(s.p + i, b); st4(e + i, a);
        }
        for (; i < end; ++i) { const float a = s.p[i], b = e[i]; s.p[i] = b; e[i] = a; }
    } else {
        for (long long i = c.start + threadIdx.x; i < end; i += OPT_WG) { const float a = s.p[i], b = e[i]; s.p[i] = b; e[i] = a; }
    }
}

}  // namespace

extern "C" int cvc_optim_chunk_elems(void) { return OPT_CHUNK; }

extern "C" int cvc_adam_clip_step(const cvc_optim_seg* segs, int nseg, const cvc_optim_chunk* chunks, int nchunk, float max_norm,
                                  float inv_world, float beta1, float beta2, float eps, int write_grad, float* partial,
                                  float* norm_coef, const int* skip, cvc_stream_t stream) {
    static_assert(sizeof(cvc_optim_seg) == sizeof(OptSeg) && sizeof(cvc_optim_chunk) == sizeof(OptChunk), "table layouts");
    if (!segs || !chunks || !partial || !norm_coef || nseg < 1 || nchunk < 1 || inv_world <= 0.f || beta1 < 0.f || beta1 >= 1.f ||
        beta2 < 0.f || beta2 >= 1.f || eps < 0.f)
        return CVC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const OptSeg* s = reinterpret_cast<const OptSeg*>(segs);
    const OptChunk* c = reinterpret_cast<const OptChunk*>(chunks);
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3(nchunk), dim3(OPT_WG), 0, st, s, c, partial);
    hipLaunchKernelGGL(optim_finalize_kernel, dim3(1), dim3(OPT_WG), 0, st, s, nseg, partial, nchunk, max_norm, inv_world, norm_coef, skip);
    hipLaunchKernelGGL(optim_adam_kernel, dim3(nchunk), dim3(OPT_WG), 0, st, s, c, norm_coef, beta1, beta2, eps, write_grad, skip);
    return cvc_launch_status();
}

namespace {
bool optim_tables_ok(const cvc_optim_seg* segs, int nseg, const cvc_optim_chunk* chunks, int nchunk, float inv_world, const float* partial,
                     const float* norm_coef) {
    return segs && chunks && partial && norm_coef && nseg >= 1 && nchunk >= 1 && inv_world > 0.f;
}
}  // namespace

// building blocks (include/cvc_hip_blocks.h): cvc_adam_clip_step's three launches with another update rule in the third
extern "C" int cvc_sgd_clip_step(const cvc_optim_seg* segs, int nseg, const cvc_optim_chunk* chunks, int nchunk, float max_norm,
                                 float inv_world, float momentum, int write_grad, float* partial, float* norm_coef, const int* skip,
                                 cvc_stream_t stream) {
    if (!optim_tables_ok(segs, nseg, chunks, nchunk, inv_world, partial, norm_coef) || !(momentum >= 0.f && momentum < 1.f)) return CVC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const OptSeg* s = reinterpret_cast<const OptSeg*>(segs);
    const OptChunk* c = reinterpret_cast<const OptChunk*>(chunks);
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3(nchunk), dim3(OPT_WG), 0, st, s, c, partial);
    hipLaunchKernelGGL(optim_finalize_kernel, dim3(1), dim3(OPT_WG), 0, st, s, nseg, partial, nchunk, max_norm, inv_world, norm_coef, skip);
    hipLaunchKernelGGL(optim_sgd_kernel, dim3(nchunk), dim3(OPT_WG), 0, st, s, c, norm_coef, momentum, write_grad, skip);
    return cvc_launch_status();
}

extern "C" int cvc_adamax_clip_step(const cvc_optim_seg* segs, int nseg, const cvc_optim_chunk* chunks, int nchunk, float max_norm,
                                    float inv_world, float beta1, float beta2, float eps, int write_grad, float* partial,
                                    float* norm_coef, const int* skip, cvc_stream_t stream) {
    if (!optim_tables_ok(segs, nseg, chunks, nchunk, inv_world, partial, norm_coef) || !(beta1 >= 0.f && beta1 < 1.f) ||
        !(beta2 >= 0.f && beta2 < 1.f) || !(eps > 0.f))
        return CVC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const OptSeg* s = reinterpret_cast<const OptSeg*>(segs);
    const OptChunk* c = reinterpret_cast<const OptChunk*>(chunks);
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3(nchunk), dim3(OPT_WG), 0, st, s, c, partial);
    hipLaunchKernelGGL(optim_finalize_kernel, dim3(1), dim3(OPT_WG), 0, st, s, nseg, partial, nchunk, max_norm, inv_world, norm_coef, skip);
    hipLaunchKernelGGL(optim_adamax_kernel, dim3(nchunk), dim3(OPT_WG), 0, st, s, c, norm_coef, beta1, beta2, eps, write_grad, skip);
    return cvc_launch_status();
}

// ---- weight averaging: the three entries above with a shadow per segment (ema[seg], NULL = none), and the exchange
namespace {
bool ema_args_ok(float* const* ema, const float* ema_state, float decay) { return ema && ema_state && decay >= 0.f && decay < 1.f; }
}  // namespace

extern "C" int cvc_adam_clip_step_ema(const cvc_optim_seg* segs, int nseg, const cvc_optim_chunk* chunks, int nchunk, float max_norm,
                                      float inv_world, float beta1, float beta2, float eps, int write_grad, float* partial,
                                      float* norm_coef, const int* skip, float* const* ema, float* ema_state, float decay, int warmup,
                                      cvc_stream_t stream) {
    if (!optim_tables_ok(segs, nseg, chunks, nchunk, inv_world, partial, norm_coef) || !(beta1 >= 0.f && beta1 < 1.f) ||
        !(beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f) || !ema_args_ok(ema, ema_state, decay))
        return CVC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const OptSeg* s = reinterpret_cast<const OptSeg*>(segs);
    const OptChunk* c = reinterpret_cast<const OptChunk*>(chunks);
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3(nchunk), dim3(OPT_WG), 0, st, s, c, partial);
    hipLaunchKernelGGL(optim_finalize_ema_kernel, dim3(1), dim3(OPT_WG), 0, st, s, nseg, partial, nchunk, max_norm, inv_world, norm_coef, skip,
                       ema_state, decay, warmup);
    hipLaunchKernelGGL(optim_adam_ema_kernel, dim3(nchunk), dim3(OPT_WG), 0, st, s, c, norm_coef, beta1, beta2, eps, write_grad, skip, ema,
                       (const float*)ema_state);
    return cvc_launch_status();
}

extern "C" int cvc_sgd_clip_step_ema(const cvc_optim_seg* segs, int nseg, const cvc_optim_chunk* chunks, int nchunk, float max_norm,
                                     float inv_world, float momentum, int write_grad, float* partial, float* norm_coef, const int* skip,
                                     float* const* ema, float* ema_state, float decay, int warmup, cvc_stream_t stream) {
    if (!optim_tables_ok(segs, nseg, chunks, nchunk, inv_world, partial, norm_coef) || !(momentum >= 0.f && momentum < 1.f) ||
        !ema_args_ok(ema, ema_state, decay))
        return CVC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const OptSeg* s = reinterpret_cast<const OptSeg*>(segs);
    const OptChunk* c = reinterpret_cast<const OptChunk*>(chunks);
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3(nchunk), dim3(OPT_WG), 0, st, s, c, partial);
    hipLaunchKernelGGL(optim_finalize_ema_kernel, dim3(1), dim3(OPT_WG), 0, st, s, nseg, partial, nchunk, max_norm, inv_world, norm_coef, skip,
                       ema_state, decay, warmup);
    hipLaunchKernelGGL(optim_sgd_ema_kernel, dim3(nchunk), dim3(OPT_WG), 0, st, s, c, norm_coef, momentum, write_grad, skip, ema,
                       (const float*)ema_state);
    return cvc_launch_status();
}

extern "C" int cvc_adamax_clip_step_ema(const cvc_optim_seg* segs, int nseg, const cvc_optim_chunk* chunks, int nchunk, float max_norm,
                                        float inv_world, float beta1, float beta2, float eps, int write_grad, float* partial,
                                        float* norm_coef, const int* skip, float* const* ema, float* ema_state, float decay, int warmup,
                                        cvc_stream_t stream) {
    if (!optim_tables_ok(segs, nseg, chunks, nchunk, inv_world, partial, norm_coef) || !(beta1 >= 0.f && beta1 < 1.f) ||
        !(beta2 >= 0.f && beta2 < 1.f) || !(eps > 0.f) || !ema_args_ok(ema, ema_state, decay))
        return CVC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const OptSeg* s = reinterpret_cast<const OptSeg*>(segs);
    const OptChunk* c = reinterpret_cast<const OptChunk*>(chunks);
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3(nchunk), dim3(OPT_WG), 0, st, s, c, partial);
    hipLaunchKernelGGL(optim_finalize_ema_kernel, dim3(1), dim3(OPT_WG), 0, st, s, nseg, partial, nchunk, max_norm, inv_world, norm_coef, skip,
                       ema_state, decay, warmup);
    hipLaunchKernelGGL(optim_adamax_ema_kernel, dim3(nchunk), dim3(OPT_WG), 0, st, s, c, norm_coef, beta1, beta2, eps, write_grad, skip, ema,
                       (const float*)ema_state);
    return cvc_launch_status();
}

extern "C" int cvc_ema_swap(const cvc_optim_seg* segs, int nseg, const cvc_optim_chunk* chunks, int nchunk, float* const* ema,
                            cvc_stream_t stream) {
    if (!segs || !chunks || !ema || nseg < 1 || nchunk < 1) return CVC_E_BADARG;
    hipLaunchKernelGGL(ema_swap_kernel, dim3(nchunk), dim3(OPT_WG), 0, (hipStream_t)stream, reinterpret_cast<const OptSeg*>(segs),
                       reinterpret_cast<const OptChunk*>(chunks), ema);
    return cvc_launch_status();
}
