// Ensemble decoding: M members' logit rows -> one row of combined log-probs, one workgroup per row (DESIGN.md section 7,
// "Ensemble decoding").  The launch between the members' steps and the ONE selection block of an ensemble's step
// (cvc/decode/ensemble.py): the block then runs on `out` with nparts = 1, bias = NULL.
//
//   x_m[r, :]  = member m's logits: its slabs summed by the selection blocks' row loader (csrc/select_row.h: slab 0 + slab 1 + ...
//                + bias) -- the bits that member's own selection block would see
//   lse_m[r]   = max + logf(sum_v expf(x_m[r, v] - max))                      block_max / block_sum of csrc/row_block.h
//   a_m[v]     = (x_m[r, v] - lse_m) + logw[m]
//   geometric == 0:  acc_0 = a_0,  acc_m = fmaxf(acc_{m-1}, a_m) + log1pf(expf(-fabsf(acc_{m-1} - a_m))),  out[r, v] = acc_{M-1}
//                    = log sum_m w_m p_m(v): normalised.  A streaming log-sum-exp over the members: logf(sum_m w_m expf(a_m)) would
//                    be -inf for a word ~87 nats below the top of every member's row, and the forced mode scores such words.
//   geometric == 1:  out[r, v] = sum_m expf(logw[m]) * (x_m[r, v] - lse_m), member order: unnormalised (the selection blocks take
//                    their own log-sum-exp)
//
// fp32 throughout, members in index order, contract(off).  The row of the current member and the accumulator live in registers (two
// NC-arrays; the build refuses scratch: build_hip.py); the M descriptors and log-weights travel by value in the kernel's arguments
// (no device table, no workspace, no atomics): capturable, bitwise deterministic.  The members' slab counts differ, so the loader
// runs in its run-time nparts form (NP = 0: the same order of the slab sum, the same bits as the unrolled forms).
//
// cvc_ensemble_mix: out[i] = sum_m expf(logw[m]) * src_m[i], member order -- the ensemble's region attention.
#include "select_row.h"
#include <math.h>

namespace {

struct EnsembleArgs {
    cvc_ensemble_src src[CVC_ENSEMBLE_MAX];
    float logw[CVC_ENSEMBLE_MAX];
};

template <int NC, bool VEC>
__global__ __launch_bounds__(WG) void ensemble_logprobs_kernel(const EnsembleArgs args, int M, int geometric, int V, float* out,
                                                               int ld_out) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    float z[NC], acc[NC];
    for (int m = 0; m < M; ++m) {
        const cvc_ensemble_src s = args.src[m];
        // (V made opaque per member: the loader's NC column tests `v < V` are otherwise hoisted out of this loop as NC lane masks
        // held in scalar registers, more than there are at NC = 32; a compare per column and member costs nothing)
        int Vm = V;
        asm volatile("" : "+s"(Vm));
        load_logit_row<NC, 0, VEC>(s.parts + (size_t)row * V, s.nparts, s.part_stride, s.bias, Vm, tid, z);
        float mx = -INFINITY;
#pragma unroll
        for (int u = 0; u < NC; ++u) mx = fmaxf(mx, z[u]);
        mx = block_max(mx, red);
        float se = 0.f;
#pragma unroll
        for (int u = 0; u < NC; ++u) se += expf(z[u] - mx);              // padding: exp(-inf) = 0
        const float lse = mx + logf(block_sum(se, red));
        const float lw = args.logw[m];
        if (geometric) {
            const float wn = expf(lw);
#pragma unroll
            for (int u = 0; u < NC; ++u) {
                const float a = wn * (z[u] - lse);
                acc[u] = m == 0 ? a : acc[u] + a;
            }
        } else {
#pragma unroll
            for (int u = 0; u < NC; ++u) {
                const float a = (z[u] - lse) + lw;
                acc[u] = m == 0 ? a : fmaxf(acc[u], a) + log1pf(expf(-fabsf(acc[u] - a)));
            }
        }
    }
    float* o = out + (size_t)row * ld_out;
    if constexpr (VEC) {
#pragma unroll
        for (int g = 0; g < NC / 4; ++g) {
            const int e = (tid + g * WG) * 4;
            if (e < V) st4(o + e, f32x4{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]});     // V % 4 == 0
        }
    } else {
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            const int v = col<false>(tid, u);
            if (v < V) o[v] = acc[u];
        }
    }
}

struct MixArgs {
    const float* src[CVC_ENSEMBLE_MAX];
    float logw[CVC_ENSEMBLE_MAX];
};

__global__ __launch_bounds__(WG) void ensemble_mix_kernel(const MixArgs args, int M, long long n, float* out) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    float acc = expf(args.logw[0]) * args.src[0][i];
    for (int m = 1; m < M; ++m) acc = acc + expf(args.logw[m]) * args.src[m][i];
    out[i] = acc;
}

bool finite_weights(const float* logw, int M) {
    for (int m = 0; m < M; ++m)
        if (!isfinite(logw[m])) return false;
    return true;
}

}  // namespace

extern "C" int cvc_ensemble_logprobs(const cvc_ensemble_src* src, int M, const float* logw, int geometric, int rows, int V, float* out,
                                     int ld_out, cvc_stream_t stream) {
    if (!src || !logw || !out || M < 1 || M > CVC_ENSEMBLE_MAX || ld_out < V) return CVC_E_BADARG;
    if (!finite_weights(logw, M)) return CVC_E_BADARG;
    EnsembleArgs args = {};
    bool vec = (ld_out & 3) == 0 && ((uintptr_t)out & 15) == 0;
    for (int m = 0; m < M; ++m) {
        const cvc_ensemble_src& s = src[m];
        // the selection blocks' shared checks, per member (the word pointer is theirs: `out` stands in, it is not read)
        const int rc = select_row_check(s.parts, s.nparts, s.part_stride, rows, V, (const int64_t*)out, 1);
        if (rc != 0) return rc;
        vec = vec && (V & 3) == 0 && ((uintptr_t)s.parts & 15) == 0 && (s.nparts == 1 || (s.part_stride & 3) == 0) &&
              ((uintptr_t)s.bias & 15) == 0;                             // select_dispatch's vector conditions
        args.src[m] = s;
        args.logw[m] = logw[m];
    }
    // NC as every selection block chooses it; the float4 form only when every member and `out` allow it: select_dispatch decides
    // from the operand it is shown (never dereferenced there) -- `out` when all are aligned, a misaligned address otherwise
    select_dispatch(vec ? out : reinterpret_cast<const float*>(uintptr_t(4)), 1, 0, nullptr, V, [&](auto nc, auto, auto isvec) {
        hipLaunchKernelGGL((ensemble_logprobs_kernel<decltype(nc)::value, decltype(isvec)::value>), dim3(rows), dim3(WG), 0,
                           (hipStream_t)stream, args, M, geometric, V, out, ld_out);
    });
    return cvc_launch_status();
}

extern "C" int cvc_ensemble_mix(const float* const* src, int M, const float* logw, long long n, float* out, cvc_stream_t stream) {
    if (!src || !logw || !out || M < 1 || M > CVC_ENSEMBLE_MAX || n < 1 || n > 0x7fffffffLL * WG) return CVC_E_BADARG;
    if (!finite_weights(logw, M)) return CVC_E_BADARG;
    MixArgs args = {};
    for (int m = 0; m < M; ++m) {
        if (!src[m]) return CVC_E_BADARG;
        args.src[m] = src[m];
        args.logw[m] = logw[m];
    }
    hipLaunchKernelGGL(ensemble_mix_kernel, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, (hipStream_t)stream, args, M, n, out);
    return cvc_launch_status();
}
