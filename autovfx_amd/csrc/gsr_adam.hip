// gsr_adam.hip -- one Adam step over every tensor of an optimizer, in one launch (include/gsr.h: gsr_adam_step).
// Defines the entry point gsr_adam_step.
//
// The update is torch.optim.Adam's default path on a GPU (torch/optim/adam.py, _multi_tensor_adam, amsgrad / maximize / weight decay
// off), whose foreach ops run one after the other over the whole tensor list:
//   _foreach_lerp_(m, g, 1 - beta1)  _foreach_mul_(v, beta2)  _foreach_addcmul_(v, g, g, 1 - beta2)  d = _foreach_sqrt(v)
//   _foreach_div_(d, sqrt(1 - beta2^t))  _foreach_add_(d, eps)  _foreach_addcdiv_(p, m, d, -lr / (1 - beta1^t))
// Here the same arithmetic runs per element, each op rounded to fp32 as ATen's foreach kernels round it (opmath = float, the Python
// scalars converted to float first):
//   1. m = m + w (g - m)                     w = fl(1 - beta1) < 0.5   (ATen's lerp for a small weight; its other branch,
//                                                                        beta1 <= 0.5, is refused and left to torch)
//   2. v = v b2,  v = v + c (g g)            b2 = fl(beta2), c = fl(1 - beta2)
//   3. d = sqrt(v) / s2 + eps                correctly rounded sqrt and divide, s2 = fl(sqrt(1 - beta2^t)), eps = fl(eps)
//   4. p = p + a (m / d)                     a = fl(-lr / (1 - beta1^t))
// ATen's ROCm build compiles those functors with clang's default contraction, so each `x + y * z` of steps 1, 2 and 4 is ONE fma:
// tests/test_adam_gpu.py (test_foreach_ops_fuse_the_multiply_add) compares _foreach_lerp_ / _foreach_addcmul_ / _foreach_addcdiv_
// against both forms and asserts the fused one, the form written below with __builtin_fmaf (the library is built with
// -ffp-contract=off, so nothing else is fused).  Denormals are kept: v reaches them for tiny gradients.
//
// Work split: a 4096-element chunk per workgroup iteration (256 lanes x 4 x 16-byte nontemporal loads of each of p, g, m, v: 16 loads
// in flight per lane), chunks numbered through all tensors, the tensor of a chunk found from the per-tensor prefix (at most 16 entries,
// uniform across the workgroup), the grid capped and walked grid-stride.  A tensor whose four pointers are all 16-byte aligned takes
// the vector path for its full chunks; its last chunk, and every chunk of a tensor with a misaligned pointer, go one element per lane
// (coalesced 4-byte accesses).  Each element is read and written by one lane: no atomics, no scratch, no host synchronisation.
#include "gsr_internal.h"

namespace gsr {
namespace {

constexpr int kThreads = 256;
constexpr int kVec = 4;      // floats per 16-byte access
constexpr int kUnroll = 4;   // 16-byte accesses per lane and array per chunk
constexpr int64_t kChunk = (int64_t)kThreads * kVec * kUnroll;
constexpr uint32_t kMaxGrid = 2048;   // 256 CUs x 8 workgroups; more chunks are walked grid-stride
static_assert(kChunk == 4096, "DESIGN.md §7d");

struct AdamTensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t numel;
    float a, s2;      // gsr.h: GsrAdamTensor::step_size, ::bias2_sqrt
    int aligned16;    // p, g, m and v all 16-byte aligned
};
struct AdamBatch {    // passed by value (kernel arguments)
    AdamTensor t[GSR_ADAM_MAX_TENSORS];
    uint64_t first_chunk[GSR_ADAM_MAX_TENSORS + 1];   // prefix of adam_chunks(numel); first_chunk[count] = the total
    int count;
    float w, b2, c, eps;
};

// 16-byte nontemporal load (the builtin wants a native vector type).  Measured on C3 groups, same process, alternated, three
// orders: nontemporal loads 2-10 % faster than plain ones in every order; nontemporal stores changed places with
// plain ones between orders; both together 6-10 % slower.  So: nontemporal loads, plain stores.
typedef float native4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 load_nt(const float* q) {
    const native4 x = __builtin_nontemporal_load(reinterpret_cast<const native4*>(q));
    return make_float4(x.x, x.y, x.z, x.w);
}

struct Scalars {
    float w, b2, c, eps;
};

__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float a, float s2, const Scalars& k) {
    const float diff = g - m;
    m = __builtin_fmaf(k.w, diff, m);
    v = v * k.b2;
    v = __builtin_fmaf(k.c, g * g, v);
    float d = __builtin_sqrtf(v);
    d = d / s2;
    d = d + k.eps;
    p = __builtin_fmaf(a, m / d, p);
}

__device__ __forceinline__ void adam_float4(float4& p, const float4& g, float4& m, float4& v, float a, float s2, const Scalars& k) {
    adam_element(p.x, g.x, m.x, v.x, a, s2, k);
    adam_element(p.y, g.y, m.y, v.y, a, s2, k);
    adam_element(p.z, g.z, m.z, v.z, a, s2, k);
    adam_element(p.w, g.w, m.w, v.w, a, s2, k);
}

__global__ __launch_bounds__(kThreads) void adam_step_kernel(const AdamBatch b) {
    const Scalars k{b.w, b.b2, b.c, b.eps};
    const uint64_t total = b.first_chunk[b.count];
    for (uint64_t chunk = blockIdx.x; chunk < total; chunk += gridDim.x) {
        int t = 0;
        while (chunk >= b.first_chunk[t + 1]) ++t;
        const AdamTensor& T = b.t[t];
        const int64_t begin = (int64_t)(chunk - b.first_chunk[t]) * kChunk;
        const int64_t n = min(kChunk, T.numel - begin);
        float* __restrict__ p = T.p + begin;
        const float* __restrict__ g = T.g + begin;
        float* __restrict__ m = T.m + begin;
        float* __restrict__ v = T.v + begin;
        if (T.aligned16 && n == kChunk) {
            float4 P[kUnroll], G[kUnroll], M[kUnroll], V[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int i = (u * kThreads + (int)threadIdx.x) * kVec;
                P[u] = load_nt(p + i);
                G[u] = load_nt(g + i);
                M[u] = load_nt(m + i);
                V[u] = load_nt(v + i);
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int i = (u * kThreads + (int)threadIdx.x) * kVec;
                adam_float4(P[u], G[u], M[u], V[u], T.a, T.s2, k);
                *reinterpret_cast<float4*>(p + i) = P[u];
                *reinterpret_cast<float4*>(m + i) = M[u];
                *reinterpret_cast<float4*>(v + i) = V[u];
            }
        } else {
            for (int i = (int)threadIdx.x; i < (int)n; i += kThreads) {
                float pi = p[i], mi = m[i], vi = v[i];
                adam_element(pi, g[i], mi, vi, T.a, T.s2, k);
                p[i] = pi;
                m[i] = mi;
                v[i] = vi;
            }
        }
    }
}

uint64_t adam_chunks(int64_t numel) { return (uint64_t)((numel + kChunk - 1) / kChunk); }   // numel >= 0

hipError_t launch_adam_step(const AdamBatch& b, hipStream_t stream) {
    const uint64_t total = b.first_chunk[b.count];
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(adam_step_kernel, dim3((uint32_t)(total < kMaxGrid ? total : kMaxGrid)), dim3(kThreads), 0, stream, b);
    return hipGetLastError();
}

}  // namespace
}  // namespace gsr

using gsr::aligned4;
using gsr::fail;

extern "C" {

int gsr_adam_step(const GsrAdamTensor* tensors, int count, float w, float b2, float c, float eps, void* stream_) {
    if (count <= 0 || count > GSR_ADAM_MAX_TENSORS)
        return fail(GSR_ERR_INVALID_ARG, "gsr_adam_step: bad count %d (1..%d)", count, GSR_ADAM_MAX_TENSORS);
    if (!tensors) return fail(GSR_ERR_INVALID_ARG, "gsr_adam_step: null tensors");
    if (!(w >= 0.0f && w < 0.5f)) return fail(GSR_ERR_INVALID_ARG, "gsr_adam_step: w = %g outside [0, 0.5) (ATen's small-weight lerp)", (double)w);
    gsr::AdamBatch b{};
    b.count = count;
    b.w = w;
    b.b2 = b2;
    b.c = c;
    b.eps = eps;
    for (int i = 0; i < count; ++i) {
        const GsrAdamTensor& t = tensors[i];
        if (t.numel < 0) return fail(GSR_ERR_INVALID_ARG, "gsr_adam_step: tensor %d: numel %lld < 0", i, (long long)t.numel);
        if (t.numel > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq))
            return fail(GSR_ERR_INVALID_ARG, "gsr_adam_step: tensor %d: null pointer", i);
        if (!aligned4(t.param) || !aligned4(t.grad) || !aligned4(t.exp_avg) || !aligned4(t.exp_avg_sq))
            return fail(GSR_ERR_INVALID_ARG, "gsr_adam_step: tensor %d: misaligned pointer (4 bytes)", i);
        const uintptr_t any = (uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq;
        b.t[i] = {t.param, t.grad, t.exp_avg, t.exp_avg_sq, t.numel, t.step_size, t.bias2_sqrt, (any & 15u) == 0u ? 1 : 0};
        b.first_chunk[i + 1] = b.first_chunk[i] + gsr::adam_chunks(t.numel);   // numel == 0: no chunk, skipped
    }
    GSR_HIP(gsr::launch_adam_step(b, (hipStream_t)stream_));
    return GSR_OK;
}

}  // extern "C"
