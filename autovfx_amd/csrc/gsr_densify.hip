// gsr_densify.hip -- the densification of the reference's training loops (scene/gaussian_model.py:339-417) without its boolean-mask
// round trips (include/gsr.h: gsr_densify_stats, gsr_densify_plan, gsr_densify_apply).
//
//   stats  add_densification_stats (:415-417): accum[i] += ||grad[i, :2]||, denom[i] += 1 where filter[i]; one launch.  Four
//          consecutive Gaussians per lane; a lane whose four filter bytes are all zero reads and writes nothing else.
//   plan   densify_and_prune (:399-413) as a classification of the N source rows -- kept original, kept clone, split parent -- and
//          three exclusive prefix sums that place them: classify + per-workgroup counts, one workgroup that scans the counts, a
//          scatter that ranks inside each workgroup with ballots.  No atomics, no spinning, nothing to zero-fill.
//   apply  one launch that writes every row of every output tensor: destination driven (row j of the result looks up where it
//          comes from), so stores are coalesced and, the plan being monotone inside each segment, loads nearly stream.
//
// Roundings are the ones PyTorch-ROCm's kernels make for the reference's expressions (gsr_device.h:183-193): torch.norm over a last
// dimension of 2 squares each element in a lane of its own and adds the two, so sqrt(fl(x*x) + fl(y*y)); exp / sigmoid are the
// device library's (torch_sigmoid); Python scalars arrive rounded to fp32 as a wrapped scalar is for an fp32 comparison.
// Defines the entry points gsr_densify_plan_scratch_bytes, gsr_densify_stats, gsr_densify_plan and gsr_densify_apply.
#include "gsr_internal.h"
#include "gsr_device.h"

namespace gsr {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRowsPerLane = 4;
constexpr uint32_t kMaxGrid = 2048;   // 256 CUs x 8 workgroups; more work is walked grid-stride
constexpr int kDensifyBlockRows = 1024;       // source rows per workgroup of the plan's classify / scatter kernels
static_assert(kDensifyBlockRows == kThreads * kRowsPerLane, "one lane classifies kRowsPerLane rows");
struct DensifyPlanArgs {   // gsr.h: gsr_densify_plan; passed by value
    int64_t n;
    const float *accum, *denom, *scaling, *opacity;
    float max_grad, dense_bound, min_opacity, ws_bound;
    int ws_test;
    int32_t *src_of, *split_idx, *counts;
    uint8_t* flags;                           // scratch: [n] class bits
    uint32_t *block_counts, *block_offsets;   // scratch: [3][blocks] each
    uint32_t blocks;
};
// Byte offsets of the regions of the plan's scratch (each 256-byte aligned); bytes = the whole.
struct DensifyPlanLayout {
    size_t flags, block_counts, block_offsets, bytes;
    uint32_t blocks;
};
inline DensifyPlanLayout densify_plan_layout(int64_t n) {
    DensifyPlanLayout l{};
    l.blocks = (uint32_t)((n + kDensifyBlockRows - 1) / kDensifyBlockRows);
    auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
    l.flags = 0;
    l.block_counts = up((size_t)n);
    l.block_offsets = l.block_counts + up((size_t)3 * l.blocks * sizeof(uint32_t));
    l.bytes = l.block_offsets + up((size_t)3 * l.blocks * sizeof(uint32_t));
    return l;
}
struct DensifyTensor {
    const float* src;
    float* dst;
    const float* side;   // the children's rows of this tensor ([2 n_split, floats_per_row]); null: copied from the parent
    int floats_per_row, is_moment;
};
struct DensifyApplyPlan {
    int64_t n_src, n_keep, n_front, n_out, n_split;
    const int32_t *src_of, *child_rows, *split_idx;
};
struct DensifyApplyBatch {   // passed by value (kernel arguments)
    DensifyTensor t[GSR_DENSIFY_MAX_TENSORS];
    uint64_t first_chunk[GSR_DENSIFY_MAX_TENSORS + 1];
    DensifyApplyPlan plan;
    int count;
};

// ---------------------------------------------------------------------------------------------------------------- stats
__device__ __forceinline__ void stats_row(bool on, float gx, float gy, float& accum, float& denom) {
    if (!on) return;
    accum = accum + sqrtf(gx * gx + gy * gy);
    denom = denom + 1.0f;
}
__device__ __forceinline__ float max_radius(float m, int r) {   // torch.max(m, float(r)): a NaN m stays
    const float f = (float)r;
    return m < f ? f : m;
}

__global__ __launch_bounds__(kThreads) void densify_stats_kernel(int64_t n, const float* __restrict__ grad, int row_floats,
                                                                const uint8_t* __restrict__ filter, float* __restrict__ accum,
                                                                float* __restrict__ denom, const int* __restrict__ radii,
                                                                float* __restrict__ max_radii, int vec) {
    const int64_t groups = (n + 3) / 4;
    for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kThreads) {
        const int64_t i = g * 4;
        if (vec && i + 4 <= n) {
            const uint32_t f = *reinterpret_cast<const uint32_t*>(filter + i);
            if (f == 0u) continue;
            float4 a = *reinterpret_cast<const float4*>(accum + i);
            float4 d = *reinterpret_cast<const float4*>(denom + i);
            float gx[4], gy[4];
            if (row_floats == 3) {   // twelve consecutive floats: three 16-byte loads
                const float4 q0 = *reinterpret_cast<const float4*>(grad + i * 3);
                const float4 q1 = *reinterpret_cast<const float4*>(grad + i * 3 + 4);
                const float4 q2 = *reinterpret_cast<const float4*>(grad + i * 3 + 8);
                gx[0] = q0.x; gy[0] = q0.y; gx[1] = q0.w; gy[1] = q1.x; gx[2] = q1.z; gy[2] = q1.w; gx[3] = q2.y; gy[3] = q2.z;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    gx[k] = grad[(i + k) * row_floats];
                    gy[k] = grad[(i + k) * row_floats + 1];
                }
            }
            stats_row((f & 0xFFu) != 0u, gx[0], gy[0], a.x, d.x);
            stats_row((f & 0xFF00u) != 0u, gx[1], gy[1], a.y, d.y);
            stats_row((f & 0xFF0000u) != 0u, gx[2], gy[2], a.z, d.z);
            stats_row((f & 0xFF000000u) != 0u, gx[3], gy[3], a.w, d.w);
            *reinterpret_cast<float4*>(accum + i) = a;
            *reinterpret_cast<float4*>(denom + i) = d;
            if (max_radii) {
                const int4 r = *reinterpret_cast<const int4*>(radii + i);
                float4 m = *reinterpret_cast<const float4*>(max_radii + i);
                if (f & 0xFFu) m.x = max_radius(m.x, r.x);
                if (f & 0xFF00u) m.y = max_radius(m.y, r.y);
                if (f & 0xFF0000u) m.z = max_radius(m.z, r.z);
                if (f & 0xFF000000u) m.w = max_radius(m.w, r.w);
                *reinterpret_cast<float4*>(max_radii + i) = m;
            }
        } else {
            for (int64_t j = i; j < i + 4 && j < n; ++j) {
                if (!filter[j]) continue;
                float a = accum[j], d = denom[j];
                stats_row(true, grad[j * row_floats], grad[j * row_floats + 1], a, d);
                accum[j] = a;
                denom[j] = d;
                if (max_radii) max_radii[j] = max_radius(max_radii[j], radii[j]);
            }
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------- plan
enum : uint32_t { kKeep = 1u, kClone = 2u, kSplit = 4u };

__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }   // torch.max: a NaN wins

// The class bits of source row i (gaussian_model.py:399-411 for thr > 0, DESIGN.md §7e points 1-5).
__device__ __forceinline__ uint32_t classify(const DensifyPlanArgs& p, int64_t i) {
    float g = p.accum[i] / p.denom[i];
    if (g != g) g = 0.0f;                                           // grads[grads.isnan()] = 0.0
    const float* s = p.scaling + i * 3;
    const float big = nan_max(nan_max(expf(s[0]), expf(s[1])), expf(s[2]));   // torch.max(get_scaling, dim=1).values
    const bool clone = sqrtf(g * g) >= p.max_grad && big <= p.dense_bound;   // torch.norm(grads, dim=-1) over one element
    const bool split = g >= p.max_grad && big > p.dense_bound;              // the padded gradient itself, not its norm
    bool pruned = torch_sigmoid(p.opacity[i]) < p.min_opacity;
    if (p.ws_test) pruned = pruned || big > p.ws_bound;             // max_radii2D was zeroed before: the screen-size test never fires
    return (!split && !pruned ? kKeep : 0u) | (clone && !pruned ? kClone : 0u) | (split ? kSplit : 0u);
}

__device__ __forceinline__ uint32_t popc64(unsigned long long m) { return (uint32_t)__popcll(m); }

// rows of a workgroup: blockIdx.x * 1024 + k * 256 + lane id, k = 0..3 -- ascending in (k, wave, lane)
__global__ __launch_bounds__(kThreads) void densify_classify_kernel(const DensifyPlanArgs p) {
    __shared__ uint32_t part[3][kWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t c[3] = {0u, 0u, 0u};
    for (int k = 0; k < kRowsPerLane; ++k) {
        const int64_t i = (int64_t)blockIdx.x * kDensifyBlockRows + k * kThreads + threadIdx.x;
        uint32_t f = 0u;
        if (i < p.n) {
            f = classify(p, i);
            p.flags[i] = (uint8_t)f;
        }
        c[0] += popc64(__ballot(f & kKeep));
        c[1] += popc64(__ballot(f & kClone));
        c[2] += popc64(__ballot(f & kSplit));
    }
    if (lane == 0) {
        part[0][wave] = c[0];
        part[1][wave] = c[1];
        part[2][wave] = c[2];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        uint32_t s = 0u;
        for (int w = 0; w < kWaves; ++w) s += part[threadIdx.x][w];
        p.block_counts[(size_t)threadIdx.x * p.blocks + blockIdx.x] = s;
    }
}

// one workgroup: exclusive prefix of each class's per-workgroup counts, and the three totals
__global__ __launch_bounds__(kThreads) void densify_scan_kernel(const DensifyPlanArgs p) {
    __shared__ uint32_t s_wave[kWaves];
    for (int cls = 0; cls < 3; ++cls) {
        const uint32_t* in = p.block_counts + (size_t)cls * p.blocks;
        uint32_t* out = p.block_offsets + (size_t)cls * p.blocks;
        uint32_t carry = 0u;   // the class's counts in front of this round (the same in every lane)
        for (uint32_t base = 0; base < p.blocks; base += kThreads) {
            const uint32_t b = base + threadIdx.x;
            uint32_t round_total;
            const uint32_t before = carry + block_exclusive_scan<kWaves>(b < p.blocks ? in[b] : 0u, s_wave, &round_total);
            if (b < p.blocks) out[b] = before;
            carry += round_total;
        }
        if (threadIdx.x == 0) p.counts[cls] = (int32_t)carry;
    }
    if (threadIdx.x == 0) p.counts[3] = 0;
}

__global__ __launch_bounds__(kThreads) void densify_scatter_kernel(const DensifyPlanArgs p) {
    __shared__ uint32_t cnt[3][kRowsPerLane][kWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t f[kRowsPerLane], rank[kRowsPerLane][3];
    for (int k = 0; k < kRowsPerLane; ++k) {
        const int64_t i = (int64_t)blockIdx.x * kDensifyBlockRows + k * kThreads + threadIdx.x;
        f[k] = i < p.n ? (uint32_t)p.flags[i] : 0u;
        for (int cls = 0; cls < 3; ++cls) {
            const unsigned long long m = __ballot(f[k] & (1u << cls));
            rank[k][cls] = popc64(m & below);
            if (lane == 0) cnt[cls][k][wave] = popc64(m);
        }
    }
    __syncthreads();
    const uint32_t kept = (uint32_t)p.counts[0];   // the clones follow the kept originals in src_of
    for (int cls = 0; cls < 3; ++cls) {
        uint32_t at = p.block_offsets[(size_t)cls * p.blocks + blockIdx.x];
        for (int k = 0; k < kRowsPerLane; ++k) {
            for (int w = 0; w < kWaves; ++w) {
                if (w == wave && (f[k] & (1u << cls))) {
                    const uint32_t i = (uint32_t)((int64_t)blockIdx.x * kDensifyBlockRows + k * kThreads + threadIdx.x);
                    const uint32_t pos = at + rank[k][cls];
                    if (cls == 0) p.src_of[pos] = (int32_t)i;
                    else if (cls == 1) p.src_of[kept + pos] = (int32_t)i;
                    else p.split_idx[pos] = (int32_t)i;
                }
                at += cnt[cls][k][w];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- apply
constexpr int kApplyUnroll = 8;
constexpr int64_t kApplyChunk = (int64_t)kThreads * kApplyUnroll;   // output floats per workgroup iteration of the apply kernel

// The value of element (row, col) of output tensor T.  Rows [0, n_keep) are kept originals, [n_keep, n_front) clones, the rest
// children: child_rows gives the child's row in the side tensors ([2S, ...], copy-major), its parent is split_idx[that mod S].
template <int FPR>
__device__ __forceinline__ float apply_element(const DensifyTensor& T, const DensifyApplyPlan& P, int64_t row, int col, int fpr_rt) {
    const int fpr = FPR > 0 ? FPR : fpr_rt;
    if (row < P.n_front) {
        if (T.is_moment && row >= P.n_keep) return 0.0f;
        const uint32_t s = (uint32_t)P.src_of[row];
        return s < (uint32_t)P.n_src ? T.src[(int64_t)s * fpr + col] : 0.0f;
    }
    if (T.is_moment) return 0.0f;
    const uint32_t c = (uint32_t)P.child_rows[row - P.n_front];
    if (c >= (uint32_t)(2 * P.n_split)) return 0.0f;
    if (T.side) return T.side[(int64_t)c * fpr + col];
    const uint32_t s = (uint32_t)P.split_idx[c >= (uint32_t)P.n_split ? c - (uint32_t)P.n_split : c];
    return s < (uint32_t)P.n_src ? T.src[(int64_t)s * fpr + col] : 0.0f;
}

template <int FPR>
__device__ __forceinline__ void apply_chunk(const DensifyTensor& T, const DensifyApplyPlan& P, int64_t begin, int64_t total) {
    const int fpr = FPR > 0 ? FPR : T.floats_per_row;
    const int64_t row0 = begin / fpr;
    const uint32_t col0 = (uint32_t)(begin - row0 * fpr);
    float v[kApplyUnroll];
#pragma unroll
    for (int u = 0; u < kApplyUnroll; ++u) {
        const uint32_t local = (uint32_t)(u * kThreads) + threadIdx.x;
        const uint32_t at = col0 + local;
        v[u] = begin + local < total ? apply_element<FPR>(T, P, row0 + at / (uint32_t)fpr, (int)(at % (uint32_t)fpr), fpr) : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < kApplyUnroll; ++u) {
        const uint32_t local = (uint32_t)(u * kThreads) + threadIdx.x;
        if (begin + local < total) T.dst[begin + local] = v[u];
    }
}

__global__ __launch_bounds__(kThreads) void densify_apply_kernel(const DensifyApplyBatch b) {
    const uint64_t total_chunks = b.first_chunk[b.count];
    for (uint64_t chunk = blockIdx.x; chunk < total_chunks; chunk += gridDim.x) {
        int t = 0;
        while (chunk >= b.first_chunk[t + 1]) ++t;
        const DensifyTensor& T = b.t[t];
        const int64_t begin = (int64_t)(chunk - b.first_chunk[t]) * kApplyChunk;
        const int64_t total = b.plan.n_out * T.floats_per_row;
        switch (T.floats_per_row) {   // the reference's row widths get a constant divisor
            case 1: apply_chunk<1>(T, b.plan, begin, total); break;
            case 3: apply_chunk<3>(T, b.plan, begin, total); break;
            case 4: apply_chunk<4>(T, b.plan, begin, total); break;
            case 45: apply_chunk<45>(T, b.plan, begin, total); break;
            default: apply_chunk<0>(T, b.plan, begin, total); break;
        }
    }
}

hipError_t launch_densify_stats(int64_t n, const float* grad, int row_floats, const uint8_t* filter, float* accum, float* denom,
                                const int* radii, float* max_radii, hipStream_t stream) {
    const uintptr_t any = (uintptr_t)grad | (uintptr_t)accum | (uintptr_t)denom | (uintptr_t)radii | (uintptr_t)max_radii;
    const int vec = (any & 15u) == 0u && ((uintptr_t)filter & 3u) == 0u ? 1 : 0;
    const int64_t blocks = ((n + 3) / 4 + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(densify_stats_kernel, dim3((uint32_t)(blocks < (int64_t)kMaxGrid * 4 ? blocks : (int64_t)kMaxGrid * 4)), dim3(kThreads), 0,
                       stream, n, grad, row_floats, filter, accum, denom, radii, max_radii, vec);
    return hipGetLastError();
}

hipError_t launch_densify_plan(const DensifyPlanArgs& p, hipStream_t stream) {
    hipLaunchKernelGGL(densify_classify_kernel, dim3(p.blocks), dim3(kThreads), 0, stream, p);
    hipLaunchKernelGGL(densify_scan_kernel, dim3(1), dim3(kThreads), 0, stream, p);
    hipLaunchKernelGGL(densify_scatter_kernel, dim3(p.blocks), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_densify_apply(const DensifyApplyBatch& b, hipStream_t stream) {
    const uint64_t total = b.first_chunk[b.count];
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(densify_apply_kernel, dim3((uint32_t)(total < kMaxGrid * 8ull ? total : kMaxGrid * 8ull)), dim3(kThreads), 0, stream, b);
    return hipGetLastError();
}

}  // namespace
}  // namespace gsr

using gsr::aligned4;
using gsr::fail;

extern "C" {

size_t gsr_densify_plan_scratch_bytes(int64_t n) {
    return n <= 0 || n >= (int64_t(1) << 31) ? 0 : gsr::densify_plan_layout(n).bytes;
}

int gsr_densify_stats(int64_t n, const float* grad, int grad_row_floats, const uint8_t* filter, float* accum, float* denom,
                      const int32_t* radii, float* max_radii, void* stream_) {
    if (n < 0 || n >= (int64_t(1) << 31)) return fail(GSR_ERR_INVALID_ARG, "gsr_densify_stats: n = %lld outside [0, 2^31)", (long long)n);
    if (grad_row_floats < 2) return fail(GSR_ERR_INVALID_ARG, "gsr_densify_stats: grad_row_floats = %d < 2", grad_row_floats);
    if (n == 0) return GSR_OK;
    if (!grad || !filter || !accum || !denom || (radii == nullptr) != (max_radii == nullptr))
        return fail(GSR_ERR_INVALID_ARG, "gsr_densify_stats: null pointer (radii and max_radii go together)");
    if (!aligned4(grad) || !aligned4(accum) || !aligned4(denom) || !aligned4(radii) || !aligned4(max_radii))
        return fail(GSR_ERR_INVALID_ARG, "gsr_densify_stats: misaligned pointer (4 bytes)");
    GSR_HIP(gsr::launch_densify_stats(n, grad, grad_row_floats, filter, accum, denom, radii, max_radii, (hipStream_t)stream_));
    return GSR_OK;
}

int gsr_densify_plan(int64_t n, const float* accum, const float* denom, const float* scaling, const float* opacity, float max_grad,
                     float dense_bound, float min_opacity, int ws_test, float ws_bound, int32_t* src_of, int32_t* split_idx,
                     int32_t* counts, void* scratch, size_t scratch_bytes, void* stream_) {
    if (n < 0 || n >= (int64_t(1) << 31)) return fail(GSR_ERR_INVALID_ARG, "gsr_densify_plan: n = %lld outside [0, 2^31)", (long long)n);
    if (n == 0) return GSR_OK;
    if (!accum || !denom || !scaling || !opacity || !src_of || !split_idx || !counts || !scratch)
        return fail(GSR_ERR_INVALID_ARG, "gsr_densify_plan: null pointer");
    if (!aligned4(accum) || !aligned4(denom) || !aligned4(scaling) || !aligned4(opacity) || !aligned4(src_of) || !aligned4(split_idx) ||
        !aligned4(counts) || !gsr::aligned256(scratch))
        return fail(GSR_ERR_INVALID_ARG, "gsr_densify_plan: misaligned pointer (arrays: 4 bytes, scratch: 256 bytes)");
    const gsr::DensifyPlanLayout l = gsr::densify_plan_layout(n);
    if (scratch_bytes < l.bytes) return fail(GSR_ERR_INVALID_ARG, "gsr_densify_plan: scratch too small (%zu of %zu bytes)", scratch_bytes, l.bytes);
    char* base = (char*)scratch;
    gsr::DensifyPlanArgs p{n, accum, denom, scaling, opacity, max_grad, dense_bound, min_opacity, ws_bound, ws_test ? 1 : 0, src_of, split_idx,
                           counts, (uint8_t*)(base + l.flags), (uint32_t*)(base + l.block_counts), (uint32_t*)(base + l.block_offsets), l.blocks};
    GSR_HIP(gsr::launch_densify_plan(p, (hipStream_t)stream_));
    return GSR_OK;
}

int gsr_densify_apply(const GsrDensifyTensor* tensors, int count, const GsrDensifyPlan* plan, void* stream_) {
    if (count <= 0 || count > GSR_DENSIFY_MAX_TENSORS)
        return fail(GSR_ERR_INVALID_ARG, "gsr_densify_apply: bad count %d (1..%d)", count, GSR_DENSIFY_MAX_TENSORS);
    if (!tensors || !plan) return fail(GSR_ERR_INVALID_ARG, "gsr_densify_apply: null tensors or plan");
    const GsrDensifyPlan& P = *plan;
    const int64_t lim = int64_t(1) << 31;
    if (P.n_src < 0 || P.n_src >= lim || P.n_split < 0 || P.n_split > P.n_src || P.n_keep < 0 || P.n_keep > P.n_front || P.n_front > P.n_out ||
        P.n_out >= lim || P.n_out - P.n_front > 2 * P.n_split)
        return fail(GSR_ERR_INVALID_ARG, "gsr_densify_apply: bad sizes (n_src %lld, n_keep %lld, n_front %lld, n_out %lld, n_split %lld)",
                    (long long)P.n_src, (long long)P.n_keep, (long long)P.n_front, (long long)P.n_out, (long long)P.n_split);
    if (P.n_out == 0) return GSR_OK;
    if ((P.n_front > 0 && !P.src_of) || (P.n_out > P.n_front && (!P.child_rows || !P.split_idx)))
        return fail(GSR_ERR_INVALID_ARG, "gsr_densify_apply: null index array");
    if (!aligned4(P.src_of) || !aligned4(P.child_rows) || !aligned4(P.split_idx))
        return fail(GSR_ERR_INVALID_ARG, "gsr_densify_apply: misaligned index array (4 bytes)");
    gsr::DensifyApplyBatch b{};
    b.count = count;
    b.plan = {P.n_src, P.n_keep, P.n_front, P.n_out, P.n_split, P.src_of, P.child_rows, P.split_idx};
    for (int i = 0; i < count; ++i) {
        const GsrDensifyTensor& t = tensors[i];
        if (t.floats_per_row < 0 || (int64_t)t.floats_per_row * P.n_out >= (int64_t(1) << 40))
            return fail(GSR_ERR_INVALID_ARG, "gsr_densify_apply: tensor %d: floats_per_row %d", i, (int)t.floats_per_row);
        if (t.floats_per_row > 0 && (!t.dst || (!t.src && !(t.is_moment && P.n_keep == 0) && P.n_src > 0)))
            return fail(GSR_ERR_INVALID_ARG, "gsr_densify_apply: tensor %d: null pointer", i);
        if (!aligned4(t.src) || !aligned4(t.dst) || !aligned4(t.side))
            return fail(GSR_ERR_INVALID_ARG, "gsr_densify_apply: tensor %d: misaligned pointer (4 bytes)", i);
        b.t[i] = {t.src, t.dst, t.side, t.floats_per_row, t.is_moment ? 1 : 0};
        const int64_t floats = (int64_t)t.floats_per_row * P.n_out;
        b.first_chunk[i + 1] = b.first_chunk[i] + (uint64_t)((floats + gsr::kApplyChunk - 1) / gsr::kApplyChunk);
    }
    GSR_HIP(gsr::launch_densify_apply(b, (hipStream_t)stream_));
    return GSR_OK;
}

}  // extern "C"
