// gsr_tree.hip -- the two steps of a box tree's build that do not look at the records (gsr_internal.h: morton_sort, tree_levels): the
// sort of the 63-bit Morton codes and the box levels above the leaves.  gsr_knn.hip builds its tree over points with them,
// gsr_meshquery.hip its plan over triangles; the trees' shape and the helpers of both are in gsr_tree.h.
#include "gsr_tree.h"

namespace gsr {
namespace {

// the high words in the order of the first sort (by the low words), for the second
__global__ __launch_bounds__(256) void tree_gather_kernel(uint32_t n, const uint32_t* __restrict__ order, const uint32_t* __restrict__ key_hi,
                                                          uint32_t* __restrict__ out) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s < n) out[s] = key_hi[order[s]];
}

__global__ __launch_bounds__(256) void tree_level_kernel(uint32_t n_parents, uint32_t n_children, const float4* __restrict__ children,
                                                         float4* __restrict__ parents) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n_parents) return;
    float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.0f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
    const uint32_t end = min(n_children, (p + 1) * kFan);
    for (uint32_t c = p * kFan; c < end; ++c) {
        const float4 a = children[2 * (size_t)c], b = children[2 * (size_t)c + 1];
        lo.x = fminf(lo.x, a.x); lo.y = fminf(lo.y, a.y); lo.z = fminf(lo.z, a.z);
        hi.x = fmaxf(hi.x, b.x); hi.y = fmaxf(hi.y, b.y); hi.z = fmaxf(hi.z, b.z);
    }
    parents[2 * (size_t)p] = lo;
    parents[2 * (size_t)p + 1] = hi;
}

}  // namespace

hipError_t morton_sort(uint32_t* radix, uint32_t n, uint32_t* keys, uint32_t* keys_alt, uint32_t* vals, uint32_t* vals_alt,
                       const uint32_t* key_hi, uint32_t** order, hipStream_t stream) {
    uint32_t *ks = nullptr, *vs = nullptr;
    hipError_t e = radix_sort_pairs(radix, n, 32, keys, keys_alt, vals, vals_alt, true, false, &ks, &vs, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tree_gather_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, (const uint32_t*)vs, key_hi, keys);
    return radix_sort_pairs(radix, n, 32, keys, keys_alt, vs, vs == vals ? vals_alt : vals, false, false, &ks, order, stream);
}

hipError_t tree_levels(float4* boxes, uint32_t leaves, int top, hipStream_t stream) {
    for (int level = 1; level <= top; ++level) {
        uint32_t below, below_at, count, offset;
        tree_level(leaves, level - 1, below, below_at);
        tree_level(leaves, level, count, offset);
        hipLaunchKernelGGL(tree_level_kernel, dim3((count + 255u) / 256u), dim3(256), 0, stream, count, below,
                           (const float4*)(boxes + 2 * (size_t)below_at), boxes + 2 * (size_t)offset);
    }
    return hipGetLastError();
}

}  // namespace gsr
