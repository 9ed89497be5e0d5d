// gsr_tree.h -- what the box trees over Morton-sorted records share: the points of gsr_knn.hip, the triangles of gsr_meshquery.hip.
// The shape of a tree, its level arithmetic and the wave, box and Morton-code helpers of the builds and the walks.  The two kernels
// and the two host steps that both builds run unchanged are in gsr_tree.hip (declared in gsr_internal.h: morton_sort, tree_levels).
#pragma once

#include "gsr_internal.h"
#include "gsr_wave.h"

namespace gsr {

// Boxes over the Morton-sorted records: level 0 = leaves of 64 records, every level above = 16 boxes of the one below, up to the
// first level of at most 16 boxes (`top`; six levels for n < 2^30).  A box is two float4 (lo, hi; w unused) at
// boxes[2 * (offset of its level + i)].
constexpr int kTreeMaxLevels = 6;
constexpr int kLeaf = 64;            // records per leaf: one wave
constexpr int kFan = 16;             // children per box above the leaves
constexpr int kStackDepth = 96;      // of a walk's stack: >= kFan + (kFan - 1) * (kTreeMaxLevels - 1)
constexpr int kBoundsBlocks = 128;   // partial bounds
constexpr uint32_t kCellMax = (1u << 21) - 1u;   // 21 bits per axis: a 63-bit Morton code, sorted as two 32-bit words
constexpr size_t kAlign = 256;
static_assert(kStackDepth >= kFan + (kFan - 1) * (kTreeMaxLevels - 1), "stack too shallow for the tree");

__host__ __device__ inline size_t align_up(size_t v) { return (v + kAlign - 1) & ~(kAlign - 1); }

// The tree over n records: pure arithmetic, the same on the host that sizes it and in a kernel that reads it.
struct TreeShape {
    uint32_t leaves, boxes;   // boxes: of all levels
    int top;
};
__host__ __device__ inline TreeShape tree_shape(uint32_t n) {
    TreeShape t = {};
    t.leaves = (n + kLeaf - 1) / kLeaf;
    uint32_t count = t.leaves;
    t.boxes = count;
    while (count > (uint32_t)kFan && t.top + 1 < kTreeMaxLevels) {
        count = (count + kFan - 1) / kFan;
        t.boxes += count;
        ++t.top;
    }
    return t;
}
// boxes of `level` and boxes below it (a few scalar operations; a table indexed by a run-time level would live in a kernel's
// scratch memory)
__host__ __device__ inline void tree_level(uint32_t leaves, int level, uint32_t& count, uint32_t& offset) {
    count = leaves;
    offset = 0;
    for (int l = 0; l < level; ++l) {
        offset += count;
        count = (count + kFan - 1) / kFan;
    }
}

__device__ __forceinline__ void wave_sync() {   // a wave's LDS operations run in program order: keep the compiler to it
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ float wave_min(float v) { return wave_fold(v, [](float a, float b) { return fminf(a, b); }); }
__device__ __forceinline__ float wave_max(float v) { return wave_fold(v, [](float a, float b) { return fmaxf(a, b); }); }
__device__ __forceinline__ float lane_value(float v, int lane) {   // lane: wave-uniform
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}

// The rounded operations of a squared distance (differences, squares summed left to right; the build has -ffp-contract=off) on the
// gap to a box: never above the computed distance of a member (see the walks).  An empty box gives +inf.
__device__ __forceinline__ float box_bound(const float4& lo, const float4& hi, float qx, float qy, float qz) {
    const float gx = fmaxf(fmaxf(lo.x - qx, qx - hi.x), 0.0f);
    const float gy = fmaxf(fmaxf(lo.y - qy, qy - hi.y), 0.0f);
    const float gz = fmaxf(fmaxf(lo.z - qz, qz - hi.z), 0.0f);
    return (gx * gx + gy * gy) + gz * gz;
}

__device__ __forceinline__ uint64_t spread21(uint32_t v) {   // bit k of v (k < 21) -> bit 3k
    uint64_t x = v & 0x1FFFFFu;
    x = (x | (x << 32)) & 0x001F00000000FFFFull;
    x = (x | (x << 16)) & 0x001F0000FF0000FFull;
    x = (x | (x << 8)) & 0x100F00F00F00F00Full;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}
__device__ __forceinline__ uint32_t grid_cell(float x, float lo, float hi) {
    const float extent = hi - lo;
    const float t = extent > 0.0f ? (x - lo) / extent * (float)kCellMax : 0.0f;
    return t >= 0.0f ? (uint32_t)fminf(t, (float)kCellMax) : 0u;   // (NaN -> 0: the code only steers the search, never its result)
}

// lo / hi of six floats reduced over the workgroup (256 lanes), result in every lane
__device__ inline void block_minmax(float lo[3], float hi[3], float* s_red /* 6 * 4 floats */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int a = 0; a < 3; ++a) { lo[a] = wave_min(lo[a]); hi[a] = wave_max(hi[a]); }
    if (lane == 0)
        for (int a = 0; a < 3; ++a) { s_red[a * 4 + wave] = lo[a]; s_red[(3 + a) * 4 + wave] = hi[a]; }
    __syncthreads();
    for (int a = 0; a < 3; ++a) {
        lo[a] = fminf(fminf(s_red[a * 4], s_red[a * 4 + 1]), fminf(s_red[a * 4 + 2], s_red[a * 4 + 3]));
        hi[a] = fmaxf(fmaxf(s_red[(3 + a) * 4], s_red[(3 + a) * 4 + 1]), fmaxf(s_red[(3 + a) * 4 + 2], s_red[(3 + a) * 4 + 3]));
    }
    __syncthreads();
}

}  // namespace gsr
