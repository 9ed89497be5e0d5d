// gsr_knn.hip -- the mean squared distance of every point to its three nearest neighbours (include/gsr.h: gsr_knn3_mean_dist), and
// the K nearest neighbours of every query with their indices (gsr_knn_points, further down: the same tree and walk, K slots).
//
// The drop-in for simple_knn's distCUDA2 (sugar/gaussian_splatting/submodules/simple-knn), which GaussianModel.create_from_pcd uses
// to give every Gaussian its initial scale.  The result is a pointwise function of the input ("Nearest neighbours"):
//   out[i] = fl(fl(fl(s0 + s1) + s2) / 3),  s0 <= s1 <= s2 the three smallest of { d(i, j) : j != i, d(i, j) < FLT_MAX }, missing = FLT_MAX,
//   d(i, j) = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)),  dx = fl(x_j - x_i), ...
// so any exact search gives the same bits.  This one, all stream-ordered, no host synchronisation:
//
//   bounds  : min / max over the finite points, per-workgroup partials (kBoundsBlocks of them, no atomics, nothing to clear);
//   codes   : 63-bit Morton codes on a (2^21)^3 grid of those bounds; a point with a non-finite coordinate gets 2^63 (sorts last).
//             Far outliers stretch the bounds of a COLMAP cloud: with 10 bits per axis its dense part would share a handful of
//             cells, the leaves would be random samples of it and the search quadratic;
//   sort    : (code, index) by the library's radix sort, low word first (iota payload), then the high word (stable): morton_sort;
//   pack    : the points gathered once in sorted order into float4 (x, y, z, index bits); one wave per leaf of 64 points reduces
//             the leaf's box (finite members only: a leaf of non-finite points has an empty box, lo = +inf, hi = -inf);
//   levels  : boxes of 16 children each, level over level, until at most 16 boxes are left (six levels below 2^30 points):
//             tree_levels, like morton_sort in gsr_tree.hip, where gsr_meshquery.hip finds them too (the tree's shape: gsr_tree.h);
//   search  : one wave per leaf, one lane per query: the slots are seeded with the wave's own leaf, then a depth-first walk over the
//             tree from the top prunes by box bounds (walk_tree, further down: the walk, its prune rule and why it is exact).
// Defines the entry points gsr_knn3_scratch_bytes, gsr_knn3_mean_dist, gsr_knn_points_scratch_bytes and gsr_knn_points.
#include "gsr_tree.h"

#include <cfloat>

namespace gsr {
namespace {

// The tree of gsr_tree.h over points, as the by-value table the search kernels receive.
struct KnnTree {
    const float4* boxes;
    uint32_t count[kTreeMaxLevels];
    uint32_t offset[kTreeMaxLevels];
    int top;
};
// Byte offsets of the regions of the caller's scratch (each 256-byte aligned); bytes = the whole.
struct KnnLayout {
    size_t keys, keys_alt, vals, vals_alt, key_hi, radix, packed, boxes, partials, bytes;
    KnnTree tree;
};
constexpr int kKnnPointsMaxK = 16;   // slots per query of gsr_knn_points
constexpr uint32_t kNonFiniteKey = 1u << 31;     // (the high word of a point with a non-finite coordinate)

// d(i, j) of the contract: candidate minus query, squares summed left to right (the build has -ffp-contract=off)
__device__ __forceinline__ float sq_dist(const float4& c, float qx, float qy, float qz) {
    const float dx = c.x - qx, dy = c.y - qy, dz = c.z - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// s0 <= s1 <= s2 stay sorted; NaN / inf / FLT_MAX change nothing (as the reference's strict `knn[j] > dist`)
__device__ __forceinline__ void insert3(float d, float& s0, float& s1, float& s2) {
    d = d < FLT_MAX ? d : FLT_MAX;
    s2 = fminf(s2, fmaxf(s1, d));
    s1 = fminf(s1, fmaxf(s0, d));
    s0 = fminf(s0, d);
}

__global__ __launch_bounds__(256) void knn_bounds_kernel(uint32_t n, const float* __restrict__ points, float4* __restrict__ partials) {
    __shared__ float s_red[24];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += kBoundsBlocks * 256u) {
        const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
        if (finite3(x, y, z)) {
            lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
            hi[0] = fmaxf(hi[0], x); hi[1] = fmaxf(hi[1], y); hi[2] = fmaxf(hi[2], z);
        }
    }
    block_minmax(lo, hi, s_red);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        partials[2 * blockIdx.x + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

__global__ __launch_bounds__(256) void knn_codes_kernel(uint32_t n, const float* __restrict__ points, const float4* __restrict__ partials,
                                                        uint32_t* __restrict__ key_lo, uint32_t* __restrict__ key_hi) {
    __shared__ float s_red[24];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (threadIdx.x < kBoundsBlocks) {
        const float4 a = partials[2 * threadIdx.x], b = partials[2 * threadIdx.x + 1];
        lo[0] = a.x; lo[1] = a.y; lo[2] = a.z; hi[0] = b.x; hi[1] = b.y; hi[2] = b.z;
    }
    block_minmax(lo, hi, s_red);
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
        uint64_t code = (uint64_t)kNonFiniteKey << 32;
        if (finite3(x, y, z))
            code = spread21(grid_cell(x, lo[0], hi[0])) | (spread21(grid_cell(y, lo[1], hi[1])) << 1) |
                   (spread21(grid_cell(z, lo[2], hi[2])) << 2);
        key_lo[i] = (uint32_t)code;
        key_hi[i] = (uint32_t)(code >> 32);
    }
}

// one wave per leaf: the sorted points packed, the leaf's box (finite members)
__global__ __launch_bounds__(256) void knn_pack_kernel(uint32_t n, const float* __restrict__ points, const uint32_t* __restrict__ order,
                                                       float4* __restrict__ packed, float4* __restrict__ leaf_boxes) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (s < n) {
        const uint32_t idx = order[s];
        const float x = points[3 * (size_t)idx], y = points[3 * (size_t)idx + 1], z = points[3 * (size_t)idx + 2];
        packed[s] = make_float4(x, y, z, __uint_as_float(idx));
        if (finite3(x, y, z)) { lo[0] = hi[0] = x; lo[1] = hi[1] = y; lo[2] = hi[2] = z; }
    }
    for (int a = 0; a < 3; ++a) { lo[a] = wave_min(lo[a]); hi[a] = wave_max(hi[a]); }
    const uint32_t leaf = s / kLeaf;
    if ((threadIdx.x & 63) == 0 && leaf * kLeaf < n) {
        leaf_boxes[2 * leaf] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        leaf_boxes[2 * leaf + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

struct Query {
    float x, y, z;
    bool active;   // in range and finite: the others answer (3 FLT_MAX) / 3 = +inf
};

// Children [first, first + cnt) of `level` kept by some lane, pushed farthest first so the nearest is popped next.
__device__ __forceinline__ void push_children(const KnnTree& tree, int level, uint32_t first, int cnt, uint32_t own_leaf, const Query& q,
                                              float s2, const float4& wlo, const float4& whi, uint32_t* stack, int& top, int lane) {
    const float4* boxes = tree.boxes + 2 * (size_t)tree.offset[level];
    float4 clo = make_float4(INFINITY, INFINITY, INFINITY, 0.0f), chi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
    if (lane < cnt) { clo = boxes[2 * (first + lane)]; chi = boxes[2 * (first + lane) + 1]; }
    uint32_t keep = 0u;
    for (int j = 0; j < cnt; ++j) {
        const float4 lo = make_float4(lane_value(clo.x, j), lane_value(clo.y, j), lane_value(clo.z, j), 0.0f);
        const float4 hi = make_float4(lane_value(chi.x, j), lane_value(chi.y, j), lane_value(chi.z, j), 0.0f);
        const float lb = box_bound(lo, hi, q.x, q.y, q.z);
        if (__ballot(q.active && !(lb > s2)) != 0ull) keep |= 1u << j;
    }
    if (level == 0 && own_leaf - first < (uint32_t)cnt) keep &= ~(1u << (own_leaf - first));   // seeded already
    if (keep == 0u) return;
    // order key: the gap between the child's box and the wave's queries' box
    const float gx = fmaxf(fmaxf(clo.x - whi.x, wlo.x - chi.x), 0.0f);
    const float gy = fmaxf(fmaxf(clo.y - whi.y, wlo.y - chi.y), 0.0f);
    const float gz = fmaxf(fmaxf(clo.z - whi.z, wlo.z - chi.z), 0.0f);
    const float key = (gx * gx + gy * gy) + gz * gz;
    int rank = 0;   // kept children farther than this one (ties: the higher index counts as farther)
    for (int j = 0; j < cnt; ++j) {
        const float kj = lane_value(key, j);
        rank += ((keep >> j) & 1u) && (kj > key || (kj == key && j > lane)) ? 1 : 0;
    }
    if (lane < cnt && ((keep >> lane) & 1u)) (stack + top)[rank] = ((uint32_t)level << 29) | (first + lane);   // (stack + top: where the pop read)
    top += __popc(keep);
    wave_sync();
}

// ---- a lane's slots: kernel locals in registers (slot numbers are compile-time constants, after unrolling for the K slots), handed
// to the walk as a pack of references.  The walk asks two overloads about them: slots_kth(slots...), the lane's pruning threshold
// (its last slot's distance), and slots_scan(leaf, cnt, q, skip, slots...): `cnt` candidates of a leaf in LDS against the slots, the
// one at position `skip` left out (-1: none).  Not a struct that owns them: the compiler then keeps sd[S], sj[S] as 2 S scalars, not
// as the two vector register groups it forms from kernel-local arrays, and the K = 16 search ran 2 - 6 % slower.

// gsr_knn3_mean_dist: three distances, s0 <= s1 <= s2, FLT_MAX while empty.
__device__ __forceinline__ float slots_kth(const float&, const float&, const float& s2) { return s2; }
__device__ __forceinline__ void slots_scan(const float4* leaf, int cnt, const Query& q, int skip, float& s0, float& s1, float& s2) {
    for (int c = 0; c < cnt; ++c) {
        const float d = sq_dist(leaf[c], q.x, q.y, q.z);
        insert3(c != skip ? d : FLT_MAX, s0, s1, s2);
    }
}

// gsr_knn_points: S = 4, 8 or 16 (distance, index in p2) pairs sd[k], sj[k] in ascending (d, j) order for K <= S
// neighbours.  Equal distances go by the lower index, so a row is a pointwise function of the input for duplicates and lattices as
// well.  The first S - K slots hold (-inf, 0), below every candidate and never displaced, so the K-th best is always slot S - 1:
// neither the threshold nor the early-out needs a run-time slot number.  An empty slot is (FLT_MAX, ~0).

// (d, j) < (sd, sj), lexicographic
__device__ __forceinline__ bool slot_less(float d, uint32_t j, float sd, uint32_t sj) { return d < sd || (d == sd && j < sj); }

// The slots stay sorted ascending; a candidate that is not below the last slot changes nothing.
template <int S>
__device__ __forceinline__ void insert_slots(float d, uint32_t j, float (&sd)[S], uint32_t (&sj)[S]) {
    bool below = slot_less(d, j, sd[S - 1], sj[S - 1]);   // below slot k
#pragma unroll
    for (int k = S - 1; k >= 1; --k) {
        const bool below_prev = slot_less(d, j, sd[k - 1], sj[k - 1]);
        sd[k] = below_prev ? sd[k - 1] : (below ? d : sd[k]);
        sj[k] = below_prev ? sj[k - 1] : (below ? j : sj[k]);
        below = below_prev;
    }
    sd[0] = below ? d : sd[0];
    sj[0] = below ? j : sj[0];
}

template <int S>
__device__ __forceinline__ float slots_kth(const float (&sd)[S], const uint32_t (&)[S]) { return sd[S - 1]; }
// A distance that is not below FLT_MAX (NaN, inf) becomes the empty slot's own pair, which is below no slot.  Most candidates enter
// nobody's row: one ballot skips their insertion.
template <int S>
__device__ __forceinline__ void slots_scan(const float4* leaf, int cnt, const Query& q, int skip, float (&sd)[S], uint32_t (&sj)[S]) {
    for (int c = 0; c < cnt; ++c) {
        const float4 cand = leaf[c];
        float d = sq_dist(cand, q.x, q.y, q.z);
        const bool ok = d < FLT_MAX && c != skip;
        d = ok ? d : FLT_MAX;
        const uint32_t j = ok ? __float_as_uint(cand.w) : ~0u;
        if (__ballot(q.active && slot_less(d, j, sd[S - 1], sj[S - 1])) == 0ull) continue;
        insert_slots<S>(d, j, sd, sj);
    }
}

// ---- the search: one wave per 64 queries, one lane per query.  Query `s` of `n`: `p` as stored (x, y, z, original index bits)
__device__ __forceinline__ Query load_query(uint32_t n, const float4* queries, uint32_t s, float4& p) {
    p = s < n ? queries[s] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    Query q;
    q.active = s < n && finite3(p.x, p.y, p.z);
    q.x = q.active ? p.x : 0.0f; q.y = q.active ? p.y : 0.0f; q.z = q.active ? p.z : 0.0f;
    return q;
}

// the box of the wave's active queries: it orders the walk
__device__ __forceinline__ void wave_box(const Query& q, float4& wlo, float4& whi) {
    wlo = make_float4(wave_min(q.active ? q.x : INFINITY), wave_min(q.active ? q.y : INFINITY), wave_min(q.active ? q.z : INFINITY), 0.0f);
    whi = make_float4(wave_max(q.active ? q.x : -INFINITY), wave_max(q.active ? q.y : -INFINITY), wave_max(q.active ? q.z : -INFINITY), 0.0f);
}

// A self query's wave holds the `cnt` points of its own leaf, `p` in lane order: they seed the slots, and the walk leaves that leaf
// out.  `skip`: the lane itself where the own point is no candidate (by position, so a duplicate stays one), -1 where it is.
template <class... Slots>
__device__ __forceinline__ void seed_own_leaf(float4* leaf, const float4& p, int cnt, const Query& q, int lane, int skip, Slots&... slots) {
    leaf[lane] = p;
    wave_sync();
    slots_scan(leaf, cnt, q, skip, slots...);
}

// The walk of both searches: depth first over the tree of `n` packed points from the top, on the wave-uniform `stack` in LDS;
// `own_leaf` is left out (seeded already; ~0: none).  A node's children are kept if some lane's lower bound is not above that lane's
// kth() (a ballot per child) and pushed nearest-first by their distance to the wave's box (push_children).  A popped leaf is tested
// again, the slots having tightened since the push, then staged into `leaf` with one coalesced 1 KiB load and scanned by all lanes
// at once.  The stage sits between two wave_sync(): its stores stay behind the previous scan's reads and ahead of the next one's.
// Exactness.  A box's lower bound is formed with the rounded operations of d(i, j) (per axis the gap lo - q or q - hi, squared,
// summed in the same order).  Rounding to nearest is monotone, so the bound never exceeds the computed distance of a member.  The
// prune rule, here and in push_children, is !(lb > kth): a box is skipped only when its bound is strictly above kth() for every
// lane, so that no member could enter a slot.  At equality a member of the K-slot search with a lower index still could: pruning
// on >= would return the right distances and, on a lattice, the wrong indices.  A distance enters a slot only when it is below
// FLT_MAX (NaN and inf map to the empty slot's value before the insertion).
template <class... Slots>
__device__ __forceinline__ void walk_tree(const KnnTree& tree, uint32_t n, const float4* packed, uint32_t own_leaf, const Query& q,
                                          float4* leaf, uint32_t* stack, int lane, Slots&... slots) {
    if (__ballot(q.active) == 0ull) return;
    float4 wlo, whi;
    wave_box(q, wlo, whi);
    int top = 0;
    push_children(tree, tree.top, 0u, (int)tree.count[tree.top], own_leaf, q, slots_kth(slots...), wlo, whi, stack, top, lane);
    while (top > 0) {
        const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)stack[--top]);
        const int level = (int)(e >> 29);
        const uint32_t node = e & ((1u << 29) - 1u);
        if (level > 0) {
            const uint32_t first = node * kFan;
            push_children(tree, level - 1, first, (int)min((uint32_t)kFan, tree.count[level - 1] - first), own_leaf, q,
                          slots_kth(slots...), wlo, whi, stack, top, lane);
            continue;
        }
        const float4 lo = tree.boxes[2 * (size_t)node], hi = tree.boxes[2 * (size_t)node + 1];   // (leaves: level offset 0)
        const float lb = box_bound(lo, hi, q.x, q.y, q.z);
        if (__ballot(q.active && !(lb > slots_kth(slots...))) == 0ull) continue;
        const uint32_t base = node * kLeaf;
        const int cnt = (int)min((uint32_t)kLeaf, n - base);
        wave_sync();
        leaf[lane] = lane < cnt ? packed[base + lane] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        wave_sync();
        slots_scan(leaf, cnt, q, -1, slots...);
    }
}

// gsr_knn3_mean_dist: one wave per leaf, whose points are its queries; the own point is no candidate.
__global__ __launch_bounds__(256) void knn_search_kernel(uint32_t n, const float4* __restrict__ packed, KnnTree tree, float* __restrict__ out) {
    __shared__ float4 s_leaf[4][kLeaf];
    __shared__ uint32_t s_stack[4][kStackDepth];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t own = blockIdx.x * 4u + (uint32_t)wave;    // this wave's leaf
    if (own * kLeaf >= n) return;
    const uint32_t s = own * kLeaf + lane;
    float4 p;
    const Query q = load_query(n, packed, s, p);
    float s0 = FLT_MAX, s1 = FLT_MAX, s2 = FLT_MAX;
    seed_own_leaf(s_leaf[wave], p, (int)min((uint32_t)kLeaf, n - own * kLeaf), q, lane, lane, s0, s1, s2);
    walk_tree(tree, n, packed, own, q, s_leaf[wave], s_stack[wave], lane, s0, s1, s2);
    if (s < n) {
        if (!q.active) s0 = s1 = s2 = FLT_MAX;
        out[__float_as_uint(p.w)] = ((s0 + s1) + s2) / 3.0f;
    }
}

// gsr_knn_points: S slots for K <= S neighbours.  kSelf: the queries are the tree's own points (queries == packed, n1 == n2); a wave
// takes the points of its leaf and seeds its slots from that leaf, the own point included (the self is a candidate like any other).
// Otherwise `queries` is p1 in the order of its Morton codes on p2's grid, and nothing is seeded.
template <int S, bool kSelf>
__global__ __launch_bounds__(256) void knn_points_search_kernel(uint32_t n1, const float4* __restrict__ queries, uint32_t n2,
                                                                const float4* __restrict__ packed, KnnTree tree, int K,
                                                                float* __restrict__ dists, long long* __restrict__ idx) {
    __shared__ float4 s_leaf[4][kLeaf];
    __shared__ uint32_t s_stack[4][kStackDepth];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t group = blockIdx.x * 4u + (uint32_t)wave;    // this wave's 64 queries; kSelf: its leaf
    if (group * kLeaf >= n1) return;
    const uint32_t s = group * kLeaf + lane;
    float4 p;
    const Query q = load_query(n1, queries, s, p);
    float sd[S];
    uint32_t sj[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
        const bool spare = k < S - K;
        sd[k] = spare ? -INFINITY : FLT_MAX;
        sj[k] = spare ? 0u : ~0u;
    }
    if (kSelf) seed_own_leaf(s_leaf[wave], p, (int)min((uint32_t)kLeaf, n2 - group * kLeaf), q, lane, -1, sd, sj);
    walk_tree(tree, n2, packed, kSelf ? group : ~0u, q, s_leaf[wave], s_stack[wave], lane, sd, sj);
    if (s >= n1) return;
    // the row of the query's original index: empty slots (all of them for a non-finite query) are (+inf, -1)
    float od[S];
    long long oj[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
        const bool filled = q.active && sd[k] < FLT_MAX;
        od[k] = filled ? sd[k] : INFINITY;
        oj[k] = filled ? (long long)sj[k] : -1ll;
    }
    const size_t row = (size_t)__float_as_uint(p.w) * (size_t)K;
    if (K == S) {   // whole rows of 4 S and 8 S bytes, 16-byte aligned: 16-byte stores
        float4* drow = reinterpret_cast<float4*>(dists + row);
        longlong2* irow = reinterpret_cast<longlong2*>(idx + row);
#pragma unroll
        for (int k = 0; k < S; k += 4) drow[k / 4] = make_float4(od[k], od[k + 1], od[k + 2], od[k + 3]);
#pragma unroll
        for (int k = 0; k < S; k += 2) irow[k / 2] = make_longlong2(oj[k], oj[k + 1]);
    } else {
#pragma unroll
        for (int k = 0; k < S; ++k)
            if (k >= S - K) { dists[row + (size_t)(k - (S - K))] = od[k]; idx[row + (size_t)(k - (S - K))] = oj[k]; }
    }
}

KnnLayout knn3_layout(uint32_t n) {
    KnnLayout L = {};
    if (n == 0) return L;
    const TreeShape shape = tree_shape(n);
    L.tree.top = shape.top;
    for (int level = 0; level <= shape.top; ++level) tree_level(shape.leaves, level, L.tree.count[level], L.tree.offset[level]);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t here = at; at = align_up(at + bytes); return here; };
    L.keys = take(4 * (size_t)n);
    L.keys_alt = take(4 * (size_t)n);
    L.vals = take(4 * (size_t)n);
    L.vals_alt = take(4 * (size_t)n);
    L.key_hi = take(4 * (size_t)n);
    L.radix = take(radix_scratch_words(n) * sizeof(uint32_t));
    L.packed = take(16 * (size_t)n);
    L.boxes = take(32 * (size_t)shape.boxes);
    L.partials = take(32 * (size_t)kBoundsBlocks);
    L.bytes = at;
    return L;
}

struct KnnRegions {
    uint32_t *keys, *keys_alt, *vals, *vals_alt, *key_hi, *radix;
    float4 *packed, *boxes, *partials;
};
KnnRegions knn_regions(const KnnLayout& L, void* scratch) {
    char* base = static_cast<char*>(scratch);
    auto u32 = [&](size_t at) { return reinterpret_cast<uint32_t*>(base + at); };
    auto f4 = [&](size_t at) { return reinterpret_cast<float4*>(base + at); };
    return {u32(L.keys), u32(L.keys_alt), u32(L.vals), u32(L.vals_alt), u32(L.key_hi), u32(L.radix), f4(L.packed), f4(L.boxes), f4(L.partials)};
}

// `points` in the order of their Morton codes on the grid of `partials`, packed into r.packed with the boxes of every 64 in r.boxes
hipError_t knn_sort_and_pack(uint32_t n, const float* points, const float4* partials, const KnnRegions& r, hipStream_t stream) {
    const uint32_t blocks = (n + 255u) / 256u;
    hipLaunchKernelGGL(knn_codes_kernel, dim3(min(blocks, 2048u)), dim3(256), 0, stream, n, points, partials, r.keys, r.key_hi);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    uint32_t* order = nullptr;
    e = morton_sort(r.radix, n, r.keys, r.keys_alt, r.vals, r.vals_alt, r.key_hi, &order, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(knn_pack_kernel, dim3(blocks), dim3(256), 0, stream, n, points, (const uint32_t*)order, r.packed, r.boxes);
    return hipGetLastError();
}

// bounds -> codes -> sort -> pack -> levels: the tree over `points` in the regions of L
hipError_t knn_build_tree(uint32_t n, const float* points, const KnnLayout& L, const KnnRegions& r, hipStream_t stream) {
    if (L.tree.count[L.tree.top] > (uint32_t)kFan) return hipErrorInvalidValue;   // (n < 2^30 never gets here)
    hipLaunchKernelGGL(knn_bounds_kernel, dim3(kBoundsBlocks), dim3(256), 0, stream, n, points, r.partials);
    hipError_t e = knn_sort_and_pack(n, points, r.partials, r, stream);
    if (e != hipSuccess) return e;
    return tree_levels(r.boxes, L.tree.count[0], L.tree.top, stream);
}

template <int S>
void launch_points_search(bool same, uint32_t n1, const float4* queries, uint32_t n2, const float4* packed, const KnnTree& tree, int K,
                          float* dists, long long* idx, hipStream_t stream) {
    const dim3 grid(((n1 + kLeaf - 1) / kLeaf + 3u) / 4u);
    if (same)
        hipLaunchKernelGGL((knn_points_search_kernel<S, true>), grid, dim3(256), 0, stream, n1, queries, n2, packed, tree, K, dists, idx);
    else
        hipLaunchKernelGGL((knn_points_search_kernel<S, false>), grid, dim3(256), 0, stream, n1, queries, n2, packed, tree, K, dists, idx);
}

// scratch: knn3_layout(n).bytes bytes, 256-byte aligned, any content; 0 < n < 2^30
hipError_t launch_knn3_mean_dist(uint32_t n, const float* points, float* out, void* scratch, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const KnnLayout L = knn3_layout(n);
    const KnnRegions r = knn_regions(L, scratch);
    hipError_t e = knn_build_tree(n, points, L, r, stream);
    if (e != hipSuccess) return e;
    KnnTree tree = L.tree;
    tree.boxes = r.boxes;
    hipLaunchKernelGGL(knn_search_kernel, dim3((L.tree.count[0] + 3u) / 4u), dim3(256), 0, stream, n, (const float4*)r.packed, tree, out);
    return hipGetLastError();
}

// The tree's regions, then (a separate query set) the same regions again for p1: its codes, their sort, the packed queries.
size_t knn_points_scratch_bytes(uint32_t n1, uint32_t n2, bool same) {
    return knn3_layout(n2).bytes + (same ? 0 : knn3_layout(n1).bytes);
}

// The same tree over p2, K <= kKnnPointsMaxK slots per query.  same = (p1 == p2 && n1 == n2): the tree's own leaves are the queries.
// scratch: knn_points_scratch_bytes(n1, n2, same) bytes, 256-byte aligned; dists / idx 16-byte aligned for K = 4, 8, 16 (4 / 8 bytes
// otherwise); 0 < K <= n2 < 2^30, n1 < 2^30
hipError_t launch_knn_points(uint32_t n1, const float* p1, uint32_t n2, const float* p2, int K, float* dists, long long* idx, void* scratch,
                             hipStream_t stream) {
    if (n1 == 0) return hipSuccess;
    if (n2 == 0 || K < 1 || K > kKnnPointsMaxK) return hipErrorInvalidValue;
    const bool same = p1 == p2 && n1 == n2;
    const KnnLayout L = knn3_layout(n2);
    const KnnRegions r = knn_regions(L, scratch);
    hipError_t e = knn_build_tree(n2, p2, L, r, stream);
    if (e != hipSuccess) return e;
    const float4* queries = r.packed;
    if (!same) {   // p1 on p2's grid (cells clamped: a query may lie outside the bounds), so that a wave's queries are neighbours
        // (the regions of a tree over n1 points, for the sorts and the packed queries; the pack kernel also leaves the boxes of every
        // 64 queries there, a by-product nobody reads -- the search forms its wave's box itself -- and `partials` stays unused)
        const KnnRegions rq = knn_regions(knn3_layout(n1), static_cast<char*>(scratch) + L.bytes);
        e = knn_sort_and_pack(n1, p1, r.partials, rq, stream);
        if (e != hipSuccess) return e;
        queries = rq.packed;
    }
    KnnTree tree = L.tree;
    tree.boxes = r.boxes;
    if (K <= 4) launch_points_search<4>(same, n1, queries, n2, r.packed, tree, K, dists, idx, stream);
    else if (K <= 8) launch_points_search<8>(same, n1, queries, n2, r.packed, tree, K, dists, idx, stream);
    else launch_points_search<16>(same, n1, queries, n2, r.packed, tree, K, dists, idx, stream);
    return hipGetLastError();
}

}  // namespace
}  // namespace gsr

using gsr::fail;

extern "C" {

size_t gsr_knn3_scratch_bytes(uint32_t n) {
    return n >= gsr::kKnn3MaxPoints ? 0 : gsr::knn3_layout(n).bytes;
}

int gsr_knn3_mean_dist(uint32_t n, const float* points, float* out, void* scratch, size_t scratch_bytes, void* stream_) {
    if (n == 0) return GSR_OK;
    if (n >= gsr::kKnn3MaxPoints) return fail(GSR_ERR_INVALID_ARG, "gsr_knn3_mean_dist: %u points (at most 2^30 - 1)", n);
    if (!points || !out || !scratch) return fail(GSR_ERR_INVALID_ARG, "null pointer");
    if (((uintptr_t)points & 3u) != 0u || ((uintptr_t)out & 3u) != 0u || !gsr::aligned256(scratch))
        return fail(GSR_ERR_INVALID_ARG, "gsr_knn3_mean_dist: misaligned pointer (points / out: 4 bytes, scratch: 256 bytes)");
    if (scratch_bytes < gsr_knn3_scratch_bytes(n))
        return fail(GSR_ERR_INVALID_ARG, "gsr_knn3_mean_dist: scratch too small (%zu of %zu bytes)", scratch_bytes, gsr_knn3_scratch_bytes(n));
    GSR_HIP(gsr::launch_knn3_mean_dist(n, points, out, scratch, (hipStream_t)stream_));
    return GSR_OK;
}

size_t gsr_knn_points_scratch_bytes(int64_t n1, int64_t n2, int same) {
    if (n1 < 0 || n2 < 0 || n1 >= (int64_t)gsr::kKnn3MaxPoints || n2 >= (int64_t)gsr::kKnn3MaxPoints) return 0;
    return gsr::knn_points_scratch_bytes((uint32_t)n1, (uint32_t)n2, same != 0);
}

int gsr_knn_points(int64_t n1, const float* p1, int64_t n2, const float* p2, int K, float* dists, int64_t* idx, void* scratch,
                   size_t scratch_bytes, void* stream_) {
    if (n1 < 0 || n2 < 0) return fail(GSR_ERR_INVALID_ARG, "gsr_knn_points: negative count (n1 %lld, n2 %lld)", (long long)n1, (long long)n2);
    if (n1 >= (int64_t)gsr::kKnn3MaxPoints || n2 >= (int64_t)gsr::kKnn3MaxPoints)
        return fail(GSR_ERR_INVALID_ARG, "gsr_knn_points: %lld and %lld points (at most 2^30 - 1 each)", (long long)n1, (long long)n2);
    if (K < 1 || K > gsr::kKnnPointsMaxK) return fail(GSR_ERR_INVALID_ARG, "gsr_knn_points: K = %d (1 to %d)", K, gsr::kKnnPointsMaxK);
    if (n1 == 0) return GSR_OK;
    if (n2 < K) return fail(GSR_ERR_INVALID_ARG, "gsr_knn_points: n2 = %lld is less than K = %d", (long long)n2, K);
    if (!p1 || !p2 || !dists || !idx || !scratch) return fail(GSR_ERR_INVALID_ARG, "gsr_knn_points: null pointer");
    // K = 4, 8, 16 rows are written with 16-byte stores; every other K element by element
    const bool wide = K == 4 || K == 8 || K == 16;
    if (((uintptr_t)p1 & 3u) != 0u || ((uintptr_t)p2 & 3u) != 0u || ((uintptr_t)dists & (wide ? 15u : 3u)) != 0u ||
        ((uintptr_t)idx & (wide ? 15u : 7u)) != 0u || !gsr::aligned256(scratch))
        return fail(GSR_ERR_INVALID_ARG, "gsr_knn_points: misaligned pointer (p1 / p2: 4 bytes; dists / idx: 16 bytes for K = 4, 8, 16, "
                                         "else 4 / 8 bytes; scratch: 256 bytes)");
    const size_t need = gsr_knn_points_scratch_bytes(n1, n2, p1 == p2 && n1 == n2);
    if (scratch_bytes < need) return fail(GSR_ERR_INVALID_ARG, "gsr_knn_points: scratch too small (%zu of %zu bytes)", scratch_bytes, need);
    GSR_HIP(gsr::launch_knn_points((uint32_t)n1, p1, (uint32_t)n2, p2, K, dists, reinterpret_cast<long long*>(idx), scratch,
                                   (hipStream_t)stream_));
    return GSR_OK;
}


}  // extern "C"
