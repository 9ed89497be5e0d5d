// gsr_meshloss.hip -- pytorch3d.loss.mesh_normal_consistency of one mesh in fused passes (include/gsr.h: gsr_normal_consistency_plan,
// gsr_normal_consistency_forward, gsr_normal_consistency_backward; the contract is the module docstring of autovfx_amd/meshloss.py and
// DESIGN.md 7k).  An incidence is a (face f, slot k) with id 3 f + k: its edge is (faces[f][(k+1)%3], faces[f][(k+2)%3]) ordered
// lo <= hi, its opposite vertex faces[f][k].
//   plan       topology only.  keys (hi and lo of every incidence; V for the incidences of a face with an index outside [0, V)), two
//              stable radix sorts over an iota payload (by hi, then by the gathered lo), the edge of every sorted position, and one
//              pass in which every position counts the later positions on its edge; their sum goes to `pairs` with one 64-bit
//              integer atomic per workgroup.  No host read.
//   forward    one lane per sorted position: nothing read beyond two words when it has no partner (half the lanes of a closed
//              manifold mesh); else its own normal, then its later partners in ascending order, their terms added serially into
//              T_s; a 256-leaf tree in LDS per workgroup, then one workgroup of 1024 lanes over the partials (chunks of 64, then the
//              chunk sums, then a 1024-leaf tree): at most 8 + 64 + 64 + 10 additions on the path of any T_s, a fixed shape, no float
//              atomics.
//   backward   the same walk; every pair adds twelve fp32 terms to grad_verts (zeroed on the stream first) with float atomics.
// The kernels trust nothing in a plan: an id outside [0, 3F), a partner count past the end and a face with a bad index are skipped.
// fp32 throughout, -ffp-contract=off, IEEE division and sqrt: the numpy restatements compute the same bits.
#include "gsr_internal.h"
#include "gsr_vec3.h"

#include <math.h>

namespace gsr {
namespace {

constexpr int kLossThreads = 256;
constexpr int kSumThreads = 1024;              // the second stage: one workgroup
constexpr int kSumChunk = 64;                  // partials a lane adds serially before the chunk sums are added
constexpr int64_t kMaxIncidences = (int64_t)1 << 30;   // 3 F from here on is refused (the radix sort's limit)
constexpr int64_t kMaxFaces = (kMaxIncidences - 1) / 3;
constexpr float kCosEps = 1e-8f;

struct Incidence {
    uint32_t lo, hi, opp;
};

// false: id outside [0, n) or a face with an index outside [0, V); nothing is read from verts by the caller then
__device__ inline bool load_incidence(const long long* __restrict__ faces, long long V, uint32_t n, uint32_t id, Incidence& inc) {
    if (id >= n) return false;
    const uint32_t f = id / 3u, k = id - 3u * f;
    const long long* row = faces + 3 * (size_t)f;
    const long long i0 = row[0], i1 = row[1], i2 = row[2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return false;
    const long long o = k == 0u ? i0 : k == 1u ? i1 : i2;
    const long long a = k == 0u ? i1 : k == 1u ? i2 : i0;
    const long long b = k == 0u ? i2 : k == 1u ? i0 : i1;
    inc.lo = (uint32_t)(a < b ? a : b), inc.hi = (uint32_t)(a < b ? b : a), inc.opp = (uint32_t)o;   // (V < 2^31)
    return true;
}

__device__ inline bool repeats_an_index(const Incidence& i) { return i.lo == i.hi || i.opp == i.lo || i.opp == i.hi; }

// ---- the plan ----------------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kLossThreads) nc_keys_kernel(uint32_t n, long long V, const long long* __restrict__ faces,
                                                               uint32_t* __restrict__ key_hi, uint32_t* __restrict__ key_lo) {
    const uint32_t id = blockIdx.x * (uint32_t)kLossThreads + threadIdx.x;
    if (id >= n) return;
    Incidence inc;
    const bool ok = load_incidence(faces, V, n, id, inc);
    key_hi[id] = ok ? inc.hi : (uint32_t)V;
    key_lo[id] = ok ? inc.lo : (uint32_t)V;
}

__global__ void __launch_bounds__(kLossThreads) nc_gather_kernel(uint32_t n, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ key_lo,
                                                                 uint32_t* __restrict__ keys) {
    const uint32_t s = blockIdx.x * (uint32_t)kLossThreads + threadIdx.x;
    if (s < n) keys[s] = key_lo[ids[s]];
}

// order[s] and the edge of the sorted position s ((V, V): none)
__global__ void __launch_bounds__(kLossThreads) nc_edges_kernel(uint32_t n, long long V, const long long* __restrict__ faces,
                                                                const uint32_t* __restrict__ ids, int* __restrict__ order,
                                                                uint2* __restrict__ edges) {
    const uint32_t s = blockIdx.x * (uint32_t)kLossThreads + threadIdx.x;
    if (s >= n) return;
    const uint32_t id = ids[s];
    Incidence inc;
    const bool ok = load_incidence(faces, V, n, id, inc);
    order[s] = (int)id;
    edges[s] = ok ? make_uint2(inc.lo, inc.hi) : make_uint2((uint32_t)V, (uint32_t)V);
}

__global__ void __launch_bounds__(kLossThreads) nc_partners_kernel(uint32_t n, uint32_t none, const uint2* __restrict__ edges,
                                                                   int* __restrict__ partners, unsigned long long* __restrict__ pairs) {
    __shared__ unsigned long long s_count[kLossThreads];
    const uint32_t s = blockIdx.x * (uint32_t)kLossThreads + threadIdx.x;
    uint32_t count = 0u;
    if (s < n) {
        const uint2 e = edges[s];
        if (e.x != none)
            for (uint32_t t = s + 1u; t < n; ++t) {
                const uint2 o = edges[t];
                if (o.x != e.x || o.y != e.y) break;
                ++count;
            }
        partners[s] = (int)count;
    }
    s_count[threadIdx.x] = count;
    __syncthreads();
    for (int half = kLossThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s_count[threadIdx.x] += s_count[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0 && s_count[0] != 0ull) atomicAdd(pairs, s_count[0]);
}

// ---- the contract's arithmetic: restated operation by operation in autovfx_amd/meshloss.py (the 3-vectors: gsr_vec3.h) -----------------

// The sum of a workgroup's N values (a power of two) by halving in LDS: leaf i + N/2 onto leaf i, then N/4, ...: log2 N additions on
// every path.  The result is valid in thread 0.
template <int N>
__device__ inline float tree_sum(float* s_leaf, float v) {
    s_leaf[threadIdx.x] = v;
    __syncthreads();
    for (int half = N / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s_leaf[threadIdx.x] = s_leaf[threadIdx.x] + s_leaf[threadIdx.x + half];
        __syncthreads();
    }
    return s_leaf[0];
}

// What a position that has partners needs of itself.
struct Walk {
    Incidence inc;
    Vec3 v_lo, e, w, n;
    uint32_t count;     // partners inside [0, n)
};

__device__ inline bool begin_walk(uint32_t n, long long V, const float* __restrict__ verts, const long long* __restrict__ faces,
                                  const int* __restrict__ order, const int* __restrict__ partners, uint32_t s, Walk& k) {
    const int claimed = partners[s];
    if (claimed <= 0) return false;
    const uint32_t room = n - 1u - s;
    k.count = (uint32_t)claimed < room ? (uint32_t)claimed : room;
    if (k.count == 0u || !load_incidence(faces, V, n, (uint32_t)order[s], k.inc)) return false;
    k.v_lo = load3(verts, k.inc.lo);
    k.e = sub(load3(verts, k.inc.hi), k.v_lo);
    k.w = sub(load3(verts, k.inc.opp), k.v_lo);
    k.n = cross(k.e, k.w);
    return true;
}

__global__ void __launch_bounds__(kLossThreads) nc_forward_kernel(uint32_t n, long long V, const float* __restrict__ verts,
                                                                  const long long* __restrict__ faces, const int* __restrict__ order,
                                                                  const int* __restrict__ partners, float* __restrict__ partials,
                                                                  float* __restrict__ terms) {
    __shared__ float s_leaf[kLossThreads];
    const uint32_t s = blockIdx.x * (uint32_t)kLossThreads + threadIdx.x;
    float T = 0.0f;
    Walk k;
    if (s < n && begin_walk(n, V, verts, faces, order, partners, s, k)) {
        const float a = fmaxf(norm(k.n), kCosEps);
        for (uint32_t j = 1u; j <= k.count; ++j) {
            Incidence other;
            if (!load_incidence(faces, V, n, (uint32_t)order[s + j], other)) continue;
            const Vec3 nt = cross(k.e, sub(load3(verts, other.opp), k.v_lo));
            const float b = fmaxf(norm(nt), kCosEps);
            T = T + (1.0f + dot(k.n, nt) / (a * b));
        }
    }
    if (s < n && terms != nullptr) terms[s] = T;
    const float sum = tree_sum<kLossThreads>(s_leaf, T);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

// One workgroup: lane j adds the partials j, j + 1024, ... in chunks of 64, then its chunk sums, then the 1024-leaf tree.
__global__ void __launch_bounds__(kSumThreads) nc_sum_kernel(uint32_t count, const float* __restrict__ partials,
                                                             const long long* __restrict__ pairs, float* __restrict__ loss) {
    __shared__ float s_leaf[kSumThreads];
    float acc = 0.0f;
    for (uint32_t first = threadIdx.x; first < count; first += (uint32_t)(kSumThreads * kSumChunk)) {
        float chunk = 0.0f;
        for (uint32_t r = 0; r < (uint32_t)kSumChunk; ++r) {
            const uint32_t i = first + r * (uint32_t)kSumThreads;
            if (i < count) chunk = chunk + partials[i];
        }
        acc = acc + chunk;
    }
    const float S = tree_sum<kSumThreads>(s_leaf, acc);
    if (threadIdx.x == 0) {
        const long long P = pairs[0];
        loss[0] = P > 0 ? S / (float)P : 0.0f;
    }
}

__global__ void __launch_bounds__(kLossThreads) nc_backward_kernel(uint32_t n, long long V, const float* __restrict__ verts,
                                                                   const long long* __restrict__ faces, const int* __restrict__ order,
                                                                   const int* __restrict__ partners, const long long* __restrict__ pairs,
                                                                   const float* __restrict__ grad_loss, float* __restrict__ grad_verts) {
    const uint32_t s = blockIdx.x * (uint32_t)kLossThreads + threadIdx.x;
    Walk k;
    if (s >= n || !begin_walk(n, V, verts, faces, order, partners, s, k)) return;
    const long long P = pairs[0];
    if (P <= 0 || repeats_an_index(k.inc)) return;
    const float c = grad_loss[0] / (float)P;
    const float ra = norm(k.n), a = fmaxf(ra, kCosEps);
    float* d_lo = grad_verts + 3 * (size_t)k.inc.lo;
    float* d_hi = grad_verts + 3 * (size_t)k.inc.hi;
    float* d_s = grad_verts + 3 * (size_t)k.inc.opp;
    for (uint32_t j = 1u; j <= k.count; ++j) {
        Incidence other;
        if (!load_incidence(faces, V, n, (uint32_t)order[s + j], other)) continue;
        other.lo = k.inc.lo, other.hi = k.inc.hi;       // (a plan's partners share the edge)
        if (repeats_an_index(other)) continue;
        const Vec3 wt = sub(load3(verts, other.opp), k.v_lo);
        const Vec3 nt = cross(k.e, wt);
        const float rb = norm(nt), b = fmaxf(rb, kCosEps);
        const float q = a * b;
        const float r = dot(k.n, nt) / q;
        // d term / d n_s = n_t / q - (r / a^2) n_s, the second part only above the clamp; likewise for n_t
        Vec3 us = over(nt, q);
        if (ra > kCosEps) us = sub(us, scale(r / (a * a), k.n));
        Vec3 ut = over(k.n, q);
        if (rb > kCosEps) ut = sub(ut, scale(r / (b * b), nt));
        const Vec3 gs = scale(c, us), gt = scale(c, ut);
        // n = e x w: d / de = w x g, d / dw = g x e
        const Vec3 ge = add(cross(k.w, gs), cross(wt, gt));
        const Vec3 ws = cross(gs, k.e), wtg = cross(gt, k.e);
        const Vec3 gw = add(ws, wtg);
        float* d_t = grad_verts + 3 * (size_t)other.opp;
        atomicAdd(d_hi + 0, ge.x), atomicAdd(d_hi + 1, ge.y), atomicAdd(d_hi + 2, ge.z);
        atomicAdd(d_lo + 0, -(ge.x + gw.x)), atomicAdd(d_lo + 1, -(ge.y + gw.y)), atomicAdd(d_lo + 2, -(ge.z + gw.z));
        atomicAdd(d_s + 0, ws.x), atomicAdd(d_s + 1, ws.y), atomicAdd(d_s + 2, ws.z);
        atomicAdd(d_t + 0, wtg.x), atomicAdd(d_t + 1, wtg.y), atomicAdd(d_t + 2, wtg.z);
    }
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------------

constexpr size_t kAlign = 256;
size_t align_up(size_t v) { return (v + kAlign - 1) & ~(kAlign - 1); }

// The plan's scratch: keys and keys_alt side by side (the sorted positions' edges, 8 bytes each, take their place after the sorts)
struct PlanLayout {
    size_t keys, vals, vals_alt, key_lo, radix, bytes;
};
PlanLayout plan_layout(uint32_t n) {
    PlanLayout L = {};
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t here = at; at = align_up(at + bytes); return here; };
    L.keys = take(8 * (size_t)n);
    L.vals = take(4 * (size_t)n);
    L.vals_alt = take(4 * (size_t)n);
    L.key_lo = take(4 * (size_t)n);
    L.radix = take(radix_scratch_words(n) * sizeof(uint32_t));
    L.bytes = at;
    return L;
}

int bit_length(uint64_t v) {
    int bits = 0;
    while (v != 0u) ++bits, v >>= 1;
    return bits;
}

hipError_t launch_plan(uint32_t n, int64_t V, const long long* faces, int* order, int* partners, unsigned long long* pairs, void* scratch,
                       hipStream_t stream) {
    const PlanLayout L = plan_layout(n);
    char* base = static_cast<char*>(scratch);
    auto u32 = [&](size_t at) { return reinterpret_cast<uint32_t*>(base + at); };
    uint32_t *keys = u32(L.keys), *keys_alt = keys + n, *vals = u32(L.vals), *vals_alt = u32(L.vals_alt), *key_lo = u32(L.key_lo);
    const dim3 grid(blocks_of(n, kLossThreads)), block(kLossThreads);
    hipLaunchKernelGGL(nc_keys_kernel, grid, block, 0, stream, n, (long long)V, faces, keys, key_lo);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // (lo, hi, id) ascending: by hi first, then by lo (both sorts are stable, the payload starts as the ids in order)
    const int bits = bit_length((uint64_t)V) > 0 ? bit_length((uint64_t)V) : 1;
    uint32_t *ks = nullptr, *vs = nullptr;
    e = radix_sort_pairs(u32(L.radix), n, bits, keys, keys_alt, vals, vals_alt, true, false, &ks, &vs, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(nc_gather_kernel, grid, block, 0, stream, n, (const uint32_t*)vs, (const uint32_t*)key_lo, keys);
    e = radix_sort_pairs(u32(L.radix), n, bits, keys, keys_alt, vs, vs == vals ? vals_alt : vals, false, false, &ks, &vs, stream);
    if (e != hipSuccess) return e;
    uint2* edges = reinterpret_cast<uint2*>(keys);
    hipLaunchKernelGGL(nc_edges_kernel, grid, block, 0, stream, n, (long long)V, faces, (const uint32_t*)vs, order, edges);
    hipLaunchKernelGGL(nc_partners_kernel, grid, block, 0, stream, n, (uint32_t)V, (const uint2*)edges, partners, pairs);
    return hipGetLastError();
}

// What the three launching entries refuse alike; null = nothing
const char* bad_mesh(int64_t V, int64_t F) {
    if (V < 0 || F < 0) return "negative count";
    if (F > kMaxFaces) return "3 F of 2^30 or more";
    if (V >= ((int64_t)1 << 31)) return "V of 2^31 or more";
    return nullptr;
}

}  // namespace
}  // namespace gsr

using gsr::fail;

extern "C" {

size_t gsr_normal_consistency_plan_scratch_bytes(int64_t F) {
    if (F < 0 || F > gsr::kMaxFaces) return 0;
    return gsr::plan_layout((uint32_t)(3 * F)).bytes;
}

int gsr_normal_consistency_plan(int64_t V, int64_t F, const int64_t* faces, int32_t* order, int32_t* partners, int64_t* pairs, void* scratch,
                                size_t scratch_bytes, void* stream_) {
    if (const char* why = gsr::bad_mesh(V, F)) return fail(GSR_ERR_INVALID_ARG, "gsr_normal_consistency_plan: %s", why);
    if (!pairs || (F > 0 && (!faces || !order || !partners || !scratch))) return fail(GSR_ERR_INVALID_ARG, "gsr_normal_consistency_plan: null pointer");
    if (!gsr::aligned8(faces) || !gsr::aligned4(order) || !gsr::aligned4(partners) || !gsr::aligned8(pairs) || !gsr::aligned256(scratch))
        return fail(GSR_ERR_INVALID_ARG, "gsr_normal_consistency_plan: misaligned pointer (order / partners: 4 bytes, faces / pairs: 8, scratch: 256)");
    const size_t need = gsr_normal_consistency_plan_scratch_bytes(F);
    if (F > 0 && scratch_bytes < need)
        return fail(GSR_ERR_INVALID_ARG, "gsr_normal_consistency_plan: scratch too small (%zu of %zu bytes)", scratch_bytes, need);
    hipStream_t stream = (hipStream_t)stream_;
    GSR_HIP(hipMemsetAsync(pairs, 0, sizeof(int64_t), stream));
    if (F == 0) return GSR_OK;
    GSR_HIP(gsr::launch_plan((uint32_t)(3 * F), V, reinterpret_cast<const long long*>(faces), order, partners,
                             reinterpret_cast<unsigned long long*>(pairs), scratch, stream));
    return GSR_OK;
}

size_t gsr_normal_consistency_scratch_bytes(int64_t F) {
    if (F < 0 || F > gsr::kMaxFaces) return 0;
    return sizeof(float) * (size_t)gsr::blocks_of(3 * F, gsr::kLossThreads);
}

int gsr_normal_consistency_forward(int64_t V, int64_t F, const float* verts, const int64_t* faces, const int32_t* order, const int32_t* partners,
                                   const int64_t* pairs, float* loss, float* terms_or_null, void* scratch, size_t scratch_bytes, void* stream_) {
    if (const char* why = gsr::bad_mesh(V, F)) return fail(GSR_ERR_INVALID_ARG, "gsr_normal_consistency_forward: %s", why);
    if (!loss || (V > 0 && !verts) || (F > 0 && (!faces || !order || !partners || !pairs || !scratch)))
        return fail(GSR_ERR_INVALID_ARG, "gsr_normal_consistency_forward: null pointer");
    if (!gsr::aligned4(verts) || !gsr::aligned8(faces) || !gsr::aligned4(order) || !gsr::aligned4(partners) || !gsr::aligned8(pairs) ||
        !gsr::aligned4(loss) || !gsr::aligned4(terms_or_null) || !gsr::aligned4(scratch))
        return fail(GSR_ERR_INVALID_ARG, "gsr_normal_consistency_forward: misaligned pointer (floats, order / partners, scratch: 4 bytes, faces / pairs: 8)");
    const size_t need = gsr_normal_consistency_scratch_bytes(F);
    if (F > 0 && scratch_bytes < need)
        return fail(GSR_ERR_INVALID_ARG, "gsr_normal_consistency_forward: scratch too small (%zu of %zu bytes)", scratch_bytes, need);
    hipStream_t stream = (hipStream_t)stream_;
    if (F == 0) {
        GSR_HIP(hipMemsetAsync(loss, 0, sizeof(float), stream));
        return GSR_OK;
    }
    const uint32_t n = (uint32_t)(3 * F), blocks = gsr::blocks_of(n, gsr::kLossThreads);
    float* partials = static_cast<float*>(scratch);
    hipLaunchKernelGGL(gsr::nc_forward_kernel, dim3(blocks), dim3(gsr::kLossThreads), 0, stream, n, (long long)V, verts,
                       reinterpret_cast<const long long*>(faces), order, partners, partials, terms_or_null);
    hipLaunchKernelGGL(gsr::nc_sum_kernel, dim3(1), dim3(gsr::kSumThreads), 0, stream, blocks, (const float*)partials,
                       reinterpret_cast<const long long*>(pairs), loss);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_normal_consistency_backward(int64_t V, int64_t F, const float* verts, const int64_t* faces, const int32_t* order, const int32_t* partners,
                                    const int64_t* pairs, const float* grad_loss, float* grad_verts, void* stream_) {
    if (const char* why = gsr::bad_mesh(V, F)) return fail(GSR_ERR_INVALID_ARG, "gsr_normal_consistency_backward: %s", why);
    if ((V > 0 && (!verts || !grad_verts)) || (F > 0 && (!faces || !order || !partners || !pairs || !grad_loss)))
        return fail(GSR_ERR_INVALID_ARG, "gsr_normal_consistency_backward: null pointer");
    if (!gsr::aligned4(verts) || !gsr::aligned8(faces) || !gsr::aligned4(order) || !gsr::aligned4(partners) || !gsr::aligned8(pairs) ||
        !gsr::aligned4(grad_loss) || !gsr::aligned4(grad_verts))
        return fail(GSR_ERR_INVALID_ARG, "gsr_normal_consistency_backward: misaligned pointer (floats, order / partners: 4 bytes, faces / pairs: 8)");
    if (V == 0) return GSR_OK;
    hipStream_t stream = (hipStream_t)stream_;
    GSR_HIP(hipMemsetAsync(grad_verts, 0, (size_t)V * 3u * sizeof(float), stream));
    if (F == 0) return GSR_OK;
    const uint32_t n = (uint32_t)(3 * F);
    hipLaunchKernelGGL(gsr::nc_backward_kernel, dim3(gsr::blocks_of(n, gsr::kLossThreads)), dim3(gsr::kLossThreads), 0, stream, n, (long long)V, verts,
                       reinterpret_cast<const long long*>(faces), order, partners, reinterpret_cast<const long long*>(pairs), grad_loss,
                       grad_verts);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

}  // extern "C"
