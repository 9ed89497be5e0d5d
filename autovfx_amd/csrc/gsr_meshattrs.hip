// gsr_meshattrs.hip -- what pytorch3d does with a mesh beside rasterizing it: face areas and normals, and the interpolation of per-face
// vertex attributes over the rasterizer's fragments, each with its backward (include/gsr.h: gsr_face_areas_normals,
// gsr_face_areas_normals_backward, gsr_interp_face_attrs, gsr_interp_face_attrs_backward; the contract is the module docstring of
// autovfx_amd/meshattrs.py and DESIGN.md 7j).  Five kernels, no scratch, no host read:
//   face forward     one lane per face: three int64 indices, a dependent gather of nine floats, one sqrt, four divisions
//   face backward    one lane per face: the forward again, then nine float atomic adds into grad_verts (zeroed on the stream first)
//   interp forward   one lane per output element (slot p, channel d): consecutive lanes write consecutive floats at every D, and the
//                    lanes of a slot read one face's rows
//   grad_bary        one lane per (slot, corner): a sum over d in ascending order, no atomics
//   grad_attrs       one lane per (slot, corner, channel): one float atomic add each; the 3 D lanes of a slot add to 12 D consecutive
//                    bytes of grad_attrs (zeroed on the stream first)
// The three slot kernels give a workgroup kSlots consecutive slots and walk slot * width with a 32-bit index, so the per-lane division
// is a 32-bit one whatever P is.
// fp32 throughout, -ffp-contract=off, IEEE division and sqrt: the numpy restatements compute the same bits; only the order in which the
// atomics arrive is free.
#include "gsr_internal.h"
#include "gsr_vec3.h"

#include <limits.h>
#include <math.h>

namespace gsr {
namespace {

constexpr int kAttrThreads = 256;
constexpr uint32_t kSlots = 256;         // slots per workgroup of the three slot kernels
constexpr int kAttrMaxD = 65536;         // kSlots * 3 * D stays below 2^32
constexpr float kNormalEps = 1e-6f;

// ---- the contract's arithmetic: restated operation by operation in autovfx_amd/meshattrs.py (the 3-vectors and the gather: gsr_vec3.h) ---

// a = v1 - v0, b = v2 - v0, c = a x b, n = |c|
__device__ __forceinline__ void face_cross(const FaceCorners& t, Vec3& a, Vec3& b, Vec3& c, float& n) {
    a = sub(t.v1, t.v0), b = sub(t.v2, t.v0);
    c = cross(a, b);
    n = norm(c);
}
// g_c from the normal's gradient gn: the projection off m = c / n, over n; below the clamp (and for a NaN n) the forward is c / 1e-6
__device__ __forceinline__ Vec3 normal_backward(const Vec3& c, float n, const Vec3& gn) {
    if (n >= kNormalEps) {
        const Vec3 m = over(c, n);
        return over(sub(gn, scale(dot(m, gn), m)), n);
    }
    return over(gn, kNormalEps);
}

__global__ void __launch_bounds__(kAttrThreads) face_areas_normals_kernel(long long V, long long F, const float* __restrict__ verts,
                                                                          const long long* __restrict__ faces, float* __restrict__ areas,
                                                                          float* __restrict__ normals) {
    const long long f = (long long)blockIdx.x * kAttrThreads + threadIdx.x;
    if (f >= F) return;
    FaceCorners t;
    float area = 0.0f;
    Vec3 normal = {0.0f, 0.0f, 0.0f};
    if (load_face_checked(verts, faces, V, (size_t)f, t)) {
        Vec3 a, b, c;
        float n;
        face_cross(t, a, b, c, n);
        area = n / 2.0f;
        normal = over(c, fmaxf(n, kNormalEps));
    }
    areas[f] = area;
    normals[3 * f + 0] = normal.x, normals[3 * f + 1] = normal.y, normals[3 * f + 2] = normal.z;
}

__global__ void __launch_bounds__(kAttrThreads) face_areas_normals_backward_kernel(long long V, long long F, const float* __restrict__ verts,
                                                                                   const long long* __restrict__ faces,
                                                                                   const float* __restrict__ grad_areas,
                                                                                   const float* __restrict__ grad_normals,
                                                                                   float* __restrict__ grad_verts) {
    const long long f = (long long)blockIdx.x * kAttrThreads + threadIdx.x;
    if (f >= F) return;
    FaceCorners t;
    if (!load_face_checked(verts, faces, V, (size_t)f, t)) return;
    const float garea = grad_areas[f];                   // (both gradients are asked for before the arithmetic waits for the corners)
    const Vec3 gn = load3(grad_normals, (size_t)f);
    Vec3 a, b, c;
    float n;
    face_cross(t, a, b, c, n);
    // the area's part: d(n / 2) / dc = c / (2 n), nothing at n == 0
    Vec3 h = {0.0f, 0.0f, 0.0f};
    if (n > 0.0f) h = over(scale(garea, c), 2.0f * n);
    const Vec3 gc = add(h, normal_backward(c, n, gn));
    const Vec3 ga = cross(b, gc), gb = cross(gc, a);
    float* d0 = grad_verts + 3 * (size_t)t.i0;
    float* d1 = grad_verts + 3 * (size_t)t.i1;
    float* d2 = grad_verts + 3 * (size_t)t.i2;
    atomicAdd(d0 + 0, -(ga.x + gb.x)), atomicAdd(d0 + 1, -(ga.y + gb.y)), atomicAdd(d0 + 2, -(ga.z + gb.z));
    atomicAdd(d1 + 0, ga.x), atomicAdd(d1 + 1, ga.y), atomicAdd(d1 + 2, ga.z);
    atomicAdd(d2 + 0, gb.x), atomicAdd(d2 + 1, gb.y), atomicAdd(d2 + 2, gb.z);
}

// The slots [p0, p0 + slots) of a workgroup, `width` work items per slot: item l belongs to slot p0 + l / width.
__device__ inline uint32_t slots_of_block(long long P, long long& p0) {
    p0 = (long long)blockIdx.x * kSlots;
    const long long left = P - p0;
    return left < (long long)kSlots ? (uint32_t)left : kSlots;
}

__global__ void __launch_bounds__(kAttrThreads) interp_forward_kernel(long long P, long long F, uint32_t D, const long long* __restrict__ pix_to_face,
                                                                      const float* __restrict__ bary, const float* __restrict__ attrs,
                                                                      float* __restrict__ out) {
    long long p0;
    const uint32_t work = slots_of_block(P, p0) * D;
    for (uint32_t l = threadIdx.x; l < work; l += kAttrThreads) {
        const uint32_t s = l / D, d = l - s * D;
        const size_t p = (size_t)p0 + s;
        const long long f = pix_to_face[p];
        float v = 0.0f;
        if (f >= 0 && f < F) {
            const float* a = attrs + (size_t)f * 3u * D + d;
            const float* w = bary + 3 * p;
            v = (w[0] * a[0] + w[1] * a[D]) + w[2] * a[2 * (size_t)D];
        }
        out[(size_t)p0 * D + l] = v;
    }
}

__global__ void __launch_bounds__(kAttrThreads) interp_grad_bary_kernel(long long P, long long F, uint32_t D, const long long* __restrict__ pix_to_face,
                                                                        const float* __restrict__ attrs, const float* __restrict__ grad_out,
                                                                        float* __restrict__ grad_bary) {
    long long p0;
    const uint32_t work = slots_of_block(P, p0) * 3u;
    for (uint32_t l = threadIdx.x; l < work; l += kAttrThreads) {
        const uint32_t s = l / 3u, k = l - s * 3u;
        const size_t p = (size_t)p0 + s;
        const long long f = pix_to_face[p];
        float acc = 0.0f;
        if (f >= 0 && f < F) {
            const float* a = attrs + ((size_t)f * 3u + k) * D;
            const float* g = grad_out + p * D;
            acc = g[0] * a[0];
            for (uint32_t d = 1; d < D; ++d) acc = acc + g[d] * a[d];
        }
        grad_bary[(size_t)p0 * 3u + l] = acc;
    }
}

__global__ void __launch_bounds__(kAttrThreads) interp_grad_attrs_kernel(long long P, long long F, uint32_t D, const long long* __restrict__ pix_to_face,
                                                                         const float* __restrict__ bary, const float* __restrict__ grad_out,
                                                                         float* __restrict__ grad_attrs) {
    long long p0;
    const uint32_t width = 3u * D;
    const uint32_t work = slots_of_block(P, p0) * width;
    for (uint32_t l = threadIdx.x; l < work; l += kAttrThreads) {
        const uint32_t s = l / width, j = l - s * width;
        const uint32_t k = j / D, d = j - k * D;
        const size_t p = (size_t)p0 + s;
        const long long f = pix_to_face[p];
        if (f < 0 || f >= F) continue;
        atomicAdd(grad_attrs + (size_t)f * width + j, bary[3 * p + k] * grad_out[p * D + d]);
    }
}

const char* bad_counts(int64_t a, int64_t b) {
    if (a < 0 || b < 0) return "negative count";
    if (a >= ((int64_t)1 << 31) || b >= ((int64_t)1 << 31)) return "a count of 2^31 or more";
    return nullptr;
}

}  // namespace
}  // namespace gsr

using gsr::fail;

extern "C" {

int gsr_face_areas_normals(int64_t V, int64_t F, const float* verts, const int64_t* faces, float* areas, float* normals, void* stream_) {
    if (const char* why = gsr::bad_counts(V, F)) return fail(GSR_ERR_INVALID_ARG, "gsr_face_areas_normals: %s", why);
    if ((V > 0 && !verts) || (F > 0 && (!faces || !areas || !normals))) return fail(GSR_ERR_INVALID_ARG, "gsr_face_areas_normals: null pointer");
    if (!gsr::aligned4(verts) || !gsr::aligned8(faces) || !gsr::aligned4(areas) || !gsr::aligned4(normals))
        return fail(GSR_ERR_INVALID_ARG, "gsr_face_areas_normals: misaligned pointer (floats: 4 bytes, faces: 8)");
    if (F == 0) return GSR_OK;
    hipLaunchKernelGGL(gsr::face_areas_normals_kernel, dim3(gsr::blocks_of(F, gsr::kAttrThreads)), dim3(gsr::kAttrThreads), 0, (hipStream_t)stream_,
                       (long long)V, (long long)F, verts, reinterpret_cast<const long long*>(faces), areas, normals);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_face_areas_normals_backward(int64_t V, int64_t F, const float* verts, const int64_t* faces, const float* grad_areas,
                                    const float* grad_normals, float* grad_verts, void* stream_) {
    if (const char* why = gsr::bad_counts(V, F)) return fail(GSR_ERR_INVALID_ARG, "gsr_face_areas_normals_backward: %s", why);
    if ((V > 0 && (!verts || !grad_verts)) || (F > 0 && (!faces || !grad_areas || !grad_normals)))
        return fail(GSR_ERR_INVALID_ARG, "gsr_face_areas_normals_backward: null pointer");
    if (!gsr::aligned4(verts) || !gsr::aligned8(faces) || !gsr::aligned4(grad_areas) || !gsr::aligned4(grad_normals) || !gsr::aligned4(grad_verts))
        return fail(GSR_ERR_INVALID_ARG, "gsr_face_areas_normals_backward: misaligned pointer (floats: 4 bytes, faces: 8)");
    if (V == 0) return GSR_OK;
    hipStream_t stream = (hipStream_t)stream_;
    GSR_HIP(hipMemsetAsync(grad_verts, 0, (size_t)V * 3u * sizeof(float), stream));
    if (F == 0) return GSR_OK;
    hipLaunchKernelGGL(gsr::face_areas_normals_backward_kernel, dim3(gsr::blocks_of(F, gsr::kAttrThreads)), dim3(gsr::kAttrThreads), 0, stream,
                       (long long)V, (long long)F, verts, reinterpret_cast<const long long*>(faces), grad_areas, grad_normals, grad_verts);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_interp_face_attrs(int64_t P, int64_t F, int D, const int64_t* pix_to_face, const float* bary, const float* attrs, float* out,
                          void* stream_) {
    if (const char* why = gsr::bad_counts(P, F)) return fail(GSR_ERR_INVALID_ARG, "gsr_interp_face_attrs: %s", why);
    if (D < 1 || D > gsr::kAttrMaxD) return fail(GSR_ERR_INVALID_ARG, "gsr_interp_face_attrs: D = %d (1 to %d)", D, gsr::kAttrMaxD);
    if ((P > 0 && (!pix_to_face || !bary || !out)) || (F > 0 && !attrs)) return fail(GSR_ERR_INVALID_ARG, "gsr_interp_face_attrs: null pointer");
    if (!gsr::aligned8(pix_to_face) || !gsr::aligned4(bary) || !gsr::aligned4(attrs) || !gsr::aligned4(out))
        return fail(GSR_ERR_INVALID_ARG, "gsr_interp_face_attrs: misaligned pointer (floats: 4 bytes, pix_to_face: 8)");
    if (P == 0) return GSR_OK;
    hipLaunchKernelGGL(gsr::interp_forward_kernel, dim3(gsr::blocks_of(P, gsr::kSlots)), dim3(gsr::kAttrThreads), 0, (hipStream_t)stream_,
                       (long long)P, (long long)F, (uint32_t)D, reinterpret_cast<const long long*>(pix_to_face), bary, attrs, out);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_interp_face_attrs_backward(int64_t P, int64_t F, int D, const int64_t* pix_to_face, const float* bary, const float* attrs,
                                   const float* grad_out, float* grad_bary, float* grad_attrs, void* stream_) {
    if (const char* why = gsr::bad_counts(P, F)) return fail(GSR_ERR_INVALID_ARG, "gsr_interp_face_attrs_backward: %s", why);
    if (D < 1 || D > gsr::kAttrMaxD) return fail(GSR_ERR_INVALID_ARG, "gsr_interp_face_attrs_backward: D = %d (1 to %d)", D, gsr::kAttrMaxD);
    if ((P > 0 && (!pix_to_face || !bary || !grad_out || !grad_bary)) || (F > 0 && (!attrs || !grad_attrs)))
        return fail(GSR_ERR_INVALID_ARG, "gsr_interp_face_attrs_backward: null pointer");
    if (!gsr::aligned8(pix_to_face) || !gsr::aligned4(bary) || !gsr::aligned4(attrs) || !gsr::aligned4(grad_out) || !gsr::aligned4(grad_bary) ||
        !gsr::aligned4(grad_attrs))
        return fail(GSR_ERR_INVALID_ARG, "gsr_interp_face_attrs_backward: misaligned pointer (floats: 4 bytes, pix_to_face: 8)");
    hipStream_t stream = (hipStream_t)stream_;
    if (F > 0) GSR_HIP(hipMemsetAsync(grad_attrs, 0, (size_t)F * 3u * (size_t)D * sizeof(float), stream));
    if (P == 0) return GSR_OK;
    const dim3 grid(gsr::blocks_of(P, gsr::kSlots)), block(gsr::kAttrThreads);
    const long long* pix = reinterpret_cast<const long long*>(pix_to_face);
    hipLaunchKernelGGL(gsr::interp_grad_bary_kernel, grid, block, 0, stream, (long long)P, (long long)F, (uint32_t)D, pix, attrs, grad_out, grad_bary);
    if (F > 0)
        hipLaunchKernelGGL(gsr::interp_grad_attrs_kernel, grid, block, 0, stream, (long long)P, (long long)F, (uint32_t)D, pix, bary, grad_out, grad_attrs);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

}  // extern "C"
