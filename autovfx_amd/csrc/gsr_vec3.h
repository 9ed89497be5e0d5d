// gsr_vec3.h -- what the kernel units that work on triangle meshes (gsr_meshattrs.hip, gsr_meshloss.hip, gsr_meshquery.hip,
// gsr_texture.hip) share, written once: a 3-vector and its operations, and the checked gather of a face's corners.
// Every unit is built with -ffp-contract=off and its contract fixes the order of every fp32 operation, so each function below IS a
// piece of those contracts: one multiplication, addition or division per operation written, sums associated as the parentheses say.
// Changing an expression tree here changes the bits of every unit that calls it (the units' tests against their numpy restatements,
// autovfx_amd/_mesh_host.py among them, say so at once).  Device only; inline in an unnamed namespace: each unit gets its own copy.
// What is NOT here: anything only one unit uses (7j's face normal and its backward, gsr_meshquery.hip's guarded division and centroid);
// gsr_bound.hip, which keeps its array form because its forward measured slower with Vec3; and a helper for the three float atomics
// of a vertex's gradient, behind which the backward kernels measured slower (DESIGN.md section 4 for both).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>

namespace gsr {
namespace {

struct Vec3 {
    float x, y, z;
};
__device__ __forceinline__ Vec3 load3(const float* __restrict__ rows, size_t i) {
    const float* p = rows + 3 * i;
    return {p[0], p[1], p[2]};
}
__device__ __forceinline__ Vec3 sub(const Vec3& u, const Vec3& v) { return {u.x - v.x, u.y - v.y, u.z - v.z}; }
__device__ __forceinline__ Vec3 add(const Vec3& u, const Vec3& v) { return {u.x + v.x, u.y + v.y, u.z + v.z}; }
__device__ __forceinline__ Vec3 neg(const Vec3& u) { return {-u.x, -u.y, -u.z}; }
__device__ __forceinline__ Vec3 scale(float s, const Vec3& v) { return {s * v.x, s * v.y, s * v.z}; }
__device__ __forceinline__ Vec3 over(const Vec3& v, float d) { return {v.x / d, v.y / d, v.z / d}; }
// u + s v, a multiplication and an addition per axis
__device__ __forceinline__ Vec3 along(const Vec3& u, float s, const Vec3& v) { return {u.x + s * v.x, u.y + s * v.y, u.z + s * v.z}; }
__device__ __forceinline__ float dot(const Vec3& u, const Vec3& v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
__device__ __forceinline__ Vec3 cross(const Vec3& u, const Vec3& v) {
    return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}
__device__ __forceinline__ float norm(const Vec3& v) { return sqrtf(dot(v, v)); }

// ---- a face's corners ---------------------------------------------------------------------------------------------------------------

struct FaceCorners {
    long long i0, i1, i2;
    Vec3 v0, v1, v2;
};
// false: an index outside [0, V), nothing read from verts.  (The index test is written here and, alone, in gsr_meshloss.hip's
// load_incidence: behind a helper of its own the kernels that call the gather compiled to other instruction streams.)
__device__ __forceinline__ bool load_face_checked(const float* __restrict__ verts, const long long* __restrict__ faces, long long V, size_t f,
                                                  FaceCorners& t) {
    t.i0 = faces[3 * f + 0], t.i1 = faces[3 * f + 1], t.i2 = faces[3 * f + 2];
    if (t.i0 < 0 || t.i0 >= V || t.i1 < 0 || t.i1 >= V || t.i2 < 0 || t.i2 >= V) return false;
    t.v0 = load3(verts, (size_t)t.i0), t.v1 = load3(verts, (size_t)t.i1), t.v2 = load3(verts, (size_t)t.i2);
    return true;
}

}  // namespace
}  // namespace gsr
