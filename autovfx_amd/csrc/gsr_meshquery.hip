// gsr_meshquery.hip -- the closest triangle of a mesh to every query point (include/gsr.h: gsr_closest_tri_plan, gsr_closest_tri_query).
//
// What Open3D's RaycastingScene.compute_closest_points answers for the melting frames of the frame loop (scene_representation.py:
// 385-412) and for object extraction (extract/extract_object.py:105-110): primitive id, squared distance, closest point.  The result
// is a pointwise function of the input: the valid face with the smallest (d(q, f), f), so any exact search gives the
// same bits.  This one is the tree of gsr_knn.hip over triangles (gsr_tree.h), all stream-ordered, no host read, no float atomics:
//
//   plan    : bounds over the valid faces' centroids (per-workgroup partials); 63-bit Morton codes of the centroids, an invalid face
//             (an index outside [0, V), a non-finite coordinate) gets 2^63 and sorts last; the library's radix sort, low word then
//             high word, stable (morton_sort); one 48-byte record per face in sorted order (three float4 a, b, c, the face index in
//             a.w; an invalid face: NaNs and index ~0); leaf boxes = the union of the 64 triangles' own boxes (valid members only);
//             levels of 16 (tree_levels); the header last, so that a plan is valid only once its build has run.
//   query   : one wave per 64 queries, one lane per query, one slot (d, face) per lane: walk_tree below, with a PointProbe.
// The plan is self-describing: its header holds F and the plan's size, and the query kernel derives every count and offset from that F
// (tri_layout, the function the host sized the plan with) and compares the total with the plan_bytes it was handed BEFORE anything
// indexes the plan.  A header that does not match answers every query (-1, +inf, 0 0 0): the host cannot see the header without a
// device-to-host read, which a query never does.
// The same plan answers the first triangle a ray hits (gsr_ray_first_hit, DESIGN.md 7m: what trimesh's mesh.ray answers for object
// extraction and removal, extract/extract_object.py:115-159, :424-434, :476-482, :563-606): the same walk with a RayProbe, one slot
// (t, face, barycentrics) per lane.  The walk is written once, over a per-lane probe that supplies what the two queries differ in: the
// box test, the order of a node's children, the scan of a leaf.
// Defines the entry points gsr_closest_tri_plan_bytes, gsr_closest_tri_plan_scratch_bytes, gsr_closest_tri_plan, gsr_closest_tri_query,
// gsr_ray_first_hit.
#include "gsr_tree.h"
#include "gsr_vec3.h"

#include <cfloat>

namespace gsr {
namespace {

constexpr uint32_t kInvalidKey = 1u << 31;       // the high word of an invalid face's code
constexpr uint32_t kNoFace = ~0u;                // the index of an invalid face's record, and of an empty slot
constexpr uint32_t kPlanMagic = 0x51495254u;     // "TRIQ"
constexpr int64_t kMaxFaces = (int64_t)1 << 30;  // refused from here on (the radix sort's limit)
constexpr int64_t kMaxVerts = (int64_t)1 << 31;
constexpr int64_t kMaxQueries = (int64_t)1 << 31;

// The first 256 bytes of a plan.
struct TriHeader {
    uint32_t magic, F;
    unsigned long long plan_bytes;
};

// The tree of gsr_tree.h over the Morton-sorted faces, and where it lies in a plan over F < 2^30 faces: pure arithmetic, the same on
// the host that sizes a plan and in the kernel that reads one.
struct TriTree {
    uint32_t leaves;
    int top;
    size_t records, boxes, bytes;   // byte offsets in the plan; bytes = the whole
};
__host__ __device__ inline TriTree tri_layout(uint32_t F) {
    const TreeShape shape = tree_shape(F);
    TriTree t = {};
    t.leaves = shape.leaves;
    t.top = shape.top;
    t.records = kAlign;
    t.boxes = align_up(t.records + 48 * (size_t)F);
    t.bytes = align_up(t.boxes + 32 * (size_t)shape.boxes);
    return t;
}

// Byte offsets of the regions of the build's scratch (each 256-byte aligned); bytes = the whole.
struct TriScratch {
    size_t keys, keys_alt, vals, vals_alt, key_hi, radix, partials, bytes;
};
TriScratch tri_scratch(uint32_t F) {
    TriScratch L = {};
    if (F == 0) return L;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t here = at; at = align_up(at + bytes); return here; };
    L.keys = take(4 * (size_t)F);
    L.keys_alt = take(4 * (size_t)F);
    L.vals = take(4 * (size_t)F);
    L.vals_alt = take(4 * (size_t)F);
    L.key_hi = take(4 * (size_t)F);
    L.radix = take(radix_scratch_words(F) * sizeof(uint32_t));
    L.partials = take(32 * (size_t)kBoundsBlocks);
    L.bytes = at;
    return L;
}

__device__ __forceinline__ float guarded(float num, float den) { return den != 0.0f ? num / den : 0.0f; }

// The three corners of face f; false for an invalid face: an index outside [0, V) (the corners are then not read) or a coordinate
// that is not finite.
__device__ __forceinline__ bool load_face(int64_t V, const float* __restrict__ verts, const long long* __restrict__ faces, uint32_t f,
                                          Vec3& a, Vec3& b, Vec3& c) {
    FaceCorners t;
    if (!load_face_checked(verts, faces, V, f, t)) return false;
    a = t.v0, b = t.v1, c = t.v2;
    return finite3(a.x, a.y, a.z) && finite3(b.x, b.y, b.z) && finite3(c.x, c.y, c.z);
}
// (it only steers the sort: an overflow to inf lands in cell 0 or the last one)
__device__ __forceinline__ Vec3 centroid(const Vec3& a, const Vec3& b, const Vec3& c) {
    return {((a.x + b.x) + c.x) / 3.0f, ((a.y + b.y) + c.y) / 3.0f, ((a.z + b.z) + c.z) / 3.0f};
}

__global__ __launch_bounds__(256) void tri_bounds_kernel(int64_t V, const float* __restrict__ verts, uint32_t F,
                                                         const long long* __restrict__ faces, float4* __restrict__ partials) {
    __shared__ float s_red[24];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t f = blockIdx.x * 256u + threadIdx.x; f < F; f += kBoundsBlocks * 256u) {
        Vec3 a, b, c;
        if (load_face(V, verts, faces, f, a, b, c)) {
            const Vec3 m = centroid(a, b, c);
            lo[0] = fminf(lo[0], m.x); lo[1] = fminf(lo[1], m.y); lo[2] = fminf(lo[2], m.z);
            hi[0] = fmaxf(hi[0], m.x); hi[1] = fmaxf(hi[1], m.y); hi[2] = fmaxf(hi[2], m.z);
        }
    }
    block_minmax(lo, hi, s_red);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        partials[2 * blockIdx.x + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

__global__ __launch_bounds__(256) void tri_codes_kernel(int64_t V, const float* __restrict__ verts, uint32_t F,
                                                        const long long* __restrict__ faces, const float4* __restrict__ partials,
                                                        uint32_t* __restrict__ key_lo, uint32_t* __restrict__ key_hi) {
    __shared__ float s_red[24];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (threadIdx.x < kBoundsBlocks) {
        const float4 a = partials[2 * threadIdx.x], b = partials[2 * threadIdx.x + 1];
        lo[0] = a.x; lo[1] = a.y; lo[2] = a.z; hi[0] = b.x; hi[1] = b.y; hi[2] = b.z;
    }
    block_minmax(lo, hi, s_red);
    for (uint32_t f = blockIdx.x * 256u + threadIdx.x; f < F; f += gridDim.x * 256u) {
        Vec3 a, b, c;
        uint64_t code = (uint64_t)kInvalidKey << 32;
        if (load_face(V, verts, faces, f, a, b, c)) {
            const Vec3 m = centroid(a, b, c);
            code = spread21(grid_cell(m.x, lo[0], hi[0])) | (spread21(grid_cell(m.y, lo[1], hi[1])) << 1) |
                   (spread21(grid_cell(m.z, lo[2], hi[2])) << 2);
        }
        key_lo[f] = (uint32_t)code;
        key_hi[f] = (uint32_t)(code >> 32);
    }
}

// one wave per leaf: the sorted faces' records, the leaf's box (the union of its valid triangles' own boxes)
__global__ __launch_bounds__(256) void tri_pack_kernel(int64_t V, const float* __restrict__ verts, uint32_t F,
                                                       const long long* __restrict__ faces, const uint32_t* __restrict__ order,
                                                       float4* __restrict__ records, float4* __restrict__ leaf_boxes) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (s < F) {
        const uint32_t f = order[s];
        Vec3 a, b, c;
        if (f < F && load_face(V, verts, faces, f, a, b, c)) {
            records[3 * (size_t)s] = make_float4(a.x, a.y, a.z, __uint_as_float(f));
            records[3 * (size_t)s + 1] = make_float4(b.x, b.y, b.z, 0.0f);
            records[3 * (size_t)s + 2] = make_float4(c.x, c.y, c.z, 0.0f);
            lo[0] = fminf(fminf(a.x, b.x), c.x); lo[1] = fminf(fminf(a.y, b.y), c.y); lo[2] = fminf(fminf(a.z, b.z), c.z);
            hi[0] = fmaxf(fmaxf(a.x, b.x), c.x); hi[1] = fmaxf(fmaxf(a.y, b.y), c.y); hi[2] = fmaxf(fmaxf(a.z, b.z), c.z);
        } else {
            const float4 none = make_float4(NAN, NAN, NAN, __uint_as_float(kNoFace));
            records[3 * (size_t)s] = none;
            records[3 * (size_t)s + 1] = none;
            records[3 * (size_t)s + 2] = none;
        }
    }
    for (int a = 0; a < 3; ++a) { lo[a] = wave_min(lo[a]); hi[a] = wave_max(hi[a]); }
    const uint32_t leaf = s / kLeaf;
    if ((threadIdx.x & 63) == 0 && leaf * kLeaf < F) {
        leaf_boxes[2 * (size_t)leaf] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        leaf_boxes[2 * (size_t)leaf + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

// the last kernel of a build
__global__ void tri_header_kernel(TriHeader* header, uint32_t F, unsigned long long plan_bytes) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        TriHeader h;
        h.magic = kPlanMagic;
        h.F = F;
        h.plan_bytes = plan_bytes;
        *header = h;
    }
}

struct Query {
    float x, y, z;
    bool active;   // in range and finite: the others answer (-1, +inf, 0 0 0)
};
// A lane's slot: the best (d, face) so far and the point p' its d_tri used (relative to the query).
struct Slot {
    float d;
    uint32_t face;
    Vec3 p;
};

// d(q, f) of the contract (autovfx_amd/meshquery.py restates it in numpy, operation for operation).
//   A = a - q, B = b - q, C = c - q: the triangle translated by -q, so that every later rounding error is relative to the distance
//   scale, not to the coordinates.  p' = the closest point of (A, B, C) to the origin by the vertex / edge / interior region tests
//   (Ericson, Real-Time Collision Detection 5.1.5), the first region that matches in the order below; every division is guarded (a zero
//   denominator takes the region's first end point), so a degenerate triangle gives a finite answer.  d_tri = |p'|^2.
//   d_box = box_bound of the triangle's own box (in the original coordinates), d_vtx = the smallest of |A|^2, |B|^2, |C|^2.
//   d = fmin(fmax(d_tri, d_box), d_vtx): fmax / fmin ignore a NaN, so an overflowed d_tri falls back on the clamps.
// The true distance lies in [d_box, d_vtx], so the clamps only remove rounding error -- and they make the search exact: see walk_tree.
__device__ __forceinline__ float tri_dist(const Vec3& a, const Vec3& b, const Vec3& c, float d_box, const Query& q, Vec3& p) {
    const Vec3 qv = {q.x, q.y, q.z};
    const Vec3 A = sub(a, qv), B = sub(b, qv), C = sub(c, qv);
    const Vec3 ab = sub(B, A), ac = sub(C, A);
    const Vec3 ap = neg(A), bp = neg(B), cp = neg(C);
    const float d1 = dot(ab, ap), d2 = dot(ac, ap);
    const float d3 = dot(ab, bp), d4 = dot(ac, bp);
    const float d5 = dot(ab, cp), d6 = dot(ac, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e = d4 - d3, g = d5 - d6;
    if (d1 <= 0.0f && d2 <= 0.0f) {
        p = A;
    } else if (d3 >= 0.0f && d4 <= d3) {
        p = B;
    } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        p = along(A, guarded(d1, d1 - d3), ab);
    } else if (d6 >= 0.0f && d5 <= d6) {
        p = C;
    } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        p = along(A, guarded(d2, d2 - d6), ac);
    } else if (va <= 0.0f && e >= 0.0f && g >= 0.0f) {
        p = along(B, guarded(e, e + g), sub(C, B));
    } else {
        const float den = (va + vb) + vc;
        p = along(along(A, guarded(vb, den), ab), guarded(vc, den), ac);
    }
    const float d_tri = dot(p, p);
    const float d_vtx = fminf(fminf(dot(A, A), dot(B, B)), dot(C, C));
    return fminf(fmaxf(d_tri, d_box), d_vtx);
}

// `cnt` records of a leaf in LDS against the lane's slot.  A record whose own box is strictly farther than the slot cannot enter it
// (d >= d_box by the clamp), so its region tests are skipped.
__device__ __forceinline__ void slot_scan(const float4* leaf, int cnt, const Query& q, Slot& slot) {
    for (int k = 0; k < cnt; ++k) {
        const float4 ra = leaf[3 * k], rb = leaf[3 * k + 1], rc = leaf[3 * k + 2];
        const uint32_t face = __float_as_uint(ra.w);
        if (face == kNoFace) continue;   // an invalid face: never answered (wave-uniform)
        const float4 lo = make_float4(fminf(fminf(ra.x, rb.x), rc.x), fminf(fminf(ra.y, rb.y), rc.y), fminf(fminf(ra.z, rb.z), rc.z), 0.0f);
        const float4 hi = make_float4(fmaxf(fmaxf(ra.x, rb.x), rc.x), fmaxf(fmaxf(ra.y, rb.y), rc.y), fmaxf(fmaxf(ra.z, rb.z), rc.z), 0.0f);
        const float d_box = box_bound(lo, hi, q.x, q.y, q.z);
        if (!q.active || d_box > slot.d) continue;
        Vec3 p;
        const float d = tri_dist({ra.x, ra.y, ra.z}, {rb.x, rb.y, rb.z}, {rc.x, rc.y, rc.z}, d_box, q, p);
        if (d < slot.d || (d == slot.d && face < slot.face)) {
            slot.d = d;
            slot.face = face;
            slot.p = p;
        }
    }
}

// ---- the first triangle a ray hits (gsr_ray_first_hit; meshquery.first_hits_host restates it in numpy) ----------------
// The second query on the same plan.  The answer is the valid face with the smallest (t(ray, f), f) among the faces the ray hits, a
// pointwise function of the input like the closest triangle.

constexpr float kSlabPad = 1.00000024f;   // 1 + 2 ulp on the far end of a slab interval (Ize, "Robust BVH Ray Traversal")

// A lane's ray and what is computed of it once: the shear of the watertight test (Woop, Benthin, Wald: kz = the axis of the largest
// |d|, ties to the lowest axis; kx, ky = the next two cyclically, swapped when d[kz] < 0; Sx = d[kx] / d[kz], Sy = d[ky] / d[kz],
// Sz = 1 / d[kz]) and the reciprocals of the slab test (inv[k] = 1 / d[k], unused where d[k] == 0).
struct Ray {
    Vec3 o, d, inv;
    int kx, ky, kz;
    float Sx, Sy, Sz;
    bool active;   // in range, six finite components, a direction that is not zero: the others answer (-1, +inf, 0 0 0)
};
struct HitSlot {
    float t;
    uint32_t face;
    float u, v, w;   // U / det, V / det, W / det: the weights of the face's corners a, b, c
};

__device__ __forceinline__ float pick(const Vec3& v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }   // (selects, no scratch)

__device__ __forceinline__ Ray make_ray(float ox, float oy, float oz, float dx, float dy, float dz) {
    Ray r = {};
    r.o = {ox, oy, oz};
    r.d = {dx, dy, dz};
    r.active = finite3(ox, oy, oz) && finite3(dx, dy, dz) && (dx != 0.0f || dy != 0.0f || dz != 0.0f);
    int kz = 0;
    float most = fabsf(dx);
    if (fabsf(dy) > most) { kz = 1; most = fabsf(dy); }
    if (fabsf(dz) > most) kz = 2;
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const float dkz = pick(r.d, kz);
    if (dkz < 0.0f) { const int s = kx; kx = ky; ky = s; }
    r.kx = kx; r.ky = ky; r.kz = kz;
    r.Sx = pick(r.d, kx) / dkz;
    r.Sy = pick(r.d, ky) / dkz;
    r.Sz = 1.0f / dkz;
    r.inv = {1.0f / dx, 1.0f / dy, 1.0f / dz};
    return r;
}

// One axis of the slab test: the interval of t in which o + t d lies between lo and hi on this axis.  d != 0: the two products
// (lo - o) inv and (hi - o) inv, ordered by the sign of inv.  d == 0: all of the line when lo <= o <= hi, else nothing (+inf, -inf).
__device__ __forceinline__ void slab_axis(float lo, float hi, float o, float d, float inv, float& near, float& far) {
    if (d != 0.0f) {
        const float a = (lo - o) * inv, b = (hi - o) * inv;
        near = inv < 0.0f ? b : a;
        far = inv < 0.0f ? a : b;
    } else {
        const bool in = lo <= o && o <= hi;
        near = in ? -INFINITY : INFINITY;
        far = in ? INFINITY : -INFINITY;
    }
}
// t_enter = max(0, the three nears), t_exit = (min of the three fars) padded; fmaxf / fminf drop a NaN (0 times an overflowed inv).
// The box is hit iff t_enter <= t_exit.  An empty box (+inf, -inf) never is.
__device__ __forceinline__ void slab(const float4& lo, const float4& hi, const Ray& r, float& t_enter, float& t_exit) {
    float n0, n1, n2, f0, f1, f2;
    slab_axis(lo.x, hi.x, r.o.x, r.d.x, r.inv.x, n0, f0);
    slab_axis(lo.y, hi.y, r.o.y, r.d.y, r.inv.y, n1, f1);
    slab_axis(lo.z, hi.z, r.o.z, r.d.z, r.inv.z, n2, f2);
    t_enter = fmaxf(fmaxf(fmaxf(0.0f, n0), n1), n2);
    t_exit = fminf(fminf(f0, f1), f2) * kSlabPad;
}

// t(ray, f) of the contract; false: the ray misses the face.
//   The corners translated by -o and sheared: Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz], Az = Sz A[kz], B and C alike.
//   U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax: a miss when one of them is < 0 and another > 0 (two-sided).
//   det = (U + V) + W: a miss when 0.  t_tri = ((U Az + V Bz) + W Cz) / det: a miss unless t_tri >= 0 (a NaN misses).
//   t = fmin(fmax(t_tri, t_enter), t_exit) + 0 of the triangle's own box (the + 0 makes a -0 a +0); a t of +inf is a miss.
// The caller has found t_enter <= t_exit.  No double-precision fallback: a ray through an edge may hit both faces or, rarely, neither.
__device__ __forceinline__ bool ray_triangle(const Vec3& a, const Vec3& b, const Vec3& c, const Ray& r, float t_enter, float t_exit,
                                             float& t, float& u, float& v, float& w) {
    const Vec3 A = sub(a, r.o), B = sub(b, r.o), C = sub(c, r.o);
    const float Akz = pick(A, r.kz), Bkz = pick(B, r.kz), Ckz = pick(C, r.kz);
    const float Ax = pick(A, r.kx) - r.Sx * Akz, Ay = pick(A, r.ky) - r.Sy * Akz;
    const float Bx = pick(B, r.kx) - r.Sx * Bkz, By = pick(B, r.ky) - r.Sy * Bkz;
    const float Cx = pick(C, r.kx) - r.Sx * Ckz, Cy = pick(C, r.ky) - r.Sy * Ckz;
    const float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f)) return false;
    const float det = (U + V) + W;
    if (det == 0.0f) return false;
    const float Az = r.Sz * Akz, Bz = r.Sz * Bkz, Cz = r.Sz * Ckz;
    const float t_tri = ((U * Az + V * Bz) + W * Cz) / det;
    if (!(t_tri >= 0.0f)) return false;
    t = fminf(fmaxf(t_tri, t_enter), t_exit) + 0.0f;
    u = U / det;
    v = V / det;
    w = W / det;
    return t < INFINITY;
}

// `cnt` records of a leaf in LDS against the lane's slot.  A record whose own box is missed, or entered strictly after the slot's t,
// cannot enter the slot (t >= t_enter by the clamp), so its triangle test is skipped.
__device__ __forceinline__ void hit_scan(const float4* leaf, int cnt, const Ray& r, HitSlot& slot) {
    for (int k = 0; k < cnt; ++k) {
        const float4 ra = leaf[3 * k], rb = leaf[3 * k + 1], rc = leaf[3 * k + 2];
        const uint32_t face = __float_as_uint(ra.w);
        if (face == kNoFace) continue;   // an invalid face: never answered (wave-uniform)
        const float4 lo = make_float4(fminf(fminf(ra.x, rb.x), rc.x), fminf(fminf(ra.y, rb.y), rc.y), fminf(fminf(ra.z, rb.z), rc.z), 0.0f);
        const float4 hi = make_float4(fmaxf(fmaxf(ra.x, rb.x), rc.x), fmaxf(fmaxf(ra.y, rb.y), rc.y), fmaxf(fmaxf(ra.z, rb.z), rc.z), 0.0f);
        float t_enter, t_exit;
        slab(lo, hi, r, t_enter, t_exit);
        if (!r.active || !(t_enter <= t_exit) || t_enter > slot.t) continue;
        float t, u, v, w;
        if (!ray_triangle({ra.x, ra.y, ra.z}, {rb.x, rb.y, rb.z}, {rc.x, rc.y, rc.z}, r, t_enter, t_exit, t, u, v, w)) continue;
        if (t < slot.t || (t == slot.t && face < slot.face)) {
            slot.t = t;
            slot.face = face;
            slot.u = u; slot.v = v; slot.w = w;
        }
    }
}

// ---- the walk, written once over a per-lane probe ---------------------------------------------------------------------------------
// A probe is a lane's question and its slot, plain scalars in a struct that lives in the kernel's registers.  It supplies:
//   active()              whether the lane asks anything;
//   begin()               what the wave works out once, before the walk (every lane calls it);
//   reaches(lo, hi, at)   whether the box can still hold a member that enters the lane's slot, and the value that decides it;
//   lanes_key / box_key   a kept child's order key, from one of two places -- the lanes that keep it (asked per child, wave-uniform) or
//                         the child's own box (asked once per child lane); the hook a probe does not use passes through;
//   scan(leaf, cnt)       `cnt` records of a leaf in LDS against the slot.
// The two order keys are measured choices and stay different.

// The closest triangle: box_bound against the slot's distance; children keyed by the gap between their box and the box of the wave's
// queries (wlo, whi).
struct PointProbe {
    Query q;
    Slot slot;
    float4 wlo, whi;

    __device__ __forceinline__ bool active() const { return q.active; }
    __device__ __forceinline__ void begin() {
        wlo = make_float4(wave_min(q.active ? q.x : INFINITY), wave_min(q.active ? q.y : INFINITY), wave_min(q.active ? q.z : INFINITY),
                          0.0f);
        whi = make_float4(wave_max(q.active ? q.x : -INFINITY), wave_max(q.active ? q.y : -INFINITY),
                          wave_max(q.active ? q.z : -INFINITY), 0.0f);
    }
    __device__ __forceinline__ bool reaches(const float4& lo, const float4& hi, float& at) const {
        at = box_bound(lo, hi, q.x, q.y, q.z);
        return q.active && !(at > slot.d);
    }
    __device__ __forceinline__ float lanes_key(bool, float) const { return INFINITY; }
    __device__ __forceinline__ float box_key(const float4& clo, const float4& chi, float) const {
        const float gx = fmaxf(fmaxf(clo.x - whi.x, wlo.x - chi.x), 0.0f);
        const float gy = fmaxf(fmaxf(clo.y - whi.y, wlo.y - chi.y), 0.0f);
        const float gz = fmaxf(fmaxf(clo.z - whi.z, wlo.z - chi.z), 0.0f);
        return (gx * gx + gy * gy) + gz * gz;   // never NaN: fmaxf drops one, and the terms are not negative
    }
    __device__ __forceinline__ void scan(const float4* leaf, int cnt) { slot_scan(leaf, cnt, q, slot); }
};

// The first hit: the slab interval against the slot's t; children keyed by the wave minimum of the keeping lanes' t_enter, so the
// box the wave's rays enter first is popped next.
struct RayProbe {
    Ray r;
    HitSlot slot;

    __device__ __forceinline__ bool active() const { return r.active; }
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ bool reaches(const float4& lo, const float4& hi, float& at) const {
        float t_exit;
        slab(lo, hi, r, at, t_exit);
        return r.active && at <= t_exit && !(at > slot.t);
    }
    __device__ __forceinline__ float lanes_key(bool mine, float at) const { return wave_min(mine ? at : INFINITY); }
    __device__ __forceinline__ float box_key(const float4&, const float4&, float key) const { return key; }
    __device__ __forceinline__ void scan(const float4* leaf, int cnt) { hit_scan(leaf, cnt, r, slot); }
};

// What a wave of a query kernel walks with: its lane, its query number and its share of the LDS.
struct Wave {
    int lane;
    uint32_t s;        // this lane's query
    float4* leaf;      // 3 * kLeaf: a staged leaf
    uint32_t* stack;   // kStackDepth
};
// The prologue of both query kernels (256 lanes, four waves of 64 queries each).  False: a wave past the n queries, which returns.
__device__ __forceinline__ bool open_wave(uint32_t n, Wave& w) {
    __shared__ float4 s_leaf[4][3 * kLeaf];
    __shared__ uint32_t s_stack[4][kStackDepth];
    const int wave = threadIdx.x >> 6;
    const uint32_t group = blockIdx.x * 4u + (uint32_t)wave;    // this wave's 64 queries
    if ((unsigned long long)group * kLeaf >= n) return false;
    w.lane = threadIdx.x & 63;
    w.s = group * kLeaf + w.lane;
    w.leaf = s_leaf[wave];
    w.stack = s_stack[wave];
    return true;
}

// Children [first, first + cnt) of `level` kept by some lane, pushed farthest first by their order key so the nearest is popped next
// (gsr_knn.hip's push_children without the own leaf).
template <class Probe>
__device__ __forceinline__ void push_children(const Wave& w, const float4* boxes /* of `level` */, int level, uint32_t first, int cnt,
                                              const Probe& probe, int& top) {
    const int lane = w.lane;
    float4 clo = make_float4(INFINITY, INFINITY, INFINITY, 0.0f), chi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
    if (lane < cnt) { clo = boxes[2 * (size_t)(first + lane)]; chi = boxes[2 * (size_t)(first + lane) + 1]; }
    uint32_t keep = 0u;
    float lanes = INFINITY;   // child `lane`'s key from the lanes that keep it
    for (int j = 0; j < cnt; ++j) {
        const float4 lo = make_float4(lane_value(clo.x, j), lane_value(clo.y, j), lane_value(clo.z, j), 0.0f);
        const float4 hi = make_float4(lane_value(chi.x, j), lane_value(chi.y, j), lane_value(chi.z, j), 0.0f);
        float at;
        const bool mine = probe.reaches(lo, hi, at);
        if (__ballot(mine) == 0ull) continue;
        keep |= 1u << j;
        const float kj = probe.lanes_key(mine, at);
        if (lane == j) lanes = kj;
    }
    if (keep == 0u) return;
    const float key = probe.box_key(clo, chi, lanes);
    int rank = 0;   // kept children farther than this one (ties: the higher index counts as farther): a permutation of the kept
    for (int j = 0; j < cnt; ++j) {
        const float kj = lane_value(key, j);
        rank += ((keep >> j) & 1u) && (kj > key || (kj == key && j > lane)) ? 1 : 0;
    }
    if (lane < cnt && ((keep >> lane) & 1u)) (w.stack + top)[rank] = ((uint32_t)level << 29) | (first + lane);
    top += __popc(keep);
    wave_sync();
}

// The walk of gsr_knn.hip over triangles: depth first from the top on the wave-uniform stack in LDS.  A node's children are kept if
// some lane's probe reaches them (a ballot per child) and pushed nearest first; a popped leaf is tested again, the slots having
// tightened since the push, then staged into w.leaf with coalesced loads (3 KiB) between two wave_sync() and scanned by all lanes at
// once.
// Exactness.  A box is skipped -- here, in push_children and, for a record's own box, in slot_scan and hit_scan -- only when no member
// could enter any lane's slot, an equal value with a lower face index included: the rule is !(bound > slot), never >=, which would
// return the right values and, above a shared vertex or on a duplicated face, the wrong index.  That needs a member's value to be
// never below the bound of a box that contains the member's own box, however badly conditioned the member's test is.  Both contracts
// clamp the value into the bounds of the member's own box, and both bounds are monotone under rounding to nearest:
//   point  d(q, f) = fmin(fmax(d_tri, d_box), d_vtx) >= d_box = box_bound of the triangle's box: per axis the gap lo - q or q - hi,
//          squared, summed in one order.  A containing box has gaps that are not larger on any axis, so its bound never exceeds d_box.
//          (The same gives d_box <= d_vtx, a corner lying inside the triangle's box: d really is clamped into [d_box, d_vtx].)
//   ray    a face is hit only if its own box is (t_enter <= t_exit), and then t is clamped into [t_enter, t_exit] of that box: a
//          subtraction from a fixed o_k, a multiplication by a fixed 1 / d_k (then by a fixed pad), max and min.  A containing box
//          has a t_enter that is not larger and a t_exit that is not smaller (on an axis with d_k == 0 it contains o_k whenever the
//          triangle's box does), so it is hit too, no later.
// The slots start at (+inf, no face).  A finite query with a valid face always has an answer, at +inf if its distances overflow; a t
// of +inf is a miss, so +inf is the answer of exactly the rays that hit nothing.
template <class Probe>
__device__ __forceinline__ void walk_tree(const Wave& w, const unsigned char* __restrict__ plan, unsigned long long plan_bytes,
                                          Probe& probe) {
    // No plan, nothing walked: the header does not describe a plan of the plan_bytes the caller holds.  It is compared before anything
    // else of the plan is read (plan_bytes >= 256: checked by the host).  Here, not in open_wave: with the kernel's loads between the
    // check and the walk the compiler carries the tree as run-time values behind a flag (tri_query_kernel: 57 VGPRs for 56).
    const TriHeader h = *reinterpret_cast<const TriHeader*>(plan);
    if (h.magic != kPlanMagic || h.plan_bytes != plan_bytes || h.F == 0u || h.F >= (uint32_t)kMaxFaces) return;
    const TriTree tree = tri_layout(h.F);
    if (tree.bytes != plan_bytes) return;
    const float4* boxes = reinterpret_cast<const float4*>(plan + tree.boxes);
    const float4* records = reinterpret_cast<const float4*>(plan + tree.records);
    if (__ballot(probe.active()) == 0ull) return;
    probe.begin();
    int top = 0;
    uint32_t count, offset;
    tree_level(tree.leaves, tree.top, count, offset);
    push_children(w, boxes + 2 * (size_t)offset, tree.top, 0u, (int)min(count, (uint32_t)kFan), probe, top);
    while (top > 0) {
        const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)w.stack[--top]);
        const int level = (int)(e >> 29);
        const uint32_t node = e & ((1u << 29) - 1u);
        if (level > 0) {
            const uint32_t first = node * kFan;
            tree_level(tree.leaves, level - 1, count, offset);
            push_children(w, boxes + 2 * (size_t)offset, level - 1, first, (int)min((uint32_t)kFan, count - first), probe, top);
            continue;
        }
        const float4 lo = boxes[2 * (size_t)node], hi = boxes[2 * (size_t)node + 1];   // (leaves: level offset 0)
        float bound;
        if (__ballot(probe.reaches(lo, hi, bound)) == 0ull) continue;
        const uint32_t base = node * kLeaf;
        const int cnt = (int)min((uint32_t)kLeaf, h.F - base);
        wave_sync();
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int at = k * kLeaf + w.lane;
            if (at < 3 * cnt) w.leaf[at] = records[3 * (size_t)base + at];
        }
        wave_sync();
        probe.scan(w.leaf, cnt);
    }
}

// gsr_closest_tri_query: one lane per query point
__global__ __launch_bounds__(256) void tri_query_kernel(uint32_t n, const float* __restrict__ points, const unsigned char* __restrict__ plan,
                                                        unsigned long long plan_bytes, long long* __restrict__ face_idx,
                                                        float* __restrict__ sq_dist, float* __restrict__ closest) {
    Wave w;
    if (!open_wave(n, w)) return;
    const uint32_t s = w.s;
    Query q = {0.0f, 0.0f, 0.0f, false};
    if (s < n) {
        const float x = points[3 * (size_t)s], y = points[3 * (size_t)s + 1], z = points[3 * (size_t)s + 2];
        if (finite3(x, y, z)) q = {x, y, z, true};
    }
    PointProbe probe = {q, {INFINITY, kNoFace, {0.0f, 0.0f, 0.0f}}};
    walk_tree(w, plan, plan_bytes, probe);
    if (s >= n) return;
    const Slot& slot = probe.slot;
    const bool found = q.active && slot.face != kNoFace;
    face_idx[s] = found ? (long long)slot.face : -1ll;
    sq_dist[s] = found ? slot.d : INFINITY;
    if (closest) {
        closest[3 * (size_t)s] = found ? q.x + slot.p.x : 0.0f;
        closest[3 * (size_t)s + 1] = found ? q.y + slot.p.y : 0.0f;
        closest[3 * (size_t)s + 2] = found ? q.z + slot.p.z : 0.0f;
    }
}

// gsr_ray_first_hit: one lane per ray
__global__ __launch_bounds__(256) void ray_hit_kernel(uint32_t n, const float* __restrict__ origins, const float* __restrict__ dirs,
                                                      const unsigned char* __restrict__ plan, unsigned long long plan_bytes,
                                                      long long* __restrict__ face_idx, float* __restrict__ t_hit, float* __restrict__ bary) {
    Wave w;
    if (!open_wave(n, w)) return;
    const uint32_t s = w.s;
    RayProbe probe = {{}, {INFINITY, kNoFace, 0.0f, 0.0f, 0.0f}};
    if (s < n)
        probe.r = make_ray(origins[3 * (size_t)s], origins[3 * (size_t)s + 1], origins[3 * (size_t)s + 2], dirs[3 * (size_t)s],
                           dirs[3 * (size_t)s + 1], dirs[3 * (size_t)s + 2]);
    walk_tree(w, plan, plan_bytes, probe);
    if (s >= n) return;
    const HitSlot& slot = probe.slot;
    const bool found = probe.r.active && slot.face != kNoFace;
    face_idx[s] = found ? (long long)slot.face : -1ll;
    t_hit[s] = found ? slot.t : INFINITY;
    if (bary) {
        bary[3 * (size_t)s] = found ? slot.u : 0.0f;
        bary[3 * (size_t)s + 1] = found ? slot.v : 0.0f;
        bary[3 * (size_t)s + 2] = found ? slot.w : 0.0f;
    }
}

// bounds -> codes -> sort -> pack -> levels -> header.  scratch: tri_scratch(F).bytes; plan: tri_layout(F).bytes; F < 2^30
hipError_t launch_plan(int64_t V, const float* verts, uint32_t F, const long long* faces, unsigned char* plan, void* scratch,
                       hipStream_t stream) {
    const TriTree tree = tri_layout(F);
    if (F > 0) {
        uint32_t count, offset;
        tree_level(tree.leaves, tree.top, count, offset);
        if (count > (uint32_t)kFan) return hipErrorInvalidValue;   // (F < 2^30 never gets here)
        const TriScratch L = tri_scratch(F);
        char* base = static_cast<char*>(scratch);
        auto u32 = [&](size_t at) { return reinterpret_cast<uint32_t*>(base + at); };
        uint32_t *keys = u32(L.keys), *keys_alt = u32(L.keys_alt), *vals = u32(L.vals), *vals_alt = u32(L.vals_alt), *key_hi = u32(L.key_hi);
        float4* partials = reinterpret_cast<float4*>(base + L.partials);
        float4* records = reinterpret_cast<float4*>(plan + tree.records);
        float4* boxes = reinterpret_cast<float4*>(plan + tree.boxes);
        const uint32_t blocks = (F + 255u) / 256u;
        hipLaunchKernelGGL(tri_bounds_kernel, dim3(kBoundsBlocks), dim3(256), 0, stream, V, verts, F, faces, partials);
        hipLaunchKernelGGL(tri_codes_kernel, dim3(min(blocks, 2048u)), dim3(256), 0, stream, V, verts, F, faces, (const float4*)partials, keys,
                           key_hi);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        uint32_t* order = nullptr;
        e = morton_sort(u32(L.radix), F, keys, keys_alt, vals, vals_alt, key_hi, &order, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(tri_pack_kernel, dim3(blocks), dim3(256), 0, stream, V, verts, F, faces, (const uint32_t*)order, records, boxes);
        e = tree_levels(boxes, tree.leaves, tree.top, stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(tri_header_kernel, dim3(1), dim3(64), 0, stream, reinterpret_cast<TriHeader*>(plan), F, (unsigned long long)tree.bytes);
    return hipGetLastError();
}

bool misaligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1u)) != 0u; }

// The argument checks of the two query entry points, in the order their refusals come: n, then the entry point's own pointers (`null`,
// `unaligned`: what it found of them; `alignments`: the text of that refusal), then plan_bytes -- every plan is a whole number of
// 256-byte blocks, the header first; the header itself is compared with plan_bytes on the device.  `what`: "queries" or "rays".
// GSR_OK with *grid == 0: n == 0, nothing to do.  Otherwise *grid workgroups of four waves of 64.
int check_query(const char* name, const char* what, int64_t n, bool null, bool unaligned, const char* alignments, size_t plan_bytes,
                uint32_t* grid) {
    *grid = 0u;
    if (n < 0) return fail(GSR_ERR_INVALID_ARG, "%s: negative count (n %lld)", name, (long long)n);
    if (n >= kMaxQueries) return fail(GSR_ERR_INVALID_ARG, "%s: %lld %s (at most 2^31 - 1)", name, (long long)n, what);
    if (n == 0) return GSR_OK;
    if (null) return fail(GSR_ERR_INVALID_ARG, "%s: null pointer", name);
    if (unaligned) return fail(GSR_ERR_INVALID_ARG, "%s: misaligned pointer (%s)", name, alignments);
    if (plan_bytes < kAlign || (plan_bytes & (kAlign - 1)) != 0)
        return fail(GSR_ERR_INVALID_ARG, "%s: plan_bytes = %zu is not the size of a plan", name, plan_bytes);
    const uint32_t groups = (uint32_t)((n + kLeaf - 1) / kLeaf);
    *grid = (groups + 3u) / 4u;
    return GSR_OK;
}

}  // namespace
}  // namespace gsr

using gsr::fail;

extern "C" {

size_t gsr_closest_tri_plan_bytes(int64_t F) {
    return (F < 0 || F >= gsr::kMaxFaces) ? 0 : gsr::tri_layout((uint32_t)F).bytes;
}

size_t gsr_closest_tri_plan_scratch_bytes(int64_t F) {
    return (F < 0 || F >= gsr::kMaxFaces) ? 0 : gsr::tri_scratch((uint32_t)F).bytes;
}

int gsr_closest_tri_plan(int64_t V, const float* verts, int64_t F, const int64_t* faces, void* plan, size_t plan_bytes, void* scratch,
                         size_t scratch_bytes, void* stream_) {
    if (V < 0 || F < 0) return fail(GSR_ERR_INVALID_ARG, "gsr_closest_tri_plan: negative count (V %lld, F %lld)", (long long)V, (long long)F);
    if (F >= gsr::kMaxFaces) return fail(GSR_ERR_INVALID_ARG, "gsr_closest_tri_plan: %lld faces (at most 2^30 - 1)", (long long)F);
    if (V >= gsr::kMaxVerts) return fail(GSR_ERR_INVALID_ARG, "gsr_closest_tri_plan: %lld vertices (at most 2^31 - 1)", (long long)V);
    const size_t need_plan = gsr_closest_tri_plan_bytes(F), need_scratch = gsr_closest_tri_plan_scratch_bytes(F);
    if ((!verts && V > 0 && F > 0) || (!faces && F > 0) || !plan || (!scratch && need_scratch > 0))
        return fail(GSR_ERR_INVALID_ARG, "gsr_closest_tri_plan: null pointer");
    if (gsr::misaligned(verts, 4) || gsr::misaligned(faces, 8) || gsr::misaligned(plan, 256) || gsr::misaligned(scratch, 256))
        return fail(GSR_ERR_INVALID_ARG, "gsr_closest_tri_plan: misaligned pointer (verts: 4 bytes, faces: 8 bytes, plan / scratch: 256 bytes)");
    if (plan_bytes < need_plan) return fail(GSR_ERR_INVALID_ARG, "gsr_closest_tri_plan: plan too small (%zu of %zu bytes)", plan_bytes, need_plan);
    if (scratch_bytes < need_scratch)
        return fail(GSR_ERR_INVALID_ARG, "gsr_closest_tri_plan: scratch too small (%zu of %zu bytes)", scratch_bytes, need_scratch);
    GSR_HIP(gsr::launch_plan(V, verts, (uint32_t)F, reinterpret_cast<const long long*>(faces), static_cast<unsigned char*>(plan), scratch,
                             (hipStream_t)stream_));
    return GSR_OK;
}

int gsr_closest_tri_query(int64_t n, const float* points, const void* plan, size_t plan_bytes, int64_t* face_idx, float* sq_dist,
                          float* closest, void* stream_) {
    uint32_t grid;
    const int status = gsr::check_query("gsr_closest_tri_query", "queries", n, !points || !plan || !face_idx || !sq_dist,
                                        gsr::misaligned(points, 4) || gsr::misaligned(plan, 256) || gsr::misaligned(face_idx, 8) ||
                                            gsr::misaligned(sq_dist, 4) || gsr::misaligned(closest, 4),
                                        "points / sq_dist / closest: 4 bytes, face_idx: 8 bytes, plan: 256 bytes", plan_bytes, &grid);
    if (status != GSR_OK || grid == 0u) return status;
    hipLaunchKernelGGL(gsr::tri_query_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream_, (uint32_t)n, points,
                       static_cast<const unsigned char*>(plan), (unsigned long long)plan_bytes, reinterpret_cast<long long*>(face_idx), sq_dist,
                       closest);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_ray_first_hit(int64_t n, const float* origins, const float* dirs, const void* plan, size_t plan_bytes, int64_t* face_idx, float* t,
                      float* bary, void* stream_) {
    uint32_t grid;
    const int status = gsr::check_query("gsr_ray_first_hit", "rays", n, !origins || !dirs || !plan || !face_idx || !t,
                                        gsr::misaligned(origins, 4) || gsr::misaligned(dirs, 4) || gsr::misaligned(plan, 256) ||
                                            gsr::misaligned(face_idx, 8) || gsr::misaligned(t, 4) || gsr::misaligned(bary, 4),
                                        "origins / dirs / t / bary: 4 bytes, face_idx: 8 bytes, plan: 256 bytes", plan_bytes, &grid);
    if (status != GSR_OK || grid == 0u) return status;
    hipLaunchKernelGGL(gsr::ray_hit_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream_, (uint32_t)n, origins, dirs,
                       static_cast<const unsigned char*>(plan), (unsigned long long)plan_bytes, reinterpret_cast<long long*>(face_idx), t,
                       bary);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

}  // extern "C"
