// gsr_bound.hip -- the Gaussians SuGaR binds to a surface mesh: SuGaR.points, SuGaR.scaling and SuGaR.quaternions with
// binded_to_surface_mesh set (sugar_model.py:376-391, :408-423, :425-452), and their backward into the vertices, _quaternions and _scales
// (include/gsr.h: gsr_bound_gaussians, gsr_bound_gaussians_backward; the contract is the module docstring of autovfx_amd/bound.py and
// DESIGN.md 7o).  Two kernels, no scratch, no host read:
//   forward    one lane per face: three int64 indices, a dependent gather of nine floats, the face's frame (R_0, base_R_1, base_R_2) once,
//              then a loop over the face's G Gaussians: 16 bytes read and 12 + 12 + 16 written per Gaussian; an output that is not
//              wanted is neither computed nor stored
//   backward   one lane per face: the forward again (nothing of size [N, .] is kept between the two), grad_complex and grad_log_scales
//              with plain stores, the face's three vertex gradients summed in registers over its Gaussians and over the three outputs,
//              then nine float atomic adds into grad_verts (zeroed on the stream first), as gsr_face_areas_normals_backward does
// fp32 throughout, -ffp-contract=off, IEEE division and sqrt: the numpy restatement computes the same bits; expf is the one operation
// whose bits may differ from the host's, and only the order in which the atomics arrive is free.
#include "gsr_internal.h"

#include <math.h>

namespace gsr {
namespace {

constexpr int kBoundThreads = 256;
constexpr int kBoundMaxG = 8;
constexpr float kFaceEps = 1e-6f;        // the clamp of the face normal (7j)
constexpr float kUnitEps = 1e-12f;       // the clamp of F.normalize
constexpr float kQuatFloor = 0.1f;       // matrix_to_quaternion's floor on the divisor

// ---- the contract's arithmetic: restated operation by operation in autovfx_amd/bound.py ------------------------------------------------
// (Arrays and the unit's own gather, not gsr_vec3.h's Vec3: with it the forward measured slower than this text)

__device__ inline float norm3(const float (&v)[3]) { return sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }
__device__ inline float dot3(const float (&a)[3], const float (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ inline void cross3(const float (&a)[3], const float (&b)[3], float (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// y = x / fmaxf(m, eps) with m = |x|: x's gradient from y's, by the branch autograd takes (m >= eps: through the norm as well)
template <int N>
__device__ inline void unit_backward(const float (&x)[N], float m, const float (&g)[N], float (&gx)[N]) {
    const float D = fmaxf(m, kUnitEps);
#pragma unroll
    for (int i = 0; i < N; ++i) gx[i] = g[i] / D;
    if (m >= kUnitEps) {
        float s = g[0] * x[0];
#pragma unroll
        for (int i = 1; i < N; ++i) s = s + g[i] * x[i];
        const float w = (-(s / (D * D))) / m;
#pragma unroll
        for (int i = 0; i < N; ++i) gx[i] = gx[i] + x[i] * w;
    }
}

// What a face gives all its Gaussians.
struct Frame {
    long long i0, i1, i2;
    float v0[3], v1[3], v2[3];
    float a[3], b[3], c[3], n;           // a = v1 - v0, b = v2 - v0, c = a x b, n = |c|                              (7j)
    float normal[3], m0, r0[3];          // normal = c / max(n, 1e-6), m0 = |normal|, R_0 = normal / max(m0, 1e-12)
    float e[3], me, b1[3];               // e = v0 - v1, base_R_1 = e / max(|e|, 1e-12)
    float x[3], mx, b2[3];               // x = R_0 x base_R_1, base_R_2 = x / max(|x|, 1e-12)
};

// false: an index outside [0, V), nothing read from verts
__device__ inline bool face_vertices(const float* __restrict__ verts, const long long* __restrict__ faces, long long V, size_t f, Frame& t) {
    t.i0 = faces[3 * f + 0], t.i1 = faces[3 * f + 1], t.i2 = faces[3 * f + 2];
    if (t.i0 < 0 || t.i0 >= V || t.i1 < 0 || t.i1 >= V || t.i2 < 0 || t.i2 >= V) return false;
    const float* p0 = verts + 3 * (size_t)t.i0;
    const float* p1 = verts + 3 * (size_t)t.i1;
    const float* p2 = verts + 3 * (size_t)t.i2;
#pragma unroll
    for (int i = 0; i < 3; ++i) t.v0[i] = p0[i], t.v1[i] = p1[i], t.v2[i] = p2[i];
    return true;
}

__device__ inline void face_frame(Frame& t) {
#pragma unroll
    for (int i = 0; i < 3; ++i) t.a[i] = t.v1[i] - t.v0[i], t.b[i] = t.v2[i] - t.v0[i];
    cross3(t.a, t.b, t.c);
    t.n = norm3(t.c);
    const float dn = fmaxf(t.n, kFaceEps);
#pragma unroll
    for (int i = 0; i < 3; ++i) t.normal[i] = t.c[i] / dn;
    t.m0 = norm3(t.normal);
    const float d0 = fmaxf(t.m0, kUnitEps);
#pragma unroll
    for (int i = 0; i < 3; ++i) t.r0[i] = t.normal[i] / d0, t.e[i] = t.v0[i] - t.v1[i];
    t.me = norm3(t.e);
    const float de = fmaxf(t.me, kUnitEps);
#pragma unroll
    for (int i = 0; i < 3; ++i) t.b1[i] = t.e[i] / de;
    cross3(t.r0, t.b1, t.x);
    t.mx = norm3(t.x);
    const float dx = fmaxf(t.mx, kUnitEps);
#pragma unroll
    for (int i = 0; i < 3; ++i) t.b2[i] = t.x[i] / dx;
}

// One Gaussian's rotation: the learned 2-D rotation of the frame, then matrix_to_quaternion (pytorch3d 0.7.4) and the last normalize.
struct Rotation {
    float p, q, mz, zr, zi;              // complex, |complex|, z = complex / max(|complex|, 1e-12)
    float r1[3], r2[3];                  // R_1 = zr base_R_1 + zi base_R_2, R_2 = (-zi) base_R_1 + zr base_R_2
    int k;                               // the candidate taken: the first of the largest q_abs
    float pre, qk, d;                    // its 1 +- m00 +- m11 +- m22, its q_abs, d = 2 max(q_abs, 0.1)
    float u[4];                          // the candidate row over d, as matrix_to_quaternion returns it (before `standardize`)
    bool flipped;                        // standardize: the row was negated
    float mq, out[4];                    // |row|, row / max(|row|, 1e-12)
};

__device__ inline void rotation_of(const Frame& t, float p, float q, int standardize, Rotation& r) {
    r.p = p, r.q = q;
    r.mz = sqrtf(p * p + q * q);
    const float dz = fmaxf(r.mz, kUnitEps);
    r.zr = p / dz, r.zi = q / dz;
    const float nzi = -r.zi;
#pragma unroll
    for (int i = 0; i < 3; ++i) r.r1[i] = r.zr * t.b1[i] + r.zi * t.b2[i], r.r2[i] = nzi * t.b1[i] + r.zr * t.b2[i];
    // R = [R_0 | R_1 | R_2]: m_ij is component i of column j
    const float m00 = t.r0[0], m10 = t.r0[1], m20 = t.r0[2];
    const float m01 = r.r1[0], m11 = r.r1[1], m21 = r.r1[2];
    const float m02 = r.r2[0], m12 = r.r2[1], m22 = r.r2[2];
    float pre[4];
    pre[0] = ((1.0f + m00) + m11) + m22;
    pre[1] = ((1.0f + m00) - m11) - m22;
    pre[2] = ((1.0f - m00) + m11) - m22;
    pre[3] = ((1.0f - m00) - m11) + m22;
    float best = pre[0] > 0.0f ? sqrtf(pre[0]) : 0.0f;
    r.k = 0, r.pre = pre[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        const float qa = pre[j] > 0.0f ? sqrtf(pre[j]) : 0.0f;
        if (qa > best) best = qa, r.k = j, r.pre = pre[j];
    }
    r.qk = best;
    const float sq = best * best;
    float c0, c1, c2, c3;
    switch (r.k) {
        case 0: c0 = sq, c1 = m21 - m12, c2 = m02 - m20, c3 = m10 - m01; break;
        case 1: c0 = m21 - m12, c1 = sq, c2 = m10 + m01, c3 = m02 + m20; break;
        case 2: c0 = m02 - m20, c1 = m10 + m01, c2 = sq, c3 = m12 + m21; break;
        default: c0 = m10 - m01, c1 = m20 + m02, c2 = m21 + m12, c3 = sq; break;
    }
    r.d = 2.0f * fmaxf(best, kQuatFloor);
    r.u[0] = c0 / r.d, r.u[1] = c1 / r.d, r.u[2] = c2 / r.d, r.u[3] = c3 / r.d;
    r.flipped = standardize != 0 && r.u[0] < 0.0f;
    float s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = r.flipped ? -r.u[i] : r.u[i];
    r.mq = sqrtf(((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]) + s[3] * s[3]);
    const float dq = fmaxf(r.mq, kUnitEps);
#pragma unroll
    for (int i = 0; i < 4; ++i) r.out[i] = s[i] / dq;
}

// The gradients of R's columns (g0 for R_0, g1 for R_1, g2 for R_2) from that of the quaternion: the last normalize, the flip, the division
// by d, the candidate's own q_abs (through its square, through d when it is above the floor, through the square root when pre > 0), and
// the sums and differences of the row.  The candidates not taken get nothing.
__device__ inline void rotation_backward(const Rotation& r, const float (&g)[4], float (&g0)[3], float (&g1)[3], float (&g2)[3]) {
    float s[4], gs[4], gu[4], gc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = r.flipped ? -r.u[i] : r.u[i];
    unit_backward<4>(s, r.mq, g, gs);
#pragma unroll
    for (int i = 0; i < 4; ++i) gu[i] = r.flipped ? -gs[i] : gs[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) gc[i] = gu[i] / r.d;
    const float sd = ((gu[0] * r.u[0] + gu[1] * r.u[1]) + gu[2] * r.u[2]) + gu[3] * r.u[3];
    const float gd = -(sd / r.d);
    const float gdiag = r.k == 0 ? gc[0] : r.k == 1 ? gc[1] : r.k == 2 ? gc[2] : gc[3];
    float gq = (2.0f * r.qk) * gdiag;
    if (r.qk > kQuatFloor) gq = gq + 2.0f * gd;
    const float gpre = r.pre > 0.0f ? gq / (2.0f * r.qk) : 0.0f;
    // the row's entry of each off-diagonal pair and whether it is the pair's difference (first - second) or its sum
    float gA, gB, gC;                    // pairs (m21, m12), (m02, m20), (m10, m01)
    bool dA, dB, dC;
    float s00, s11, s22;                 // the signs of m00, m11, m22 in the candidate's pre
    switch (r.k) {
        case 0: gA = gc[1], dA = true, gB = gc[2], dB = true, gC = gc[3], dC = true, s00 = 1.0f, s11 = 1.0f, s22 = 1.0f; break;
        case 1: gA = gc[0], dA = true, gB = gc[3], dB = false, gC = gc[2], dC = false, s00 = 1.0f, s11 = -1.0f, s22 = -1.0f; break;
        case 2: gA = gc[3], dA = false, gB = gc[0], dB = true, gC = gc[1], dC = false, s00 = -1.0f, s11 = 1.0f, s22 = -1.0f; break;
        default: gA = gc[2], dA = false, gB = gc[1], dB = false, gC = gc[0], dC = true, s00 = -1.0f, s11 = -1.0f, s22 = 1.0f; break;
    }
    const float gm21 = gA, gm12 = dA ? -gA : gA;
    const float gm02 = gB, gm20 = dB ? -gB : gB;
    const float gm10 = gC, gm01 = dC ? -gC : gC;
    g0[0] = s00 * gpre, g0[1] = gm10, g0[2] = gm20;
    g1[0] = gm01, g1[1] = s11 * gpre, g1[2] = gm21;
    g2[0] = gm02, g2[1] = gm12, g2[2] = s22 * gpre;
}

__global__ void __launch_bounds__(kBoundThreads) bound_gaussians_kernel(long long V, long long F, int G, const float* __restrict__ verts,
                                                                        const long long* __restrict__ faces, const float* __restrict__ bary,
                                                                        const float* __restrict__ complex_, const float* __restrict__ log_scales,
                                                                        const float* __restrict__ thickness, int standardize,
                                                                        float* __restrict__ points, float* __restrict__ scaling,
                                                                        float* __restrict__ quaternions) {
    const long long f = (long long)blockIdx.x * kBoundThreads + threadIdx.x;
    if (f >= F) return;
    const size_t first = (size_t)f * (size_t)G;
    if (scaling) {                       // (does not depend on the face)
        const float th = thickness[0];
        for (int g = 0; g < G; ++g) {
            const size_t i = first + g;
            float* s = scaling + 3 * i;
            s[0] = th, s[1] = expf(log_scales[2 * i + 0]), s[2] = expf(log_scales[2 * i + 1]);
        }
    }
    if (!points && !quaternions) return;
    Frame t;
    const bool valid = face_vertices(verts, faces, V, (size_t)f, t);
    if (valid && quaternions) face_frame(t);
    for (int g = 0; g < G; ++g) {
        const size_t i = first + g;
        if (points) {
            float* o = points + 3 * i;
            if (valid) {
                const float w0 = bary[3 * g + 0], w1 = bary[3 * g + 1], w2 = bary[3 * g + 2];
#pragma unroll
                for (int j = 0; j < 3; ++j) o[j] = (t.v0[j] * w0 + t.v1[j] * w1) + t.v2[j] * w2;
            } else {
                o[0] = 0.0f, o[1] = 0.0f, o[2] = 0.0f;
            }
        }
        if (quaternions) {
            float* o = quaternions + 4 * i;
            if (valid) {
                Rotation r;
                rotation_of(t, complex_[2 * i + 0], complex_[2 * i + 1], standardize, r);
                o[0] = r.out[0], o[1] = r.out[1], o[2] = r.out[2], o[3] = r.out[3];
            } else {
                o[0] = 0.0f, o[1] = 0.0f, o[2] = 0.0f, o[3] = 0.0f;
            }
        }
    }
}

__global__ void __launch_bounds__(kBoundThreads) bound_gaussians_backward_kernel(
    long long V, long long F, int G, const float* __restrict__ verts, const long long* __restrict__ faces, const float* __restrict__ bary,
    const float* __restrict__ complex_, const float* __restrict__ log_scales, int standardize, const float* __restrict__ grad_points,
    const float* __restrict__ grad_scaling, const float* __restrict__ grad_quaternions, float* __restrict__ grad_verts,
    float* __restrict__ grad_complex, float* __restrict__ grad_log_scales) {
    const long long f = (long long)blockIdx.x * kBoundThreads + threadIdx.x;
    if (f >= F) return;
    const size_t first = (size_t)f * (size_t)G;
    for (int g = 0; g < G; ++g) {        // scaling = (thickness, exp(s0), exp(s1)): nothing of the face in it
        const size_t i = first + g;
        float l0 = 0.0f, l1 = 0.0f;
        if (grad_scaling) l0 = grad_scaling[3 * i + 1] * expf(log_scales[2 * i + 0]), l1 = grad_scaling[3 * i + 2] * expf(log_scales[2 * i + 1]);
        grad_log_scales[2 * i + 0] = l0, grad_log_scales[2 * i + 1] = l1;
    }
    Frame t;
    const bool valid = face_vertices(verts, faces, V, (size_t)f, t);
    if (!valid || !grad_quaternions) {
        for (int g = 0; g < G; ++g) grad_complex[2 * (first + g) + 0] = 0.0f, grad_complex[2 * (first + g) + 1] = 0.0f;
    }
    if (!valid || (!grad_points && !grad_quaternions)) return;
    float t0[3] = {0.0f, 0.0f, 0.0f}, t1[3] = {0.0f, 0.0f, 0.0f}, t2[3] = {0.0f, 0.0f, 0.0f};   // what the face adds to v0, v1, v2
    if (grad_points) {
        for (int g = 0; g < G; ++g) {
            const float* gp = grad_points + 3 * (first + g);
            const float w0 = bary[3 * g + 0], w1 = bary[3 * g + 1], w2 = bary[3 * g + 2];
#pragma unroll
            for (int j = 0; j < 3; ++j) t0[j] = t0[j] + w0 * gp[j], t1[j] = t1[j] + w1 * gp[j], t2[j] = t2[j] + w2 * gp[j];
        }
    }
    if (grad_quaternions) {
        face_frame(t);
        float G0[3] = {0.0f, 0.0f, 0.0f}, G1[3] = {0.0f, 0.0f, 0.0f}, G2[3] = {0.0f, 0.0f, 0.0f};   // of R_0, base_R_1, base_R_2, over the Gaussians
        for (int g = 0; g < G; ++g) {
            const size_t i = first + g;
            Rotation r;
            rotation_of(t, complex_[2 * i + 0], complex_[2 * i + 1], standardize, r);
            const float gq[4] = {grad_quaternions[4 * i + 0], grad_quaternions[4 * i + 1], grad_quaternions[4 * i + 2], grad_quaternions[4 * i + 3]};
            float g0[3], g1[3], g2[3];
            rotation_backward(r, gq, g0, g1, g2);
            const float gz[2] = {dot3(g1, t.b1) + dot3(g2, t.b2), dot3(g1, t.b2) - dot3(g2, t.b1)};
            const float z[2] = {r.p, r.q};
            float gcx[2];
            unit_backward<2>(z, r.mz, gz, gcx);
            grad_complex[2 * i + 0] = gcx[0], grad_complex[2 * i + 1] = gcx[1];
            const float nzi = -r.zi;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                G0[j] = G0[j] + g0[j];
                G1[j] = G1[j] + (r.zr * g1[j] + nzi * g2[j]);
                G2[j] = G2[j] + (r.zi * g1[j] + r.zr * g2[j]);
            }
        }
        // base_R_2 = x / max(|x|, 1e-12), x = R_0 x base_R_1
        float gx[3], gr0[3], gb1[3], ge[3], gn[3], gc[3], ga[3], gb[3];
        unit_backward<3>(t.x, t.mx, G2, gx);
        cross3(t.b1, gx, gr0);
        cross3(gx, t.r0, gb1);
#pragma unroll
        for (int j = 0; j < 3; ++j) G0[j] = G0[j] + gr0[j], G1[j] = G1[j] + gb1[j];
        unit_backward<3>(t.e, t.me, G1, ge);             // base_R_1 = e / max(|e|, 1e-12), e = v0 - v1
        unit_backward<3>(t.normal, t.m0, G0, gn);        // R_0 = normal / max(|normal|, 1e-12)
        if (t.n >= kFaceEps) {                           // normal = c / max(n, 1e-6): 7j's backward without the area
            const float m[3] = {t.c[0] / t.n, t.c[1] / t.n, t.c[2] / t.n};
            const float dot = dot3(m, gn);
#pragma unroll
            for (int j = 0; j < 3; ++j) gc[j] = (gn[j] - m[j] * dot) / t.n;
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) gc[j] = gn[j] / kFaceEps;
        }
        cross3(t.b, gc, ga);                             // g_a = b x g_c
        cross3(gc, t.a, gb);                             // g_b = g_c x a
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            t0[j] = (t0[j] + ge[j]) + (-(ga[j] + gb[j]));
            t1[j] = (t1[j] + (-ge[j])) + ga[j];
            t2[j] = t2[j] + gb[j];
        }
    }
    float* d0 = grad_verts + 3 * (size_t)t.i0;
    float* d1 = grad_verts + 3 * (size_t)t.i1;
    float* d2 = grad_verts + 3 * (size_t)t.i2;
    atomicAdd(d0 + 0, t0[0]), atomicAdd(d0 + 1, t0[1]), atomicAdd(d0 + 2, t0[2]);
    atomicAdd(d1 + 0, t1[0]), atomicAdd(d1 + 1, t1[1]), atomicAdd(d1 + 2, t1[2]);
    atomicAdd(d2 + 0, t2[0]), atomicAdd(d2 + 1, t2[1]), atomicAdd(d2 + 2, t2[2]);
}

const char* bad_bound_sizes(int64_t V, int64_t F, int G) {
    if (V < 0 || F < 0) return "negative count";
    if (G < 1 || G > kBoundMaxG) return "G outside 1..8";
    if (V >= ((int64_t)1 << 31) || F * (int64_t)G >= ((int64_t)1 << 31)) return "2^31 or more vertices or Gaussians";
    return nullptr;
}

}  // namespace
}  // namespace gsr

using gsr::fail;

extern "C" {

int gsr_bound_gaussians(int64_t V, int64_t F, int G, const float* verts, const int64_t* faces, const float* bary, const float* complex_,
                        const float* log_scales, const float* thickness, int standardize, float* points, float* scaling,
                        float* quaternions, void* stream_) {
    if (const char* why = gsr::bad_bound_sizes(V, F, G)) return fail(GSR_ERR_INVALID_ARG, "gsr_bound_gaussians: %s", why);
    if (F == 0) return GSR_OK;
    const bool geometry = points || quaternions;
    if ((geometry && (!faces || (V > 0 && !verts))) || (points && !bary) || (quaternions && !complex_) || (scaling && (!log_scales || !thickness)))
        return fail(GSR_ERR_INVALID_ARG, "gsr_bound_gaussians: null pointer (an input of a wanted output)");
    if (!gsr::aligned4(verts) || !gsr::aligned8(faces) || !gsr::aligned4(bary) || !gsr::aligned4(complex_) || !gsr::aligned4(log_scales) ||
        !gsr::aligned4(thickness) || !gsr::aligned4(points) || !gsr::aligned4(scaling) || !gsr::aligned4(quaternions))
        return fail(GSR_ERR_INVALID_ARG, "gsr_bound_gaussians: misaligned pointer (floats: 4 bytes, faces: 8)");
    if (!points && !scaling && !quaternions) return GSR_OK;
    hipLaunchKernelGGL(gsr::bound_gaussians_kernel, dim3(gsr::blocks_of(F, gsr::kBoundThreads)), dim3(gsr::kBoundThreads), 0, (hipStream_t)stream_,
                       (long long)V, (long long)F, G, verts, reinterpret_cast<const long long*>(faces), bary, complex_, log_scales, thickness,
                       standardize, points, scaling, quaternions);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_bound_gaussians_backward(int64_t V, int64_t F, int G, const float* verts, const int64_t* faces, const float* bary,
                                 const float* complex_, const float* log_scales, int standardize, const float* grad_points,
                                 const float* grad_scaling, const float* grad_quaternions, float* grad_verts, float* grad_complex,
                                 float* grad_log_scales, void* stream_) {
    if (const char* why = gsr::bad_bound_sizes(V, F, G)) return fail(GSR_ERR_INVALID_ARG, "gsr_bound_gaussians_backward: %s", why);
    if ((V > 0 && (!verts || !grad_verts)) || (F > 0 && (!faces || !grad_complex || !grad_log_scales)) || (F > 0 && grad_points && !bary) ||
        (F > 0 && grad_quaternions && !complex_) || (F > 0 && grad_scaling && !log_scales))
        return fail(GSR_ERR_INVALID_ARG, "gsr_bound_gaussians_backward: null pointer");
    if (!gsr::aligned4(verts) || !gsr::aligned8(faces) || !gsr::aligned4(bary) || !gsr::aligned4(complex_) || !gsr::aligned4(log_scales) ||
        !gsr::aligned4(grad_points) || !gsr::aligned4(grad_scaling) || !gsr::aligned4(grad_quaternions) || !gsr::aligned4(grad_verts) ||
        !gsr::aligned4(grad_complex) || !gsr::aligned4(grad_log_scales))
        return fail(GSR_ERR_INVALID_ARG, "gsr_bound_gaussians_backward: misaligned pointer (floats: 4 bytes, faces: 8)");
    hipStream_t stream = (hipStream_t)stream_;
    if (V > 0) GSR_HIP(hipMemsetAsync(grad_verts, 0, (size_t)V * 3u * sizeof(float), stream));
    if (F == 0) return GSR_OK;
    hipLaunchKernelGGL(gsr::bound_gaussians_backward_kernel, dim3(gsr::blocks_of(F, gsr::kBoundThreads)), dim3(gsr::kBoundThreads), 0, stream,
                       (long long)V, (long long)F, G, verts, reinterpret_cast<const long long*>(faces), bary, complex_, log_scales, standardize,
                       grad_points, grad_scaling, grad_quaternions, grad_verts, grad_complex, grad_log_scales);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

}  // extern "C"
