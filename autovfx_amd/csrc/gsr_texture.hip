// gsr_texture.hip -- the texture bake of SuGaR's refined mesh (sugar_model.py:2398-2614, extract_texture_image_and_uv_from_gaussians):
// which texel of the UV atlas a rasterized pixel sees, one camera's colours into the atlas, and the atlas's initial fill (include/gsr.h:
// gsr_texture_texels, gsr_texture_bake_view, gsr_texture_fill; the contract is the module docstring of autovfx_amd/texture.py and
// DESIGN.md 7n).  Five kernels, no scratch, no host read, no float atomics:
//   texels       one lane per pixel: the texel index, or -1
//   claim        one lane per pixel: atomicMin(owner[texel], pixel index) -- the lowest pixel of a camera on a texel wins it
//   accumulate   one lane per pixel: the pixel that finds its own index in owner[texel] adds its colour (or replaces the fill on the
//                texel's first visit), counts, and puts 0xFFFFFFFF back; a loser reads the winner's index or 0xFFFFFFFF, never its own
//   constant     the atlas to 0.5 (what SH2RGB makes of the reference's zeros)
//   fill         one lane per (face, texel of the face): the texel's point on the face, q of each of the face's G Gaussians (the
//                density field's q, gsr_field.hip), the colour of the first Gaussian with the smallest q
// fp32 throughout, -ffp-contract=off, IEEE division, rintf to nearest even: the numpy restatements compute the same bits.
#include "gsr_internal.h"
#include "gsr_vec3.h"

#include <math.h>

namespace gsr {
namespace {

constexpr int kTexThreads = 256;
constexpr uint32_t kNoOwner = 0xFFFFFFFFu;
constexpr int kTexMaxG = 8;
constexpr int kTexMinS = 4, kTexMaxS = 32;
constexpr int kTexMaxT = 46340;                  // T * T < 2^31
constexpr float kShC0 = 0.28209479177387814f;    // SH2RGB: sh * C0 + 0.5

// ---- the contract's arithmetic: restated operation by operation in autovfx_amd/texture.py ---------------------------------------------

// The texel (row * T + col) pixel p sees, or -1: a face outside [0, F), a depth that is not > 0, a NaN coordinate.
__device__ inline int texel_of_pixel(long long F, int T, const long long* __restrict__ pix_to_face, const float* __restrict__ bary,
                                     const float* __restrict__ zbuf, const float* __restrict__ face_uvs, size_t p) {
    const long long f = pix_to_face[p];
    if (f < 0 || f >= F) return -1;
    if (!(zbuf[p] > 0.0f)) return -1;
    const float b0 = bary[3 * p + 0], b1 = bary[3 * p + 1], b2 = bary[3 * p + 2];
    const float* uv = face_uvs + 6 * (size_t)f;
    const float last = (float)(T - 1);
    int ic[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float uvc = (b0 * uv[c] + b1 * uv[2 + c]) + b2 * uv[4 + c];
        const float g = uvc * 2.0f - 1.0f;
        const float x = ((g + 1.0f) / 2.0f) * last;
        if (x != x) return -1;
        ic[c] = (int)rintf(fminf(last, fmaxf(x, 0.0f)));
    }
    return (T - 1 - ic[1]) * T + ic[0];
}

__global__ void __launch_bounds__(kTexThreads) texture_texels_kernel(long long P, long long F, int T, const long long* __restrict__ pix_to_face,
                                                                     const float* __restrict__ bary, const float* __restrict__ zbuf,
                                                                     const float* __restrict__ face_uvs, int* __restrict__ texel) {
    const long long p = (long long)blockIdx.x * kTexThreads + threadIdx.x;
    if (p >= P) return;
    texel[p] = texel_of_pixel(F, T, pix_to_face, bary, zbuf, face_uvs, (size_t)p);
}

__global__ void __launch_bounds__(kTexThreads) texture_claim_kernel(long long P, long long F, int T, const long long* __restrict__ pix_to_face,
                                                                    const float* __restrict__ bary, const float* __restrict__ zbuf,
                                                                    const float* __restrict__ face_uvs, uint32_t* owner) {
    const long long p = (long long)blockIdx.x * kTexThreads + threadIdx.x;
    if (p >= P) return;
    const int t = texel_of_pixel(F, T, pix_to_face, bary, zbuf, face_uvs, (size_t)p);
    if (t >= 0) atomicMin(owner + t, (uint32_t)p);
}

__global__ void __launch_bounds__(kTexThreads) texture_accumulate_kernel(long long P, long long F, int T, const long long* __restrict__ pix_to_face,
                                                                         const float* __restrict__ bary, const float* __restrict__ zbuf,
                                                                         const float* __restrict__ face_uvs, const float* __restrict__ rgb,
                                                                         long long rgb_stride, float* __restrict__ tex,
                                                                         float* __restrict__ count, uint32_t* owner) {
    const long long p = (long long)blockIdx.x * kTexThreads + threadIdx.x;
    if (p >= P) return;
    const int t = texel_of_pixel(F, T, pix_to_face, bary, zbuf, face_uvs, (size_t)p);
    if (t < 0 || owner[t] != (uint32_t)p) return;
    const float* c = rgb + (size_t)p * (size_t)rgb_stride;
    float* d = tex + 3 * (size_t)t;
    const float n = count[t];
    if (n == 0.0f) {
        d[0] = c[0], d[1] = c[1], d[2] = c[2];
    } else {
        d[0] = d[0] + c[0], d[1] = d[1] + c[1], d[2] = d[2] + c[2];
    }
    count[t] = n + 1.0f;
    owner[t] = kNoOwner;
}

__global__ void __launch_bounds__(kTexThreads) texture_constant_kernel(float* __restrict__ tex, size_t n, float value) {
    for (size_t i = (size_t)blockIdx.x * kTexThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kTexThreads) tex[i] = value;
}

// Work item l of the whole call is texel l % n of face l / n; a workgroup's 256 items start at face f0, so the per-lane division is a
// 32-bit one whatever F is.
__global__ void __launch_bounds__(kTexThreads) texture_fill_kernel(long long V, long long F, int G, int A, int S, uint32_t n,
                                                                   const float* __restrict__ verts, const long long* __restrict__ faces,
                                                                   const float* __restrict__ centers, const float* __restrict__ M,
                                                                   const float* __restrict__ features, const int* __restrict__ texel_offset,
                                                                   const float* __restrict__ texel_bary, float* __restrict__ tex) {
    const long long base = (long long)blockIdx.x * kTexThreads;
    const long long f0 = base / n;
    const uint32_t l = (uint32_t)(base - f0 * n) + threadIdx.x;
    const uint32_t df = l / n, t = l - df * n;
    const long long f = f0 + df;
    if (f >= F) return;
    FaceCorners corners;
    if (!load_face_checked(verts, faces, V, (size_t)f, corners)) return;
    const size_t row_of_tables = (size_t)(f & 1) * n + t;
    const int o0 = texel_offset[2 * row_of_tables + 0], o1 = texel_offset[2 * row_of_tables + 1];
    if (o0 < 0 || o0 >= S || o1 < 0 || o1 >= S) return;        // (the tables are the caller's: nothing is written outside the face's square)
    const float w0 = texel_bary[3 * row_of_tables + 0], w1 = texel_bary[3 * row_of_tables + 1], w2 = texel_bary[3 * row_of_tables + 2];
    const Vec3 x = add(add(scale(w0, corners.v0), scale(w1, corners.v1)), scale(w2, corners.v2));

    int best = 0;
    float best_q = 0.0f;
    for (int g = 0; g < G; ++g) {
        const size_t j = (size_t)f * (size_t)G + (size_t)g;
        const float* c = centers + 3 * j;
        const float* m = M + 9 * j;
        const float s0 = x.x - c[0], s1 = x.y - c[1], s2 = x.z - c[2];
        float w[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) w[a] = (m[a] * s0 + m[3 + a] * s1) + m[6 + a] * s2;
        const float q_raw = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
        const float q = q_raw < 0.0f ? 0.0f : (q_raw > 1e8f ? 1e8f : q_raw);   // (a NaN stays one)
        // the first NaN wins; else the first smallest
        if (g == 0 || (best_q == best_q && (q != q || q < best_q))) best = g, best_q = q;
    }
    const long long s = f >> 1;
    const int a = (int)(s / A), b = (int)(s - (long long)a * A);
    const int T = A * S;
    const size_t at = ((size_t)(T - 1 - (b * S + o1)) * (size_t)T + (size_t)(a * S + o0)) * 3u;
    const float* feat = features + 3 * ((size_t)f * (size_t)G + (size_t)best);
#pragma unroll
    for (int c = 0; c < 3; ++c) tex[at + c] = feat[c] * kShC0 + 0.5f;
}

// What the three per-pixel entry points refuse, or nullptr.
const char* bad_view(int64_t P, int64_t F, int T, const int64_t* pix_to_face, const float* bary, const float* zbuf, const float* face_uvs) {
    if (P < 0 || F < 0) return "negative count";
    if (P > (int64_t)0xFFFFFFFEll) return "more than 2^32 - 2 pixels";
    if (F >= ((int64_t)1 << 31)) return "2^31 faces or more";
    if (T < 1 || T > kTexMaxT) return "texture_size outside 1..46340 (T * T < 2^31)";
    if ((P > 0 && (!pix_to_face || !bary || !zbuf)) || (F > 0 && !face_uvs)) return "null pointer";
    if (!aligned8(pix_to_face) || !aligned4(bary) || !aligned4(zbuf) || !aligned4(face_uvs))
        return "misaligned pointer (floats: 4 bytes, pix_to_face: 8)";
    return nullptr;
}

}  // namespace
}  // namespace gsr

using gsr::fail;

extern "C" {

int gsr_texture_texels(int64_t P, int64_t F, int T, const int64_t* pix_to_face, const float* bary, const float* zbuf, const float* face_uvs,
                       int32_t* texel, void* stream_) {
    if (const char* why = gsr::bad_view(P, F, T, pix_to_face, bary, zbuf, face_uvs)) return fail(GSR_ERR_INVALID_ARG, "gsr_texture_texels: %s", why);
    if (P > 0 && !texel) return fail(GSR_ERR_INVALID_ARG, "gsr_texture_texels: null pointer");
    if (!gsr::aligned4(texel)) return fail(GSR_ERR_INVALID_ARG, "gsr_texture_texels: misaligned pointer (texel: 4 bytes)");
    if (P == 0) return GSR_OK;
    hipLaunchKernelGGL(gsr::texture_texels_kernel, dim3(gsr::blocks_of(P, gsr::kTexThreads)), dim3(gsr::kTexThreads), 0, (hipStream_t)stream_,
                       (long long)P, (long long)F, T, reinterpret_cast<const long long*>(pix_to_face), bary, zbuf, face_uvs, texel);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_texture_bake_view(int64_t P, int64_t F, int T, const int64_t* pix_to_face, const float* bary, const float* zbuf,
                          const float* face_uvs, const float* rgb, int64_t rgb_stride, float* tex, float* count, uint32_t* owner,
                          void* stream_) {
    if (const char* why = gsr::bad_view(P, F, T, pix_to_face, bary, zbuf, face_uvs)) return fail(GSR_ERR_INVALID_ARG, "gsr_texture_bake_view: %s", why);
    if (rgb_stride < 3 || rgb_stride >= ((int64_t)1 << 31)) return fail(GSR_ERR_INVALID_ARG, "gsr_texture_bake_view: rgb_stride outside 3..2^31 - 1");
    if (!tex || !count || !owner || (P > 0 && !rgb)) return fail(GSR_ERR_INVALID_ARG, "gsr_texture_bake_view: null pointer");
    if (!gsr::aligned4(rgb) || !gsr::aligned4(tex) || !gsr::aligned4(count) || !gsr::aligned4(owner))
        return fail(GSR_ERR_INVALID_ARG, "gsr_texture_bake_view: misaligned pointer (rgb, tex, count, owner: 4 bytes)");
    if (P == 0 || F == 0) return GSR_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid(gsr::blocks_of(P, gsr::kTexThreads)), block(gsr::kTexThreads);
    const long long* pix = reinterpret_cast<const long long*>(pix_to_face);
    hipLaunchKernelGGL(gsr::texture_claim_kernel, grid, block, 0, stream, (long long)P, (long long)F, T, pix, bary, zbuf, face_uvs, owner);
    hipLaunchKernelGGL(gsr::texture_accumulate_kernel, grid, block, 0, stream, (long long)P, (long long)F, T, pix, bary, zbuf, face_uvs, rgb,
                       (long long)rgb_stride, tex, count, owner);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

int gsr_texture_fill(int64_t V, int64_t F, int G, int A, int S, int n, const float* verts, const int64_t* faces, const float* centers,
                     const float* inv_scaled_rot, const float* features, const int32_t* texel_offset, const float* texel_bary, float* tex,
                     void* stream_) {
    if (V < 0 || F < 0) return fail(GSR_ERR_INVALID_ARG, "gsr_texture_fill: negative count");
    if (V >= ((int64_t)1 << 31) || F >= ((int64_t)1 << 28)) return fail(GSR_ERR_INVALID_ARG, "gsr_texture_fill: V >= 2^31 or F >= 2^28");
    if (G < 1 || G > gsr::kTexMaxG) return fail(GSR_ERR_INVALID_ARG, "gsr_texture_fill: G = %d (1 to %d)", G, gsr::kTexMaxG);
    if (S < gsr::kTexMinS || S > gsr::kTexMaxS) return fail(GSR_ERR_INVALID_ARG, "gsr_texture_fill: S = %d (%d to %d)", S, gsr::kTexMinS, gsr::kTexMaxS);
    if (A < 1 || (int64_t)A * S > gsr::kTexMaxT) return fail(GSR_ERR_INVALID_ARG, "gsr_texture_fill: A = %d (A >= 1, A * S <= %d)", A, gsr::kTexMaxT);
    if ((F + 1) / 2 > (int64_t)A * A) return fail(GSR_ERR_INVALID_ARG, "gsr_texture_fill: %lld faces need more than A * A = %d squares", (long long)F, A * A);
    if (n < 1 || n > S * S) return fail(GSR_ERR_INVALID_ARG, "gsr_texture_fill: n = %d (1 to S * S)", n);
    if (!tex || !texel_offset || !texel_bary || (V > 0 && !verts) || (F > 0 && (!faces || !centers || !inv_scaled_rot || !features)))
        return fail(GSR_ERR_INVALID_ARG, "gsr_texture_fill: null pointer");
    if (!gsr::aligned4(verts) || !gsr::aligned8(faces) || !gsr::aligned4(centers) || !gsr::aligned4(inv_scaled_rot) || !gsr::aligned4(features) ||
        !gsr::aligned4(texel_offset) || !gsr::aligned4(texel_bary) || !gsr::aligned4(tex))
        return fail(GSR_ERR_INVALID_ARG, "gsr_texture_fill: misaligned pointer (floats and int32: 4 bytes, faces: 8)");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t floats = (size_t)A * S * (size_t)A * S * 3u;
    const unsigned cblocks = (unsigned)((floats + gsr::kTexThreads - 1) / gsr::kTexThreads);
    hipLaunchKernelGGL(gsr::texture_constant_kernel, dim3(cblocks < 8192u ? cblocks : 8192u), dim3(gsr::kTexThreads), 0, stream, tex, floats, 0.5f);
    if (F > 0)
        hipLaunchKernelGGL(gsr::texture_fill_kernel, dim3(gsr::blocks_of(F * (int64_t)n, gsr::kTexThreads)), dim3(gsr::kTexThreads), 0, stream,
                           (long long)V, (long long)F, G, A, S, (uint32_t)n, verts, reinterpret_cast<const long long*>(faces), centers,
                           inv_scaled_rot, features, texel_offset, texel_bary, tex);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

}  // extern "C"
