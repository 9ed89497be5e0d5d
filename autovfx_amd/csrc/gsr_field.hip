// gsr_field.hip -- SuGaR's density field over a neighbour list, forward and backward (include/gsr.h: gsr_field_forward,
// gsr_field_backward).
//
// SuGaR.get_field_values (sugar/sugar_scene/sugar_model.py:1118-1187) and SuGaR.compute_density (:1216-1239) gather, for N samples and
// their K nearest Gaussians, [N,K,3] centres, [N,K,3,3] inverse scaled rotations and [N,K] strengths, and sum K Gaussian bumps per sample.
// Here one lane owns a sample and walks its K neighbours; nothing of size [N,K] exists except the outputs the caller asked for.
//
// The contract, per (sample i, slot k) with j = idx[i,k], plain fp32, left to right, no contraction (-ffp-contract=off):
//   s_b = x_i[b] - c_j[b]
//   w_a = (M_j[0][a] s_0 + M_j[1][a] s_1) + M_j[2][a] s_2                    (M^T s, :1146)
//   q   = clamp((w_0 w_0 + w_1 w_1) + w_2 w_2, 0, 1e8)
//   o   = (density_factor sigma_j) expf(-0.5 q)
//   density[i] = sum_k o, beta[i] = (sum_k m_j) / K, both from 0 with k ascending
// A slot with j outside [0, P) is skipped: 0 to both sums, an opacity of 0, no gradient, nothing read.
//
// Kernels:
//   field_pack_kernel       one lane per Gaussian: centre, matrix, strength and minimum scale into one 64-byte record, so that a
//                           (sample, neighbour) pair touches one line instead of three or four scattered ones.
//   field_forward_kernel    256 samples per workgroup.  The neighbour list is walked in rounds of 16 slots: the round's [256 x 16]
//                           block of int64 indices is read with coalesced loads into LDS (range-checked, as int32), each lane then
//                           reads its own row from LDS (pitch 17 words: no bank conflicts), and the round's opacities leave through
//                           the same tile with coalesced stores.
//   field_backward_kernel   the same walk; w, q and expf are recomputed.  dx stays in the lane's registers.  The 14 per-Gaussian
//                           gradients (3 centre, 9 matrix, strength, minimum scale) go by float atomics into the Gaussian's 64-byte
//                           line of accum [P,16].  The 64 pairs of a wave are first laid out in LDS so that 16 consecutive lanes
//                           add into one line (4 lines of 64 bytes per wave-instruction) instead of 64 lanes into 64 lines, which
//                           was measured 13 x slower.  Exact zeros are not added.
//   level_surface_kernel   the ray march of SuGaR's coarse mesh extraction (compute_level_surface_points_from_camera_fast,
//                           sugar_model.py:1853-1950): one lane owns a ray and keeps the running densities of its S <= 32
//                           samples in registers.  The neighbour loop is outermost, so a record is read once per ray instead of once
//                           per sample and every density is still summed with k ascending; the crossings of up to 8 levels are found
//                           in registers, and a second walk over the same K records sums the field's gradient at every crossing.
// No host synchronisation, no allocation, everything on the caller's stream.
// Defines the entry points gsr_field_scratch_bytes, gsr_field_forward, gsr_field_backward and gsr_level_surface.
#include "gsr_internal.h"

namespace gsr {
namespace {

constexpr int kThreads = 256;
constexpr int kRound = 16;             // neighbour slots staged per round
constexpr int kPitch = kRound + 1;     // LDS row pitch in words: lane l reads word l * 17 + kk
constexpr int kLine = 16;              // floats per packed record and per accumulator line
constexpr int kGrads = 14;             // of which are gradients: dc 0-2, dM 3-11, dsigma 12, dm 13
constexpr int kFieldMaxK = 64;
struct FieldInputs {
    int64_t n;                   // samples, 0 < n < 2^30
    int K;                       // neighbour slots per sample, 1 .. kFieldMaxK
    int64_t P;                   // Gaussians, 0 <= P < 2^30
    const float* x;              // [n,3]
    const long long* idx;        // [n,K]; a slot outside [0, P) is skipped
    const float *centers, *M, *strengths, *min_scaling;   // [P,3], [P,3,3], [P], [P] or null
    float density_factor;
};

__global__ __launch_bounds__(kThreads) void field_pack_kernel(uint32_t P, const float* __restrict__ centers, const float* __restrict__ M,
                                                              const float* __restrict__ strengths, const float* __restrict__ min_scaling,
                                                              float4* __restrict__ packed) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= P) return;
    const float* c = centers + (size_t)j * 3;
    const float* m = M + (size_t)j * 9;
    float4* out = packed + (size_t)j * 4;
    out[0] = make_float4(c[0], c[1], c[2], m[0]);
    out[1] = make_float4(m[1], m[2], m[3], m[4]);
    out[2] = make_float4(m[5], m[6], m[7], m[8]);
    out[3] = make_float4(strengths[j], min_scaling ? min_scaling[j] : 0.0f, 0.0f, 0.0f);
}

// One (sample, Gaussian) pair of the contract.
struct Pair {
    float s[3], w[3], M[9], q_raw, e, sigma, m;
};

__device__ __forceinline__ void eval_pair(const float4* __restrict__ packed, int j, float x0, float x1, float x2, Pair& p) {
    const float4* r = packed + (size_t)j * 4;
    const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    p.M[0] = r0.w; p.M[1] = r1.x; p.M[2] = r1.y; p.M[3] = r1.z; p.M[4] = r1.w;
    p.M[5] = r2.x; p.M[6] = r2.y; p.M[7] = r2.z; p.M[8] = r2.w;
    p.sigma = r3.x;
    p.m = r3.y;
    p.s[0] = x0 - r0.x;
    p.s[1] = x1 - r0.y;
    p.s[2] = x2 - r0.z;
#pragma unroll
    for (int a = 0; a < 3; ++a) p.w[a] = (p.M[a] * p.s[0] + p.M[3 + a] * p.s[1]) + p.M[6 + a] * p.s[2];
    p.q_raw = (p.w[0] * p.w[0] + p.w[1] * p.w[1]) + p.w[2] * p.w[2];
    const float q = p.q_raw < 0.0f ? 0.0f : (p.q_raw > 1e8f ? 1e8f : p.q_raw);   // (a NaN stays one, as torch's clamp leaves it)
    p.e = expf(-0.5f * q);
}

// The [256 x kc] block of idx rows first .. first+255, slots k0 .. k0+kc-1, into tile[row * kPitch + kk] as int32; -1 for a slot
// outside [0, P) and for rows past n.  Consecutive lanes read consecutive slots of a row: runs of 8 kc bytes.
__device__ __forceinline__ void stage_indices(int* tile, const long long* __restrict__ idx, uint32_t first, uint32_t n, int K, int k0, int kc,
                                              long long P) {
    for (int e = (int)threadIdx.x; e < kThreads * kc; e += kThreads) {
        const int row = e / kc, kk = e - row * kc;
        const uint32_t i = first + (uint32_t)row;
        int j = -1;
        if (i < n) {
            const long long v = idx[(size_t)i * (size_t)K + (size_t)(k0 + kk)];
            if (v >= 0 && v < P) j = (int)v;
        }
        tile[row * kPitch + kk] = j;
    }
}

__device__ __forceinline__ void stage_floats(float* tile, const float* __restrict__ src, uint32_t first, uint32_t n, int K, int k0, int kc) {
    for (int e = (int)threadIdx.x; e < kThreads * kc; e += kThreads) {
        const int row = e / kc, kk = e - row * kc;
        const uint32_t i = first + (uint32_t)row;
        tile[row * kPitch + kk] = i < n ? src[(size_t)i * (size_t)K + (size_t)(k0 + kk)] : 0.0f;
    }
}

__global__ __launch_bounds__(kThreads) void field_forward_kernel(uint32_t n, int K, long long P, const float* __restrict__ x,
                                                                 const long long* __restrict__ idx, const float4* __restrict__ packed,
                                                                 float density_factor, float* __restrict__ density,
                                                                 float* __restrict__ opacities, float* __restrict__ beta) {
    __shared__ int tile[kThreads * kPitch];   // a round's indices, then (same words) its opacities
    const uint32_t first = blockIdx.x * kThreads;
    const uint32_t i = first + threadIdx.x;
    const bool active = i < n;
    float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f;
    if (active) {
        x0 = x[(size_t)i * 3];
        x1 = x[(size_t)i * 3 + 1];
        x2 = x[(size_t)i * 3 + 2];
    }
    float dens = 0.0f, msum = 0.0f;
    for (int k0 = 0; k0 < K; k0 += kRound) {
        const int kc = K - k0 < kRound ? K - k0 : kRound;
        __syncthreads();
        stage_indices(tile, idx, first, n, K, k0, kc, P);
        __syncthreads();
        if (active) {
            int* row = tile + threadIdx.x * kPitch;
            for (int kk = 0; kk < kc; ++kk) {
                const int j = row[kk];
                float o = 0.0f;
                if (j >= 0) {
                    Pair p;
                    eval_pair(packed, j, x0, x1, x2, p);
                    o = (density_factor * p.sigma) * p.e;
                    msum = msum + p.m;
                }
                dens = dens + o;
                row[kk] = __float_as_int(o);
            }
        }
        if (opacities) {
            __syncthreads();
            for (int e = (int)threadIdx.x; e < kThreads * kc; e += kThreads) {
                const int r = e / kc, kk = e - r * kc;
                const uint32_t ir = first + (uint32_t)r;
                if (ir < n) opacities[(size_t)ir * (size_t)K + (size_t)(k0 + kk)] = __int_as_float(tile[r * kPitch + kk]);
            }
        }
    }
    if (active) {
        density[i] = dens;
        if (beta) beta[i] = msum / (float)K;
    }
}

__global__ __launch_bounds__(kThreads) void field_backward_kernel(uint32_t n, int K, long long P, const float* __restrict__ x,
                                                                  const long long* __restrict__ idx, const float4* __restrict__ packed,
                                                                  float density_factor, const float* __restrict__ g_density,
                                                                  const float* __restrict__ g_opacities, const float* __restrict__ g_beta,
                                                                  float* __restrict__ dx, float* __restrict__ accum) {
    __shared__ int tile_j[kThreads * kPitch];
    __shared__ float tile_g[kThreads * kPitch];
    __shared__ float tile_v[kThreads * kPitch];   // per wave: 64 pairs x 14 gradients, pitch 17
    __shared__ int tile_t[kThreads];              // ... and their Gaussians
    const uint32_t first = blockIdx.x * kThreads;
    const uint32_t i = first + threadIdx.x;
    const bool active = i < n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f, gd = 0.0f, gm = 0.0f;
    if (active) {
        x0 = x[(size_t)i * 3];
        x1 = x[(size_t)i * 3 + 1];
        x2 = x[(size_t)i * 3 + 2];
        if (g_density) gd = g_density[i];
        if (g_beta) gm = g_beta[i] / (float)K;
    }
    float dx0 = 0.0f, dx1 = 0.0f, dx2 = 0.0f;
    for (int k0 = 0; k0 < K; k0 += kRound) {
        const int kc = K - k0 < kRound ? K - k0 : kRound;
        __syncthreads();
        stage_indices(tile_j, idx, first, n, K, k0, kc, P);
        if (g_opacities) stage_floats(tile_g, g_opacities, first, n, K, k0, kc);
        __syncthreads();
        for (int kk = 0; kk < kc; ++kk) {
            const int j = active ? tile_j[threadIdx.x * kPitch + kk] : -1;
            float v[kGrads];
#pragma unroll
            for (int c = 0; c < kGrads; ++c) v[c] = 0.0f;
            if (j >= 0) {
                Pair p;
                eval_pair(packed, j, x0, x1, x2, p);
                const float G = g_opacities ? gd + tile_g[threadIdx.x * kPitch + kk] : gd;
                const float o = (density_factor * p.sigma) * p.e;
                const float dq = (p.q_raw < 0.0f || p.q_raw > 1e8f) ? 0.0f : (-0.5f * G) * o;   // torch's clamp passes min <= q <= max
                float dw[3], ds[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) dw[a] = (2.0f * p.w[a]) * dq;
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    ds[b] = (p.M[3 * b] * dw[0] + p.M[3 * b + 1] * dw[1]) + p.M[3 * b + 2] * dw[2];
                    v[b] = -ds[b];
#pragma unroll
                    for (int a = 0; a < 3; ++a) v[3 + 3 * b + a] = p.s[b] * dw[a];
                }
                dx0 = dx0 + ds[0];
                dx1 = dx1 + ds[1];
                dx2 = dx2 + ds[2];
                v[12] = (G * density_factor) * p.e;
                v[13] = gm;
            }
            // 64 pairs x 14 values of this wave, then 16 lanes per Gaussian's line
            float* mine = tile_v + wave * 64 * kPitch;
#pragma unroll
            for (int c = 0; c < kGrads; ++c) mine[lane * kPitch + c] = v[c];
            tile_t[threadIdx.x] = j;
            __syncthreads();
            const int c = lane & 15;
            if (c < kGrads) {
                for (int it = 0; it < 16; ++it) {
                    const int pair = it * 4 + (lane >> 4);
                    const int jj = tile_t[wave * 64 + pair];
                    if (jj >= 0) {
                        const float val = mine[pair * kPitch + c];
                        if (val != 0.0f) atomicAdd(accum + (size_t)jj * kLine + c, val);
                    }
                }
            }
            __syncthreads();
        }
    }
    if (active && dx) {
        dx[(size_t)i * 3] = dx0;
        dx[(size_t)i * 3 + 1] = dx1;
        dx[(size_t)i * 3 + 2] = dx2;
    }
}

constexpr int kLevelMaxS = 32;         // samples per ray: the densities are a fixed register array
constexpr int kLevelMaxL = 8;          // levels per call
struct LevelSet {
    float v[kLevelMaxL];
};

// Per ray i (include/gsr.h: gsr_level_surface): tau_s = range[s] stds[i], x_s = origins[i] + tau_s dirs[i], d_s = the field at x_s
// (eval_pair's contract, k ascending, >= 1 renormalised), per level the first s with d_s > level after d_0 < level, the interpolated
// crossing, and there -g / max(|g|, 1e-12) with g = sum_k o_k (M_k w_k).  The loops over s and over the levels are unrolled to their
// largest counts under uniform guards, so that d[], the crossings and g[] are registers.
__global__ __launch_bounds__(kThreads) void level_surface_kernel(uint32_t n, int K, long long P, int S, int L, const float* __restrict__ origins,
                                                                 const float* __restrict__ dirs, const float* __restrict__ stds,
                                                                 const long long* __restrict__ idx, const float4* __restrict__ packed,
                                                                 float density_factor, const float* __restrict__ range, LevelSet levels,
                                                                 unsigned char* __restrict__ hit, float* __restrict__ t_out,
                                                                 float* __restrict__ points, float* __restrict__ normals,
                                                                 float* __restrict__ densities) {
    __shared__ int tile[kThreads * kPitch];
    const uint32_t first = blockIdx.x * kThreads;
    const uint32_t i = first + threadIdx.x;
    const bool active = i < n;
    float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f, v0 = 0.0f, v1 = 0.0f, v2 = 0.0f, sd = 0.0f;
    if (active) {
        o0 = origins[(size_t)i * 3];
        o1 = origins[(size_t)i * 3 + 1];
        o2 = origins[(size_t)i * 3 + 2];
        v0 = dirs[(size_t)i * 3];
        v1 = dirs[(size_t)i * 3 + 1];
        v2 = dirs[(size_t)i * 3 + 2];
        sd = stds[i];
    }
    float tau[kLevelMaxS], d[kLevelMaxS];
#pragma unroll
    for (int s = 0; s < kLevelMaxS; ++s) {
        tau[s] = s < S ? range[s] * sd : 0.0f;
        d[s] = 0.0f;
    }
    const int* row = tile + threadIdx.x * kPitch;
    for (int k0 = 0; k0 < K; k0 += kRound) {
        const int kc = K - k0 < kRound ? K - k0 : kRound;
        __syncthreads();
        stage_indices(tile, idx, first, n, K, k0, kc, P);
        __syncthreads();
        if (!active) continue;
        for (int kk = 0; kk < kc; ++kk) {
            const int j = row[kk];
            if (j < 0) continue;
#pragma unroll
            for (int s = 0; s < kLevelMaxS; ++s) {
                if (s >= S) break;            // (a chain of exits, not 32 separate guards: the record's loads then dominate every sample)
                Pair p;
                eval_pair(packed, j, o0 + tau[s] * v0, o1 + tau[s] * v1, o2 + tau[s] * v2, p);
                d[s] = d[s] + (density_factor * p.sigma) * p.e;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < kLevelMaxS; ++s) {
        if (s < S) {
            if (d[s] >= 1.0f) d[s] = d[s] / (d[s] + 1e-12f);
            if (active && densities) densities[(size_t)i * (size_t)S + (size_t)s] = d[s];
        }
    }
    float px[kLevelMaxL], py[kLevelMaxL], pz[kLevelMaxL];
    unsigned hits = 0u;
#pragma unroll
    for (int l = 0; l < kLevelMaxL; ++l) {
        px[l] = py[l] = pz[l] = 0.0f;
        if (l < L) {
            const float level = levels.v[l];
            bool found = false;
            float d_a = 0.0f, d_b = 0.0f, tau_a = 0.0f, tau_b = 0.0f;
#pragma unroll
            for (int s = 1; s < kLevelMaxS; ++s) {
                if (s < S && !found && d[s] > level) {
                    found = true;
                    d_a = d[s];
                    d_b = d[s - 1];
                    tau_a = tau[s];
                    tau_b = tau[s - 1];
                }
            }
            float t = 0.0f;
            if (found && d[0] < level) {      // (d_0 > level: the first sample above is sample 0; a NaN is neither under nor above)
                t = (level - d_b) / (d_a - d_b) * (tau_a - tau_b) + tau_b;
                px[l] = o0 + t * v0;
                py[l] = o1 + t * v1;
                pz[l] = o2 + t * v2;
                hits |= 1u << l;
            }
            if (active) {
                const size_t at = (size_t)l * (size_t)n + (size_t)i;
                hit[at] = (unsigned char)((hits >> l) & 1u);
                t_out[at] = t;
                points[at * 3] = px[l];
                points[at * 3 + 1] = py[l];
                points[at * 3 + 2] = pz[l];
            }
        }
    }
    if (!normals) return;
    float g0[kLevelMaxL], g1[kLevelMaxL], g2[kLevelMaxL];
#pragma unroll
    for (int l = 0; l < kLevelMaxL; ++l) g0[l] = g1[l] = g2[l] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += kRound) {
        const int kc = K - k0 < kRound ? K - k0 : kRound;
        if (K > kRound) {                     // (K <= 16: the tile still holds the one round)
            __syncthreads();
            stage_indices(tile, idx, first, n, K, k0, kc, P);
            __syncthreads();
        }
        if (hits == 0u) continue;
        for (int kk = 0; kk < kc; ++kk) {
            const int j = row[kk];
            if (j < 0) continue;
#pragma unroll
            for (int l = 0; l < kLevelMaxL; ++l) {
                if (l < L && ((hits >> l) & 1u)) {
                    Pair p;
                    eval_pair(packed, j, px[l], py[l], pz[l], p);
                    const float o = (density_factor * p.sigma) * p.e;
                    g0[l] = g0[l] + o * ((p.M[0] * p.w[0] + p.M[1] * p.w[1]) + p.M[2] * p.w[2]);
                    g1[l] = g1[l] + o * ((p.M[3] * p.w[0] + p.M[4] * p.w[1]) + p.M[5] * p.w[2]);
                    g2[l] = g2[l] + o * ((p.M[6] * p.w[0] + p.M[7] * p.w[1]) + p.M[8] * p.w[2]);
                }
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int l = 0; l < kLevelMaxL; ++l) {
        if (l < L) {
            float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f;
            if ((hits >> l) & 1u) {
                const float norm = sqrtf((g0[l] * g0[l] + g1[l] * g1[l]) + g2[l] * g2[l]);
                const float den = norm > 1e-12f ? norm : 1e-12f;
                m0 = -(g0[l] / den);
                m1 = -(g1[l] / den);
                m2 = -(g2[l] / den);
            }
            const size_t at = ((size_t)l * (size_t)n + (size_t)i) * 3;
            normals[at] = m0;
            normals[at + 1] = m1;
            normals[at + 2] = m2;
        }
    }
}

hipError_t pack(const FieldInputs& in, void* scratch, hipStream_t stream) {
    if (in.P == 0) return hipSuccess;
    hipLaunchKernelGGL(field_pack_kernel, dim3((uint32_t)((in.P + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, (uint32_t)in.P,
                       in.centers, in.M, in.strengths, in.min_scaling, reinterpret_cast<float4*>(scratch));
    return hipGetLastError();
}

// scratch: field_scratch_bytes(P) bytes (one 64-byte record per Gaussian), 256-byte aligned, any content; both calls fill it themselves.
size_t field_scratch_bytes(int64_t P) { return (size_t)(P > 0 ? P : 1) * kLine * sizeof(float); }

hipError_t launch_field_forward(const FieldInputs& in, float* density, float* opacities, float* beta, void* scratch, hipStream_t stream) {
    hipError_t e = pack(in, scratch, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(field_forward_kernel, dim3((uint32_t)((in.n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, (uint32_t)in.n,
                       in.K, (long long)in.P, in.x, in.idx, reinterpret_cast<const float4*>(scratch), in.density_factor, density, opacities,
                       beta);
    return hipGetLastError();
}

// accum [P,16], zeroed by the caller, 64-byte aligned: floats 0-2 of a line dL/dcentre, 3-11 dL/dM row-major, 12 dL/dstrength,
// 13 dL/dmin_scaling.
hipError_t launch_field_backward(const FieldInputs& in, const float* g_density, const float* g_opacities, const float* g_beta, float* dx,
                                 float* accum, void* scratch, hipStream_t stream) {
    hipError_t e = pack(in, scratch, stream);
    if (e != hipSuccess) return e;
    const dim3 grid((uint32_t)((in.n + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(field_backward_kernel, grid, dim3(kThreads), 0, stream, (uint32_t)in.n, in.K, (long long)in.P, in.x, in.idx,
                       reinterpret_cast<const float4*>(scratch), in.density_factor, g_density, g_opacities, g_beta, dx, accum);
    return hipGetLastError();
}

hipError_t launch_level_surface(const FieldInputs& in, const float* dirs, const float* stds, int S, int L, const float* range,
                                const LevelSet& levels, unsigned char* hit, float* t, float* points, float* normals, float* densities,
                                void* scratch, hipStream_t stream) {
    hipError_t e = pack(in, scratch, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(level_surface_kernel, dim3((uint32_t)((in.n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, (uint32_t)in.n,
                       in.K, (long long)in.P, S, L, in.x, dirs, stds, in.idx, reinterpret_cast<const float4*>(scratch), in.density_factor,
                       range, levels, hit, t, points, normals, densities);
    return hipGetLastError();
}

}  // namespace
}  // namespace gsr

using gsr::fail;

namespace {
// What gsr_field_forward and gsr_field_backward check alike; 1: n == 0, nothing to do.
int field_check(const char* who, const gsr::FieldInputs& in, bool wants_beta, const void* scratch, size_t scratch_bytes) {
    if (in.K < 1 || in.K > gsr::kFieldMaxK) return fail(GSR_ERR_INVALID_ARG, "%s: K = %d (1 to %d)", who, in.K, gsr::kFieldMaxK);
    if (in.n < 0 || in.P < 0) return fail(GSR_ERR_INVALID_ARG, "%s: negative count (n %lld, P %lld)", who, (long long)in.n, (long long)in.P);
    if (in.n >= (int64_t)gsr::kKnn3MaxPoints || in.P >= (int64_t)gsr::kKnn3MaxPoints)
        return fail(GSR_ERR_INVALID_ARG, "%s: %lld samples and %lld Gaussians (at most 2^30 - 1 each)", who, (long long)in.n, (long long)in.P);
    if (in.n == 0) return 1;
    if (!in.x || !in.idx || !scratch || (in.P > 0 && (!in.centers || !in.M || !in.strengths)))
        return fail(GSR_ERR_INVALID_ARG, "%s: null pointer", who);
    if (wants_beta && !in.min_scaling) return fail(GSR_ERR_INVALID_ARG, "%s: beta needs min_scaling", who);
    if ((((uintptr_t)in.x | (uintptr_t)in.centers | (uintptr_t)in.M | (uintptr_t)in.strengths | (uintptr_t)in.min_scaling) & 3u) != 0u ||
        !gsr::aligned8(in.idx) || !gsr::aligned256(scratch))
        return fail(GSR_ERR_INVALID_ARG, "%s: misaligned pointer (floats: 4 bytes, idx: 8, scratch: 256)", who);
    const size_t need = gsr::field_scratch_bytes(in.P);
    if (scratch_bytes < need) return fail(GSR_ERR_INVALID_ARG, "%s: scratch too small (%zu of %zu bytes)", who, scratch_bytes, need);
    return GSR_OK;
}
}  // namespace

extern "C" {

size_t gsr_field_scratch_bytes(int64_t P) {
    return (P < 0 || P >= (int64_t)gsr::kKnn3MaxPoints) ? 0 : gsr::field_scratch_bytes(P);
}

int gsr_field_forward(int64_t n, int K, int64_t P, const float* x, const int64_t* idx, const float* centers, const float* M,
                      const float* strengths, const float* min_scaling, float density_factor, float* density, float* opacities, float* beta,
                      void* scratch, size_t scratch_bytes, void* stream_) {
    const gsr::FieldInputs in{n, K, P, x, reinterpret_cast<const long long*>(idx), centers, M, strengths, min_scaling, density_factor};
    const int rc = field_check("gsr_field_forward", in, beta != nullptr, scratch, scratch_bytes);
    if (rc != GSR_OK) return rc == 1 ? GSR_OK : rc;
    if (!density) return fail(GSR_ERR_INVALID_ARG, "gsr_field_forward: null pointer");
    if ((((uintptr_t)density | (uintptr_t)opacities | (uintptr_t)beta) & 3u) != 0u)
        return fail(GSR_ERR_INVALID_ARG, "gsr_field_forward: misaligned pointer (density / opacities / beta: 4 bytes)");
    GSR_HIP(gsr::launch_field_forward(in, density, opacities, beta, scratch, (hipStream_t)stream_));
    return GSR_OK;
}

int gsr_field_backward(int64_t n, int K, int64_t P, const float* x, const int64_t* idx, const float* centers, const float* M,
                       const float* strengths, const float* min_scaling, float density_factor, const float* g_density,
                       const float* g_opacities, const float* g_beta, float* dx, float* accum, void* scratch, size_t scratch_bytes,
                       void* stream_) {
    const gsr::FieldInputs in{n, K, P, x, reinterpret_cast<const long long*>(idx), centers, M, strengths, min_scaling, density_factor};
    const int rc = field_check("gsr_field_backward", in, g_beta != nullptr, scratch, scratch_bytes);
    if (rc != GSR_OK) return rc == 1 ? GSR_OK : rc;
    if (!accum && P > 0) return fail(GSR_ERR_INVALID_ARG, "gsr_field_backward: null pointer");
    if ((((uintptr_t)g_density | (uintptr_t)g_opacities | (uintptr_t)g_beta | (uintptr_t)dx) & 3u) != 0u || ((uintptr_t)accum & 63u) != 0u)
        return fail(GSR_ERR_INVALID_ARG, "gsr_field_backward: misaligned pointer (gradients: 4 bytes, accum: 64)");
    GSR_HIP(gsr::launch_field_backward(in, g_density, g_opacities, g_beta, dx, accum, scratch, (hipStream_t)stream_));
    return GSR_OK;
}

int gsr_level_surface(int64_t n, int K, int64_t P, int S, int L, const float* origins, const float* dirs, const float* stds,
                      const int64_t* idx, const float* centers, const float* M, const float* strengths, float density_factor,
                      const float* range, const float* levels, uint8_t* hit, float* t, float* points, float* normals, float* densities,
                      void* scratch, size_t scratch_bytes, void* stream_) {
    const char* who = "gsr_level_surface";
    if (S < 2 || S > gsr::kLevelMaxS) return fail(GSR_ERR_INVALID_ARG, "%s: S = %d (2 to %d)", who, S, gsr::kLevelMaxS);
    if (L < 1 || L > gsr::kLevelMaxL) return fail(GSR_ERR_INVALID_ARG, "%s: L = %d (1 to %d)", who, L, gsr::kLevelMaxL);
    const gsr::FieldInputs in{n, K, P, origins, reinterpret_cast<const long long*>(idx), centers, M, strengths, nullptr, density_factor};
    const int rc = field_check(who, in, false, scratch, scratch_bytes);
    if (rc != GSR_OK) return rc == 1 ? GSR_OK : rc;
    if (!dirs || !stds || !range || !levels || !hit || !t || !points) return fail(GSR_ERR_INVALID_ARG, "%s: null pointer", who);
    if ((((uintptr_t)dirs | (uintptr_t)stds | (uintptr_t)range | (uintptr_t)levels | (uintptr_t)t | (uintptr_t)points | (uintptr_t)normals |
          (uintptr_t)densities) & 3u) != 0u)
        return fail(GSR_ERR_INVALID_ARG, "%s: misaligned pointer (dirs / stds / range / levels / t / points / normals / densities: 4 bytes)", who);
    gsr::LevelSet set{};
    for (int l = 0; l < L; ++l) set.v[l] = levels[l];
    GSR_HIP(gsr::launch_level_surface(in, dirs, stds, S, L, range, set, hit, t, points, normals, densities, scratch, (hipStream_t)stream_));
    return GSR_OK;
}

}  // extern "C"
