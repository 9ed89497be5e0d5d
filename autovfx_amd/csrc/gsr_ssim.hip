// gsr_ssim.hip -- the structural similarity of the reference's training loss (include/gsr.h: gsr_ssim_forward / gsr_ssim_backward).
//
// The drop-in for loss_utils.ssim (sugar/gaussian_splatting/utils/loss_utils.py:33-62): per plane (n, c), with zero padding outside
// the image as conv2d(padding=5) has it,
//   mx = w*x, my = w*y, Exx = w*x^2, Eyy = w*y^2, Exy = w*xy           (w: the separable 11-tap Gaussian, sigma 1.5)
//   A1 = 2 mx my + C1, A2 = 2 (Exy - mx my) + C2, B1 = mx^2 + my^2 + C1, B2 = (Exx - mx^2) + (Eyy - my^2) + C2
//   S = A1 A2 / (B1 B2),  the result: the mean of S over N C H W (or over C H W per image).
// With a gradient wanted the forward also writes three maps of dS/d(moment) per pixel (no division by A1 or A2):
//   a = dS/dmx = 2 my (A2 - A1) / (B1 B2) - S 2 mx (1/B1 - 1/B2),  b = dS/dExx = -S / B2,  c = dS/dExy = 2 A1 / (B1 B2)
// and, w being symmetric and the maps zero outside the image, the backward is three more blurs:
//   dL/dx = (g / M) (w*a + 2 x (w*b) + y (w*c)),  g the upstream gradient read from device memory, M the averaged count.
//
// Tiling: one 256-lane workgroup per 32 x 16 output tile of one plane.  The 42 x 26 haloed inputs are staged in LDS
// (zero outside the image), a horizontal pass writes the 11-tap row sums of every moment for the 26 rows (4 outputs per lane from a
// 14-value register window), a vertical pass turns them into the 32 x 16 moments (2 rows per lane).  Row pitches: 45 floats for the
// staged inputs (lanes 8 apart in a row group read rows 45 floats apart: all 32 banks distinct), 33 for the row sums (the same for
// the 4-wide writes); the vertical reads are 32 consecutive floats per half-wave.
//
// Reduction order, fixed: the workgroup's S values are summed per wave by xor-shuffles, the four wave sums in wave order, one partial
// per workgroup in the caller's scratch; ssim_mean_kernel adds the partials of one output in fp64 over a fixed lane assignment and tree.
// No atomics anywhere: two calls on the same inputs give the same bits, forward and backward.
// Defines the entry points gsr_ssim_scratch_bytes, gsr_ssim_forward and gsr_ssim_backward.
#include "gsr_internal.h"
#include "gsr_wave.h"

namespace gsr {
namespace {

constexpr int kTileW = 32, kTileH = 16, kRadius = 5, kTaps = 2 * kRadius + 1;
constexpr int kHaloW = kTileW + 2 * kRadius;      // 42
constexpr int kHaloH = kTileH + 2 * kRadius;      // 26
constexpr int kInPitch = 45;                      // staged inputs (see the file comment)
constexpr int kSumPitch = kTileW + 1;             // row sums
constexpr int kStrip = 4;                         // horizontal pass: outputs per lane along a row
constexpr int kRowItems = kHaloH * (kTileW / kStrip);   // 208 lanes busy in the horizontal pass
constexpr int kThreads = 256;
constexpr uint32_t kMaxGrid = 1u << 16;           // workgroups launched; more tiles are walked grid-stride
static_assert(kTileW * kTileH == 2 * kThreads, "the vertical pass gives every lane two outputs");
static_assert(kRowItems <= kThreads, "one horizontal item per lane");
constexpr int kSsimTaps = kTaps;                  // gsr.h: window11
constexpr float kSsimC1 = (float)(0.01 * 0.01);   // the reference's Python constants, rounded to fp32 as its fp32 tensor ops do
constexpr float kSsimC2 = (float)(0.03 * 0.03);
struct SsimWindow {   // the separable window, passed by value
    float w[kSsimTaps];
};
struct SsimShape {
    int n, c, h, w;
    int tiles_x;
    uint32_t tiles_per_plane, blocks;   // blocks = n c tiles_per_plane (one partial sum each)
};

struct TileAt {
    int x0, y0;      // first output pixel of the tile
    size_t plane;    // element offset of the plane
};

__device__ __forceinline__ TileAt tile_at(const SsimShape& s, uint32_t b) {
    const uint32_t plane = b / s.tiles_per_plane, t = b % s.tiles_per_plane;
    return {(int)(t % s.tiles_x) * kTileW, (int)(t / s.tiles_x) * kTileH, (size_t)plane * s.h * s.w};
}

// `count` planes of one tile's haloed input -> LDS, zero outside the image
template <int count>
__device__ __forceinline__ void stage(const SsimShape& s, const TileAt& at, const float* const (&src)[count],
                                      float (&dst)[count][kHaloH][kInPitch]) {
    for (int i = threadIdx.x; i < kHaloH * kHaloW; i += kThreads) {
        const int r = i / kHaloW, c = i % kHaloW;
        const int gy = at.y0 - kRadius + r, gx = at.x0 - kRadius + c;
        const bool in = gy >= 0 && gy < s.h && gx >= 0 && gx < s.w;
        const size_t off = at.plane + (size_t)(in ? gy : 0) * s.w + (in ? gx : 0);
#pragma unroll
        for (int k = 0; k < count; ++k) dst[k][r][c] = in ? src[k][off] : 0.0f;
    }
}

// the vertical pass of one moment for the lane's two outputs (rows r0, r0 + 1 of column col)
__device__ __forceinline__ void vertical(const float (&rows)[kHaloH][kSumPitch], int r0, int col, const SsimWindow& win, float& o0,
                                         float& o1) {
    o0 = 0.0f;
    o1 = 0.0f;
#pragma unroll
    for (int j = 0; j <= kTaps; ++j) {
        const float v = rows[r0 + j][col];
        if (j < kTaps) o0 += win.w[j] * v;
        if (j > 0) o1 += win.w[j - 1] * v;
    }
}

__global__ __launch_bounds__(kThreads) void ssim_forward_kernel(SsimShape s, SsimWindow win, const float* __restrict__ x,
                                                                const float* __restrict__ y, float* __restrict__ partials,
                                                                float* __restrict__ coef) {
    __shared__ float in[2][kHaloH][kInPitch];
    __shared__ float rows[5][kHaloH][kSumPitch];
    __shared__ float wave_sums[kThreads / 64];
    const int t = threadIdx.x;
    const size_t total = (size_t)s.n * s.c * s.h * s.w;
    for (uint32_t b = blockIdx.x; b < s.blocks; b += gridDim.x) {
        const TileAt at = tile_at(s, b);
        const float* const src[2] = {x, y};
        stage<2>(s, at, src, in);
        __syncthreads();
        if (t < kRowItems) {   // horizontal: row r, outputs c0 .. c0 + 3
            const int r = t / (kTileW / kStrip), c0 = (t % (kTileW / kStrip)) * kStrip;
            float vx[kStrip + kTaps - 1], vy[kStrip + kTaps - 1];
#pragma unroll
            for (int k = 0; k < kStrip + kTaps - 1; ++k) {
                vx[k] = in[0][r][c0 + k];
                vy[k] = in[1][r][c0 + k];
            }
            float acc[5][kStrip] = {};
#pragma unroll
            for (int k = 0; k < kTaps; ++k) {
                const float wk = win.w[k];
#pragma unroll
                for (int q = 0; q < kStrip; ++q) {
                    const float a = vx[q + k], b2 = vy[q + k];
                    acc[0][q] += wk * a;
                    acc[1][q] += wk * b2;
                    acc[2][q] += wk * (a * a);
                    acc[3][q] += wk * (b2 * b2);
                    acc[4][q] += wk * (a * b2);
                }
            }
#pragma unroll
            for (int m = 0; m < 5; ++m)
#pragma unroll
                for (int q = 0; q < kStrip; ++q) rows[m][r][c0 + q] = acc[m][q];
        }
        __syncthreads();
        const int col = t % kTileW, r0 = (t / kTileW) * 2;
        float mom[5][2];
#pragma unroll
        for (int m = 0; m < 5; ++m) vertical(rows[m], r0, col, win, mom[m][0], mom[m][1]);
        float sum = 0.0f;
        const int gx = at.x0 + col;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int gy = at.y0 + r0 + i;
            if (gx >= s.w || gy >= s.h) continue;
            const float mx = mom[0][i], my = mom[1][i], exx = mom[2][i], eyy = mom[3][i], exy = mom[4][i];
            const float mx2 = mx * mx, my2 = my * my, mxy = mx * my;
            const float A1 = 2.0f * mxy + kSsimC1, A2 = 2.0f * (exy - mxy) + kSsimC2;
            const float B1 = (mx2 + my2) + kSsimC1, B2 = ((exx - mx2) + (eyy - my2)) + kSsimC2;
            const float D = B1 * B2;
            const float S = (A1 * A2) / D;
            sum += S;
            if (coef) {
                const size_t off = at.plane + (size_t)gy * s.w + gx;
                coef[off] = (2.0f * my * (A2 - A1)) / D - (S * (2.0f * mx)) * (1.0f / B1 - 1.0f / B2);
                coef[total + off] = -S / B2;
                coef[2 * total + off] = (2.0f * A1) / D;
            }
        }
        sum = wave_fold(sum, [](float a, float b) { return a + b; });   // the butterfly pairing: part of the fixed order
        if ((t & 63) == 0) wave_sums[t >> 6] = sum;
        __syncthreads();
        if (t == 0) partials[b] = ((wave_sums[0] + wave_sums[1]) + wave_sums[2]) + wave_sums[3];
        __syncthreads();   // the next tile overwrites the LDS
    }
}

// one workgroup per output: the mean of `per_out` consecutive partials, added in fp64 in a fixed order
__global__ __launch_bounds__(kThreads) void ssim_mean_kernel(const float* __restrict__ partials, uint32_t per_out, double count,
                                                             float* __restrict__ out) {
    __shared__ double acc[kThreads];
    const float* p = partials + (size_t)blockIdx.x * per_out;
    double v = 0.0;
    for (uint32_t i = threadIdx.x; i < per_out; i += kThreads) v += (double)p[i];
    acc[threadIdx.x] = v;
    __syncthreads();
    for (int k = kThreads / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) acc[threadIdx.x] += acc[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(acc[0] / count);
}

__global__ __launch_bounds__(kThreads) void ssim_backward_kernel(SsimShape s, SsimWindow win, const float* __restrict__ x,
                                                                 const float* __restrict__ y, const float* __restrict__ coef,
                                                                 const float* __restrict__ grad_out, int per_image, double count,
                                                                 float* __restrict__ grad_x) {
    __shared__ float in[3][kHaloH][kInPitch];
    __shared__ float rows[3][kHaloH][kSumPitch];
    const int t = threadIdx.x;
    const size_t total = (size_t)s.n * s.c * s.h * s.w;
    for (uint32_t b = blockIdx.x; b < s.blocks; b += gridDim.x) {
        const TileAt at = tile_at(s, b);
        const float* const src[3] = {coef, coef + total, coef + 2 * total};
        stage<3>(s, at, src, in);
        __syncthreads();
        if (t < kRowItems) {
            const int r = t / (kTileW / kStrip), c0 = (t % (kTileW / kStrip)) * kStrip;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                float v[kStrip + kTaps - 1];
#pragma unroll
                for (int k = 0; k < kStrip + kTaps - 1; ++k) v[k] = in[m][r][c0 + k];
                float acc[kStrip] = {};
#pragma unroll
                for (int k = 0; k < kTaps; ++k)
#pragma unroll
                    for (int q = 0; q < kStrip; ++q) acc[q] += win.w[k] * v[q + k];
#pragma unroll
                for (int q = 0; q < kStrip; ++q) rows[m][r][c0 + q] = acc[q];
            }
        }
        __syncthreads();
        const int col = t % kTileW, r0 = (t / kTileW) * 2;
        float blur[3][2];
#pragma unroll
        for (int m = 0; m < 3; ++m) vertical(rows[m], r0, col, win, blur[m][0], blur[m][1]);
        const uint32_t plane = b / s.tiles_per_plane;
        const float scale = (float)((double)grad_out[per_image ? plane / (uint32_t)s.c : 0u] / count);
        const int gx = at.x0 + col;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int gy = at.y0 + r0 + i;
            if (gx >= s.w || gy >= s.h) continue;
            const size_t off = at.plane + (size_t)gy * s.w + gx;
            grad_x[off] = scale * ((blur[0][i] + (2.0f * x[off]) * blur[1][i]) + y[off] * blur[2][i]);
        }
        __syncthreads();
    }
}

SsimShape ssim_shape(int n, int c, int h, int w) {   // n c h w < 2^31
    SsimShape s{n, c, h, w, (w + kTileW - 1) / kTileW, 0, 0};
    s.tiles_per_plane = (uint32_t)s.tiles_x * (uint32_t)((h + kTileH - 1) / kTileH);
    s.blocks = (uint32_t)n * (uint32_t)c * s.tiles_per_plane;
    return s;
}

hipError_t launch_ssim_forward(const SsimShape& s, const SsimWindow& win, const float* x, const float* y, int per_image, float* out,
                               float* coef, float* partials, hipStream_t stream) {
    hipLaunchKernelGGL(ssim_forward_kernel, dim3(min(s.blocks, kMaxGrid)), dim3(kThreads), 0, stream, s, win, x, y, partials, coef);
    const uint32_t outs = per_image ? (uint32_t)s.n : 1u;
    const double count = (double)s.c * s.h * s.w * (per_image ? 1 : s.n);
    hipLaunchKernelGGL(ssim_mean_kernel, dim3(outs), dim3(kThreads), 0, stream, (const float*)partials, s.blocks / outs, count, out);
    return hipGetLastError();
}

hipError_t launch_ssim_backward(const SsimShape& s, const SsimWindow& win, const float* x, const float* y, const float* coef,
                                int per_image, const float* grad_out, float* grad_x, hipStream_t stream) {
    const double count = (double)s.c * s.h * s.w * (per_image ? 1 : s.n);
    hipLaunchKernelGGL(ssim_backward_kernel, dim3(min(s.blocks, kMaxGrid)), dim3(kThreads), 0, stream, s, win, x, y, coef, grad_out,
                       per_image, count, grad_x);
    return hipGetLastError();
}

}  // namespace
}  // namespace gsr

using gsr::aligned4;
using gsr::fail;

namespace {
// the sizes gsr_ssim_* accept: every dimension > 0, n c h w < 2^31
bool ssim_size_ok(int n, int c, int h, int w) {
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return false;
    const int64_t nc = (int64_t)n * c, nch = nc * h;
    return nc < (int64_t(1) << 31) && nch < (int64_t(1) << 31) && nch * w < (int64_t(1) << 31);
}
gsr::SsimWindow ssim_window(const float* window11) {
    gsr::SsimWindow win;
    for (int k = 0; k < gsr::kSsimTaps; ++k) win.w[k] = window11[k];
    return win;
}
}  // namespace


extern "C" {

size_t gsr_ssim_scratch_bytes(int n, int c, int h, int w) {
    return ssim_size_ok(n, c, h, w) ? (size_t)gsr::ssim_shape(n, c, h, w).blocks * sizeof(float) : 0;
}

int gsr_ssim_forward(int n, int c, int h, int w, const float* x, const float* y, const float* window11, int per_image, float* out,
                     float* coef_or_null, void* scratch, size_t scratch_bytes, void* stream_) {
    if (!ssim_size_ok(n, c, h, w)) return fail(GSR_ERR_INVALID_ARG, "gsr_ssim_forward: bad size %d x %d x %d x %d (each > 0, product < 2^31)", n, c, h, w);
    if (!x || !y || !window11 || !out || !scratch) return fail(GSR_ERR_INVALID_ARG, "gsr_ssim_forward: null pointer");
    if (!aligned4(x) || !aligned4(y) || !aligned4(out) || !aligned4(coef_or_null) || !aligned4(scratch))
        return fail(GSR_ERR_INVALID_ARG, "gsr_ssim_forward: misaligned pointer (4 bytes)");
    if (scratch_bytes < gsr_ssim_scratch_bytes(n, c, h, w))
        return fail(GSR_ERR_INVALID_ARG, "gsr_ssim_forward: scratch too small (%zu of %zu bytes)", scratch_bytes, gsr_ssim_scratch_bytes(n, c, h, w));
    GSR_HIP(gsr::launch_ssim_forward(gsr::ssim_shape(n, c, h, w), ssim_window(window11), x, y, per_image ? 1 : 0, out, coef_or_null,
                                     (float*)scratch, (hipStream_t)stream_));
    return GSR_OK;
}

int gsr_ssim_backward(int n, int c, int h, int w, const float* x, const float* y, const float* coef, const float* window11, int per_image,
                      const float* grad_out, float* grad_x, void* stream_) {
    if (!ssim_size_ok(n, c, h, w)) return fail(GSR_ERR_INVALID_ARG, "gsr_ssim_backward: bad size %d x %d x %d x %d (each > 0, product < 2^31)", n, c, h, w);
    if (!x || !y || !coef || !window11 || !grad_out || !grad_x) return fail(GSR_ERR_INVALID_ARG, "gsr_ssim_backward: null pointer");
    if (!aligned4(x) || !aligned4(y) || !aligned4(coef) || !aligned4(grad_out) || !aligned4(grad_x))
        return fail(GSR_ERR_INVALID_ARG, "gsr_ssim_backward: misaligned pointer (4 bytes)");
    GSR_HIP(gsr::launch_ssim_backward(gsr::ssim_shape(n, c, h, w), ssim_window(window11), x, y, coef, per_image ? 1 : 0, grad_out, grad_x,
                                      (hipStream_t)stream_));
    return GSR_OK;
}

}  // extern "C"
