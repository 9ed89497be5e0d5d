// gsr_panorama.hip -- a cube map to an equirectangular panorama on the GPU (include/gsr.h: gsr_cube_to_equirect).
//
// The reference turns the six faces of a panorama (render_panorama.py:100-145) into a 2:1 equirectangular image on the host:
// c2e(cube, h, w, mode='bilinear', cube_format='dict') (utils/py360_utils.py:7-65), which pads every face with two rows and
// two columns taken from its neighbours (sample_cubefaces, :201-239) and samples the padded cube with
// scipy.ndimage.map_coordinates(order=1).  Here one lane makes one output pixel, all channels:
//
//   * face type: the column roll of 3W/8 and the up / down ceiling per column.  The ceilings (W/4 integers) and the per-column
//     u / per-row v angles (fp32 linspace) come from the host, computed there in numpy's own arithmetic (autovfx_amd/panorama.py),
//     so the face type is the reference's bit for bit;
//   * face coordinates in the reference's fp32 operation order (subtract, tan, cos, divide: the build has -ffp-contract=off and
//     no fast math), renormalised in fp64 as numpy does: (clip(c, -0.5, 0.5) + 0.5) * S -- pixel i's centre sits at coordinate
//     i, so the coordinates run 0 .. S and the taps at S + 1 land in the padding;
//   * the padding is not materialised: pad_source() maps a (face, row, col) of the (S+2)^2 padded face to the texel of the six
//     faces the padded array holds there (or to one of the zeros the reference leaves in the corners of the up / down faces);
//   * bilinear weights as map_coordinates forms them (w0 = 1 - t, w1 = 1 - w0) and the taps summed in its order, in fp64.
//
// Optional outputs: the float panorama [H,W,C]; the LDR bytes the reference saves, uint8(clip(x * 255, 0, 255)) of the float
// value (truncation, not save_image's + 0.5); and the radial-distance panorama: the same taps and weights over
// depth * sqrt(1 + (2 cx)^2 + (2 cy)^2), evaluated at each tap's SOURCE texel ("Panoramas").
// Defines the entry point gsr_cube_to_equirect.
#include "gsr_internal.h"

#include <cmath>

namespace gsr {
namespace {

// The six faces of a cube map, in the reference's dict order (front, right, back, left, up, down): planar [C,S,S] colour or [S,S] depth.
struct CubeFacePointers { const float* p[6]; };

// the reference's dict order (cube_dict2h): 0 front, 1 right, 2 back, 3 left, 4 up, 5 down
struct Texel { int face, row, col; };   // face < 0: a zero of the padding

// (face k, row r, col c) of the padded face, 0 <= r, c < S + 2 -> the texel of the six S x S faces the padded array holds there.
// Rows are padded first (rows S, S + 1), then columns (cols S, S + 1) from the ROW-PADDED neighbours, which is why a column pad
// may resolve to a row pad of its neighbour.  Up / down column pads are defined on rows 1 .. S only, and read row 0 (up) or
// row S -- the first row pad -- (down) of the right and left faces.
__device__ inline Texel pad_source(int k, int r, int c, int S) {
    const int m = S - 1;
    if (c >= S) {
        const bool first = c == S;
        if (k < 4) {                      // first pad column: the next side face's column 0; second: the previous one's last column
            k = first ? (k + 1) & 3 : (k + 3) & 3;
            c = first ? 0 : m;
        } else {
            if (r == 0 || r == S + 1) return {-1, 0, 0};
            if (k == 4) c = first ? S - r : r - 1;
            else        c = first ? r - 1 : S - r;
            r = k == 4 ? 0 : S;
            k = first ? 1 : 3;
        }
    }
    if (r >= S) {
        const bool first = r == S;
        switch (k) {
        case 0:  return first ? Texel{5, 0, c} : Texel{4, m, c};
        case 1:  return first ? Texel{5, c, m} : Texel{4, m - c, m};
        case 2:  return first ? Texel{5, m, m - c} : Texel{4, 0, m - c};
        case 3:  return first ? Texel{5, m - c, 0} : Texel{4, c, 0};
        case 4:  return first ? Texel{0, 0, c} : Texel{2, 0, m - c};
        default: return first ? Texel{2, m, m - c} : Texel{0, m, c};
        }
    }
    return {k, r, c};
}

// np.pi * i / 2 as numpy rounds it to fp32 before the fp32 subtraction (a Python float meets a float32 array)
__constant__ float kSideShift[4] = {0.0f, (float)(M_PI * 1 / 2), (float)(M_PI * 2 / 2), (float)(M_PI * 3 / 2)};
constexpr float kHalfPi = (float)(M_PI / 2);

// the radial-distance factor of a texel: its pixel centre lies at (2 cx, 2 cy, 1) in the face camera's frame (90 degree field of
// view; cx = (col + 0.5) / S - 0.5), so distance = depth * |(2 cx, 2 cy, 1)|
__device__ inline float radial_factor(int row, int col, int S) {
    const float x = (float)(2 * col + 1 - S) / (float)S, y = (float)(2 * row + 1 - S) / (float)S;
    return sqrtf(1.0f + x * x + y * y);
}

__global__ void __launch_bounds__(256) cube_to_equirect_kernel(CubeFacePointers faces, CubeFacePointers depth, int S, int C,
                                                               const float* __restrict__ grid_u, const float* __restrict__ grid_v,
                                                               const int* __restrict__ grid_ceil, int H, int W, float* __restrict__ out,
                                                               uint8_t* __restrict__ out_u8, float* __restrict__ out_depth) {
    const int col = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (col >= W) return;
    // face type (equirect_facetype): the side faces in quarters of the width, rolled right by 3W/8, and the ceilings
    const int q = W / 4, src = (col + W - 3 * (W / 8)) % W, ceil_j = grid_ceil[src % q];
    int tp = src / q;
    if (row < ceil_j) tp = 4;
    if (H - 1 - row < ceil_j) tp = 5;      // the flipped mask is applied second: it wins where both hold

    const float u = grid_u[col], v = grid_v[row];
    float cx, cy;
    if (tp < 4) {
        const float a = u - kSideShift[tp];
        cx = 0.5f * tanf(a);
        cy = (-0.5f * tanf(v)) / cosf(a);
    } else {
        const float c = 0.5f * tanf(kHalfPi - (tp == 4 ? v : fabsf(v)));
        cx = c * sinf(u);
        cy = tp == 4 ? c * cosf(u) : -c * cosf(u);
    }
    const double x = (fmin(fmax((double)cx, -0.5), 0.5) + 0.5) * S;
    const double y = (fmin(fmax((double)cy, -0.5), 0.5) + 0.5) * S;
    const int x0 = (int)floor(x), y0 = (int)floor(y);    // 0 .. S: the taps x0, x0 + 1 stay inside the padded S + 2
    const double wx0 = 1.0 - (x - x0), wy0 = 1.0 - (y - y0);
    const double wx[2] = {wx0, 1.0 - wx0}, wy[2] = {wy0, 1.0 - wy0};

    Texel tap[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) tap[t] = pad_source(tp, y0 + (t >> 1), x0 + (t & 1), S);

    const size_t plane = (size_t)S * S, pix = (size_t)row * W + col;
    for (int ch = 0; ch < C; ++ch) {
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double value = tap[t].face < 0 ? 0.0 : (double)faces.p[tap[t].face][ch * plane + (size_t)tap[t].row * S + tap[t].col];
            acc += value * wy[t >> 1] * wx[t & 1];
        }
        const float g = (float)acc;
        if (out) out[pix * C + ch] = g;
        if (out_u8) out_u8[pix * C + ch] = (uint8_t)fminf(fmaxf(g * 255.0f, 0.0f), 255.0f);
    }
    if (out_depth) {
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            double value = 0.0;
            if (tap[t].face >= 0)
                value = (double)(depth.p[tap[t].face][(size_t)tap[t].row * S + tap[t].col] * radial_factor(tap[t].row, tap[t].col, S));
            acc += value * wy[t >> 1] * wx[t & 1];
        }
        out_depth[pix] = (float)acc;
    }
}

// c2e(..., mode='bilinear') of the reference (gsr.h: gsr_cube_to_equirect); grid_u [W], grid_v [H], grid_ceil [W/4] as the host computes
// them; any of out [H,W,C] / out_u8 [H,W,C] / out_depth [H,W] may be null (depth.p is read only when out_depth is set).
hipError_t launch_cube_to_equirect(const CubeFacePointers& faces, const CubeFacePointers& depth, int S, int C, const float* grid_u,
                                   const float* grid_v, const int* grid_ceil, int H, int W, float* out, uint8_t* out_u8, float* out_depth,
                                   hipStream_t stream) {
    hipLaunchKernelGGL(cube_to_equirect_kernel, dim3((W + 255) / 256, H), dim3(256), 0, stream, faces, depth, S, C, grid_u, grid_v,
                       grid_ceil, H, W, out, out_u8, out_depth);
    return hipGetLastError();
}

}  // namespace
}  // namespace gsr

using gsr::fail;

extern "C" {

int gsr_cube_to_equirect(const float* const* faces, int face_size, int channels, const float* const* depth_faces, const float* grid_u,
                         const float* grid_v, const int32_t* grid_ceil, int height, int width, float* out, uint8_t* out_u8, float* out_depth,
                         void* stream_) {
    if (width <= 0 || width % 8 != 0) return fail(GSR_ERR_INVALID_ARG, "gsr_cube_to_equirect: the width (%d) must be a positive multiple of 8", width);
    if (height < 2 || height > 65535) return fail(GSR_ERR_INVALID_ARG, "gsr_cube_to_equirect: bad height %d (2 .. 65535)", height);
    if (face_size < 2 || face_size > 32768) return fail(GSR_ERR_INVALID_ARG, "gsr_cube_to_equirect: bad face size %d (2 .. 32768)", face_size);
    if (channels < 1 || channels > 4) return fail(GSR_ERR_INVALID_ARG, "gsr_cube_to_equirect: %d channels (1 .. 4)", channels);
    if (!faces || !grid_u || !grid_v || !grid_ceil || (!out && !out_u8 && !out_depth) || (out_depth && !depth_faces))
        return fail(GSR_ERR_INVALID_ARG, "null pointer");
    gsr::CubeFacePointers f = {}, d = {};
    for (int k = 0; k < 6; ++k) {
        if (!(f.p[k] = faces[k])) return fail(GSR_ERR_INVALID_ARG, "gsr_cube_to_equirect: face %d is null", k);
        if (out_depth && !(d.p[k] = depth_faces[k])) return fail(GSR_ERR_INVALID_ARG, "gsr_cube_to_equirect: depth face %d is null", k);
    }
    GSR_HIP(gsr::launch_cube_to_equirect(f, d, face_size, channels, grid_u, grid_v, grid_ceil, height, width, out, out_u8, out_depth,
                                         (hipStream_t)stream_));
    return GSR_OK;
}


}  // extern "C"
