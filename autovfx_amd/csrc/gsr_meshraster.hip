// gsr_meshraster.hip -- a z-buffer over triangle meshes: the forward of pytorch3d's rasterize_meshes at blur_radius == 0
// (include/gsr.h: gsr_mesh_raster_count, gsr_mesh_raster; the contract is the module docstring of autovfx_amd/meshraster.py and
// DESIGN.md 7i).  Four kernels and one host read:
//   count   one lane per face: the culls, the mesh the face belongs to, the rectangle of 16x16 tiles its bounding box touches (padded
//           by a pixel: the exact test is the blend's), one integer atomic add per touched tile
//   scan    one workgroup: exclusive prefix of the per-tile counts, the counts cleared for their second use, the pair total
//           -> the host reads the pair total (the only host read of a call) and sizes the pair list
//   fill    one lane per face again: a slot in each touched tile's list from an atomic cursor (the raster kernel clears it behind the
//           fill, so a plan serves any number of raster calls); the order inside a list is whatever the atomics gave, and no result
//           depends on it because the blend orders by (depth, face index)
//   raster  one 256-lane workgroup per tile, one pixel per lane: the list goes through LDS in chunks of kMeshChunk faces, set up once
//           per chunk (every lane reads the same LDS address: a broadcast); the K nearest (depth, face) pairs sit in registers; the
//           barycentrics and the distance are computed again from face_verts when the pixel is written (the same operations, so the
//           same bits), which keeps the slots at two registers each.
// A rectangle of more than kWaveRect tiles is walked by the whole wave, not by the lane that owns the face.
// fp32 throughout, -ffp-contract=off, IEEE division, no transcendental: the numpy restatement computes the same bits.
#include "gsr_internal.h"
#include "gsr_wave.h"

#include <limits.h>
#include <math.h>

namespace gsr {
namespace {

constexpr int kMeshThreads = 256;
constexpr int kMeshChunk = 256;          // faces set up in LDS at a time (one per lane); tests/test_meshraster_gpu.py: CHUNK copies it for
                                         // its list of three chunks in one tile -- change both together
constexpr uint32_t kWaveRect = 64;       // rectangles of more tiles than this are walked by the wave
constexpr int kScanPerLane = 16;         // the scan's workgroup covers 256 * 16 tiles per round
constexpr float kMeshEps = 1e-8f;
constexpr float kBaryClipEps = 1e-5f;
constexpr uint32_t kNoMesh = 0xFFFFFFFFu;
constexpr int kMeshMaxK = 16;
constexpr int kMeshMaxSide = 16384;

struct MeshPlanHeader {
    unsigned long long pair_total;
    uint32_t pad[62];
};
static_assert(sizeof(MeshPlanHeader) == 256, "the arrays behind the header start 256-byte aligned");

// The plan scratch: what the count step leaves for the raster step.
struct MeshPlan {
    MeshPlanHeader* header;
    uint2* rects;        // [F] tile rectangle: x0 | x1 << 16, y0 | y1 << 16 (inclusive)
    uint32_t* mesh;      // [F] the mesh (= image) of the face, kNoMesh: culled, in no mesh, or off the image
    uint32_t* counts;    // [N * T] faces per tile, then (cleared by the scan, and again by the raster kernel) the fill's cursors
    uint32_t* offsets;   // [N * T] where each tile's list starts in the pair list
    size_t bytes;
};

inline size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }

MeshPlan plan_layout(int64_t F, int64_t tiles, void* base) {
    char* p = static_cast<char*>(base);
    MeshPlan L;
    size_t at = 0;
    L.header = reinterpret_cast<MeshPlanHeader*>(p + at), at += sizeof(MeshPlanHeader);
    L.rects = reinterpret_cast<uint2*>(p + at), at += round256((size_t)F * sizeof(uint2));
    L.mesh = reinterpret_cast<uint32_t*>(p + at), at += round256((size_t)F * sizeof(uint32_t));
    L.counts = reinterpret_cast<uint32_t*>(p + at), at += round256((size_t)tiles * sizeof(uint32_t));
    L.offsets = reinterpret_cast<uint32_t*>(p + at), at += round256((size_t)tiles * sizeof(uint32_t));
    L.bytes = at;
    return L;
}

// ---- the contract's arithmetic: every function below is restated operation by operation in autovfx_amd/meshraster.py ----------------

__device__ inline float edge_fn(float px, float py, float ax, float ay, float bx, float by) {
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

// Centre of pixel index i along an axis of S1 pixels whose other axis has S2 (pytorch3d's NonSquarePixToNdc).
__device__ inline float pix_to_ndc(int i, int S1, int S2) {
    const float range = S1 > S2 ? (2.0f * (float)S1) / (float)S2 : 2.0f;
    const float offset = range / 2.0f;
    return -offset + (range * (float)i + offset) / (float)S1;
}

struct FaceSetup {
    float x0, y0, x1, y1, x2, y2;
    float z0, z1, z2;
    float denom;                       // edge(v2, v0, v1) + eps
    float xmin, xmax, ymin, ymax;
    int face;
    int nbr;
};
static_assert(sizeof(FaceSetup) == 64, "four 16-byte LDS reads per face");

__device__ inline void load_face(const float* __restrict__ face_verts, int f, FaceSetup& s) {
    const float* v = face_verts + (size_t)f * 9;
    s.x0 = v[0], s.y0 = v[1], s.z0 = v[2];
    s.x1 = v[3], s.y1 = v[4], s.z1 = v[5];
    s.x2 = v[6], s.y2 = v[7], s.z2 = v[8];
    s.denom = edge_fn(s.x2, s.y2, s.x0, s.y0, s.x1, s.y1) + kMeshEps;
    s.xmin = fminf(s.x0, fminf(s.x1, s.x2)), s.xmax = fmaxf(s.x0, fmaxf(s.x1, s.x2));
    s.ymin = fminf(s.y0, fminf(s.y1, s.y2)), s.ymax = fmaxf(s.y0, fmaxf(s.y1, s.y2));
    s.face = f;
    s.nbr = -1;
}

// The per-face skips that do not depend on the pixel.
__device__ inline bool face_culled(const FaceSetup& s, int cull_backfaces) {
    const float zmax = fmaxf(s.z0, fmaxf(s.z1, s.z2));
    const float area = edge_fn(s.x0, s.y0, s.x1, s.y1, s.x2, s.y2);
    return zmax < kMeshEps || fabsf(area) <= kMeshEps || (cull_backfaces && area < 0.0f);
}

// Is the face kept at (px, py)?  Then pz and the barycentrics it is listed with.
__device__ inline bool face_at_pixel(const FaceSetup& s, float px, float py, int perspective, int clip, float& pz, float& b0, float& b1,
                                     float& b2) {
    if (px < s.xmin || px > s.xmax || py < s.ymin || py > s.ymax) return false;
    const float w0 = edge_fn(px, py, s.x1, s.y1, s.x2, s.y2) / s.denom;
    const float w1 = edge_fn(px, py, s.x2, s.y2, s.x0, s.y0) / s.denom;
    const float w2 = edge_fn(px, py, s.x0, s.y0, s.x1, s.y1) / s.denom;
    if (!(w0 > 0.0f && w1 > 0.0f && w2 > 0.0f)) return false;
    b0 = w0, b1 = w1, b2 = w2;
    if (perspective) {
        const float t0 = (w0 * s.z1) * s.z2, t1 = (s.z0 * w1) * s.z2, t2 = (s.z0 * s.z1) * w2;
        const float d = fmaxf((t0 + t1) + t2, kMeshEps);
        b0 = t0 / d, b1 = t1 / d, b2 = t2 / d;
    }
    if (clip) {
        const float c0 = fmaxf(0.0f, fminf(1.0f, b0)), c1 = fmaxf(0.0f, fminf(1.0f, b1)), c2 = fmaxf(0.0f, fminf(1.0f, b2));
        const float d = fmaxf((c0 + c1) + c2, kBaryClipEps);
        b0 = c0 / d, b1 = c1 / d, b2 = c2 / d;
    }
    pz = (b0 * s.z0 + b1 * s.z1) + b2 * s.z2;
    return !(pz < 0.0f);
}

__device__ inline float segment_dist2(float px, float py, float ax, float ay, float bx, float by) {
    const float dx = bx - ax, dy = by - ay;
    const float l2 = dx * dx + dy * dy;
    if (l2 <= kMeshEps) {
        const float ex = px - bx, ey = py - by;
        return ex * ex + ey * ey;
    }
    const float t = (dx * (px - ax) + dy * (py - ay)) / l2;
    const float tt = fminf(fmaxf(t, 0.0f), 1.0f);
    const float qx = ax + tt * dx, qy = ay + tt * dy;
    const float ex = px - qx, ey = py - qy;
    return ex * ex + ey * ey;
}

__device__ inline float triangle_dist2(const FaceSetup& s, float px, float py) {
    const float e01 = segment_dist2(px, py, s.x0, s.y0, s.x1, s.y1);
    const float e02 = segment_dist2(px, py, s.x0, s.y0, s.x2, s.y2);
    const float e12 = segment_dist2(px, py, s.x1, s.y1, s.x2, s.y2);
    return fminf(e01, fminf(e02, e12));
}

// ---- binning ------------------------------------------------------------------------------------------------------------------------

// Pixel indices [first, last] along an axis whose centres can lie in [lo, hi], padded by one pixel on both sides (the inverse of
// pix_to_ndc is only used here, where a pixel too many costs a list entry and nothing else).  False: none on the image.
__device__ inline bool pixel_span(float lo, float hi, int S1, int S2, int& first, int& last) {
    const float range = S1 > S2 ? (2.0f * (float)S1) / (float)S2 : 2.0f;
    const float offset = range / 2.0f;
    const float scale = (float)S1 / range;
    const float a = floorf((lo + offset) * scale - 0.5f) - 1.0f;
    const float b = ceilf((hi + offset) * scale - 0.5f) + 1.0f;
    if (!(b >= 0.0f) || !(a <= (float)(S1 - 1))) return false;   // (a NaN bound: no pixel)
    first = (int)fmaxf(a, 0.0f);
    last = (int)fminf(b, (float)(S1 - 1));
    return first <= last;
}

struct MeshBinArgs {
    int F, N, H, W;
    int tiles_x, tiles_y;
    int cull_backfaces;
    const float* face_verts;
    const long long* first_idx;
    const long long* num_faces;
    uint2* rects;
    uint32_t* mesh;
    uint32_t* counts;
    const uint32_t* offsets;
    uint32_t* pairs;
    uint32_t pair_total;
};

// fn(tile, face) for every tile of the lane's rectangle; all 64 lanes of the wave must arrive (live = false: nothing of its own).
template <class Fn>
__device__ inline void for_each_tile(bool live, uint32_t base, uint32_t tiles_x, uint2 rect, uint32_t face, Fn fn) {
    const uint32_t x0 = rect.x & 0xFFFFu, y0 = rect.y & 0xFFFFu;
    const uint32_t w = live ? (rect.x >> 16) - x0 + 1u : 0u, h = live ? (rect.y >> 16) - y0 + 1u : 0u;
    const uint32_t n = w * h;
    const bool big = n > kWaveRect;
    if (!big)
        for (uint32_t i = 0; i < n; ++i) fn(base + (y0 + i / w) * tiles_x + x0 + i % w, face);
    unsigned long long todo = __ballot(big);
    const uint32_t lane = threadIdx.x & 63u;
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t bw = (uint32_t)__shfl((int)w, src), bn = (uint32_t)__shfl((int)n, src);
        const uint32_t bx0 = (uint32_t)__shfl((int)x0, src), by0 = (uint32_t)__shfl((int)y0, src);
        const uint32_t bbase = (uint32_t)__shfl((int)base, src), bface = (uint32_t)__shfl((int)face, src);
        for (uint32_t i = lane; i < bn; i += 64u) fn(bbase + (by0 + i / bw) * tiles_x + bx0 + i % bw, bface);
    }
}

__global__ __launch_bounds__(kMeshThreads) void mesh_count_kernel(const MeshBinArgs a) {
    const long long fl = (long long)blockIdx.x * kMeshThreads + threadIdx.x;
    const bool in_range = fl < a.F;
    const int f = in_range ? (int)fl : 0;
    uint32_t mesh = kNoMesh;
    uint2 rect = make_uint2(0u, 0u);
    if (in_range) {
        FaceSetup s;
        load_face(a.face_verts, f, s);
        if (!face_culled(s, a.cull_backfaces)) {
            for (int n = 0; n < a.N; ++n) {   // the lowest mesh whose range holds the face (N is a batch size)
                const long long first = a.first_idx[n];
                if (fl >= first && fl - first < a.num_faces[n]) {
                    mesh = (uint32_t)n;
                    break;
                }
            }
            int i0, i1, j0, j1;
            if (mesh != kNoMesh && pixel_span(s.xmin, s.xmax, a.W, a.H, i0, i1) && pixel_span(s.ymin, s.ymax, a.H, a.W, j0, j1)) {
                // pixel index i along x is column W - 1 - i, along y row H - 1 - i
                const uint32_t c0 = (uint32_t)(a.W - 1 - i1) >> 4, c1 = (uint32_t)(a.W - 1 - i0) >> 4;
                const uint32_t r0 = (uint32_t)(a.H - 1 - j1) >> 4, r1 = (uint32_t)(a.H - 1 - j0) >> 4;
                rect = make_uint2(c0 | c1 << 16, r0 | r1 << 16);
            } else {
                mesh = kNoMesh;
            }
        }
        a.rects[f] = rect;
        a.mesh[f] = mesh;
    }
    const bool live = mesh != kNoMesh;
    const uint32_t base = live ? mesh * (uint32_t)(a.tiles_x * a.tiles_y) : 0u;
    uint32_t* counts = a.counts;
    for_each_tile(live, base, (uint32_t)a.tiles_x, rect, (uint32_t)f, [counts](uint32_t tile, uint32_t) { atomicAdd(&counts[tile], 1u); });
}

__global__ __launch_bounds__(kMeshThreads) void mesh_fill_kernel(const MeshBinArgs a) {
    const long long fl = (long long)blockIdx.x * kMeshThreads + threadIdx.x;
    const bool in_range = fl < a.F;
    const int f = in_range ? (int)fl : 0;
    const uint32_t mesh = in_range ? a.mesh[f] : kNoMesh;
    const bool live = mesh != kNoMesh && mesh < (uint32_t)a.N;
    const uint2 rect = live ? a.rects[f] : make_uint2(0u, 0u);
    const uint32_t base = live ? mesh * (uint32_t)(a.tiles_x * a.tiles_y) : 0u;
    uint32_t* cursors = a.counts;
    const uint32_t* offsets = a.offsets;
    uint32_t* pairs = a.pairs;
    const uint32_t total = a.pair_total;
    for_each_tile(live, base, (uint32_t)a.tiles_x, rect, (uint32_t)f, [=](uint32_t tile, uint32_t face) {
        const unsigned long long at = (unsigned long long)offsets[tile] + atomicAdd(&cursors[tile], 1u);
        if (at < total) pairs[at] = face;   // (always, for the plan this total was read from)
    });
}

// One workgroup: offsets = exclusive prefix of counts, counts cleared, the total into the header.  Sums in 64 bits (the offsets are
// stored in 32: a total they cannot hold is refused by gsr_mesh_raster before anything reads them).
__global__ __launch_bounds__(kMeshThreads) void mesh_scan_kernel(uint32_t* counts, uint32_t* offsets, long long tiles, MeshPlanHeader* header) {
    __shared__ unsigned long long s_wave[kMeshThreads / 64];   // 64 bits: a round of 4096 tiles may hold 2^32 pairs, and the total decides a refusal
    const int t = threadIdx.x;
    unsigned long long running = 0;
    for (long long start = 0; start < tiles; start += (long long)kMeshThreads * kScanPerLane) {
        const long long mine = start + (long long)t * kScanPerLane;
        uint32_t v[kScanPerLane];
        unsigned long long sum = 0;
#pragma unroll
        for (int i = 0; i < kScanPerLane; ++i) {
            v[i] = mine + i < tiles ? counts[mine + i] : 0u;
            sum += v[i];
        }
        unsigned long long round_total;
        unsigned long long at = running + block_exclusive_scan<kMeshThreads / 64>(sum, s_wave, &round_total);
        running += round_total;
#pragma unroll
        for (int i = 0; i < kScanPerLane; ++i) {
            if (mine + i < tiles) {
                offsets[mine + i] = (uint32_t)at;
                counts[mine + i] = 0u;
            }
            at += v[i];
        }
    }
    if (t == 0) header->pair_total = running;
}

// ---- the z-buffer ------------------------------------------------------------------------------------------------------------------

struct MeshRasterArgs {
    int F, N, H, W, K;
    int tiles_x, tiles_y;
    int perspective, clip, cull_backfaces;
    const float* face_verts;
    const long long* first_idx;
    const long long* num_faces;
    const long long* nbr;
    const uint32_t* offsets;
    uint32_t* cursors;
    const uint32_t* pairs;
    uint32_t pair_total;
    long long* pix_to_face;
    float* zbuf;
    float* bary;
    float* dists;
};

// The neighbour rule: face s.face names s.nbr; it gives way when that face is kept at the pixel too and is nearer to its own edges
// (equal: the lower index stays).
__device__ inline bool yields_to_neighbour(const MeshRasterArgs& a, const FaceSetup& s, float px, float py, long long mesh_first,
                                           long long mesh_count) {
    const long long g = s.nbr;
    if (g == s.face || g < mesh_first || g - mesh_first >= mesh_count || g >= a.F) return false;
    FaceSetup o;
    load_face(a.face_verts, (int)g, o);
    if (face_culled(o, a.cull_backfaces)) return false;
    float pz, b0, b1, b2;
    if (!face_at_pixel(o, px, py, a.perspective, a.clip, pz, b0, b1, b2)) return false;
    const float mine = triangle_dist2(s, px, py), theirs = triangle_dist2(o, px, py);
    return theirs < mine || (theirs == mine && g < s.face);
}

template <int KB>
__global__ __launch_bounds__(kMeshThreads) void mesh_raster_kernel(const MeshRasterArgs a) {
    __shared__ FaceSetup staged[kMeshChunk];
    const int tiles = a.tiles_x * a.tiles_y;
    const int n = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int col = (tile % a.tiles_x) * kTile + (threadIdx.x & 15), row = (tile / a.tiles_x) * kTile + (threadIdx.x >> 4);
    const bool on_image = col < a.W && row < a.H;
    const float px = pix_to_ndc(a.W - 1 - col, a.W, a.H), py = pix_to_ndc(a.H - 1 - row, a.H, a.W);
    const long long mesh_first = a.first_idx[n], mesh_count = a.num_faces[n];

    // this tile's list: [begin, end) of the pair list, never past what the caller allocated
    const uint32_t begin = min(a.offsets[blockIdx.x], a.pair_total);
    const uint32_t end = (long long)blockIdx.x + 1 < (long long)a.N * tiles ? min(max(a.offsets[blockIdx.x + 1], begin), a.pair_total) : a.pair_total;

    if (threadIdx.x == 0) a.cursors[blockIdx.x] = 0u;   // the fill's cursor of this tile: the plan is ready for another fill

    float slot_z[KB];
    int slot_f[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) slot_z[k] = INFINITY, slot_f[k] = INT_MAX;

    for (uint32_t chunk = begin; chunk < end; chunk += kMeshChunk) {
        const int in_chunk = (int)min((uint32_t)kMeshChunk, end - chunk);
        __syncthreads();
        if ((int)threadIdx.x < in_chunk) {
            const uint32_t f = a.pairs[chunk + threadIdx.x];
            FaceSetup s;
            if (f < (uint32_t)a.F) {
                load_face(a.face_verts, (int)f, s);
                const long long g = a.nbr[f];
                s.nbr = g >= 0 && g <= INT_MAX ? (int)g : -1;
            } else {   // (a list the fill did not write: no pixel is inside an empty box)
                s = FaceSetup{};
                s.xmin = 1.0f, s.xmax = -1.0f, s.nbr = -1;
            }
            staged[threadIdx.x] = s;
        }
        __syncthreads();
        if (!on_image) continue;
        for (int j = 0; j < in_chunk; ++j) {
            const FaceSetup& s = staged[j];
            float pz, b0, b1, b2;
            if (!face_at_pixel(s, px, py, a.perspective, a.clip, pz, b0, b1, b2)) continue;
            if (s.nbr >= 0 && yields_to_neighbour(a, s, px, py, mesh_first, mesh_count)) continue;
            const int face = s.face;
#pragma unroll
            for (int k = KB - 1; k >= 0; --k) {   // ascending (pz, face): the new pair moves down while it is the smaller one
                if (pz < slot_z[k] || (pz == slot_z[k] && face < slot_f[k])) {
                    if (k + 1 < KB) slot_z[k + 1] = slot_z[k], slot_f[k + 1] = slot_f[k];
                    slot_z[k] = pz, slot_f[k] = face;
                }
            }
        }
    }
    if (!on_image) return;

    const size_t pixel = ((size_t)n * a.H + row) * a.W + col;
    long long* out_face = a.pix_to_face + pixel * a.K;
    float* out_z = a.zbuf + pixel * a.K;
    float* out_b = a.bary + pixel * a.K * 3;
    float* out_d = a.dists + pixel * a.K;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        if (k < a.K) {
            long long face = -1;
            float z = -1.0f, b0 = -1.0f, b1 = -1.0f, b2 = -1.0f, d = -1.0f;
            if (slot_f[k] != INT_MAX) {
                FaceSetup s;
                load_face(a.face_verts, slot_f[k], s);
                face_at_pixel(s, px, py, a.perspective, a.clip, z, b0, b1, b2);   // as when it was listed: kept, and z == slot_z[k]
                d = -triangle_dist2(s, px, py);
                face = slot_f[k];
            }
            out_face[k] = face;
            out_z[k] = z;
            out_b[3 * k + 0] = b0, out_b[3 * k + 1] = b1, out_b[3 * k + 2] = b2;
            out_d[k] = d;
        }
    }
}

// F == 0: every output element is -1.
__global__ __launch_bounds__(kMeshThreads) void mesh_empty_kernel(size_t slots, long long* pix_to_face, float* zbuf, float* bary, float* dists) {
    for (size_t i = (size_t)blockIdx.x * kMeshThreads + threadIdx.x; i < slots; i += (size_t)gridDim.x * kMeshThreads) {
        pix_to_face[i] = -1;
        zbuf[i] = -1.0f;
        dists[i] = -1.0f;
        bary[3 * i + 0] = -1.0f, bary[3 * i + 1] = -1.0f, bary[3 * i + 2] = -1.0f;
    }
}

inline int tiles_of(int side) { return (side + kTile - 1) / kTile; }

// What both steps refuse about the sizes; nullptr when they are fine.
const char* bad_sizes(int64_t F, int64_t N, int H, int W) {
    if (F < 0 || N < 0) return "negative count";
    if (F >= (int64_t)INT_MAX) return "2^31 - 1 faces or more";
    if (H < 1 || H > kMeshMaxSide || W < 1 || W > kMeshMaxSide) return "H and W must be in 1..16384";
    if (N * (int64_t)tiles_of(H) * tiles_of(W) >= (int64_t)INT_MAX) return "2^31 - 1 tiles or more over the batch";
    return nullptr;
}

}  // namespace
}  // namespace gsr

using gsr::fail;

extern "C" {

size_t gsr_mesh_raster_plan_bytes(int64_t F, int64_t N, int H, int W) {
    if (gsr::bad_sizes(F, N, H, W)) return 0;
    return gsr::plan_layout(F, N * (int64_t)gsr::tiles_of(H) * gsr::tiles_of(W), nullptr).bytes;
}

size_t gsr_mesh_raster_pair_bytes(int64_t pairs) {
    if (pairs < 0 || pairs >= ((int64_t)1 << 31)) return 0;
    return gsr::round256((size_t)(pairs > 0 ? pairs : 1) * sizeof(uint32_t));
}

int gsr_mesh_raster_count(int64_t F, int64_t N, const float* face_verts, const int64_t* mesh_to_face_first_idx, const int64_t* num_faces_per_mesh,
                          int H, int W, int cull_backfaces, void* plan, size_t plan_bytes, int64_t* pair_total, void* stream_) {
    if (const char* why = gsr::bad_sizes(F, N, H, W)) return fail(GSR_ERR_INVALID_ARG, "gsr_mesh_raster_count: %s", why);
    if (!pair_total) return fail(GSR_ERR_INVALID_ARG, "gsr_mesh_raster_count: null pointer (pair_total)");
    *pair_total = 0;
    if (F == 0 || N == 0) return GSR_OK;
    if (!face_verts || !mesh_to_face_first_idx || !num_faces_per_mesh || !plan) return fail(GSR_ERR_INVALID_ARG, "gsr_mesh_raster_count: null pointer");
    if (((uintptr_t)face_verts & 3u) != 0u || !gsr::aligned8(mesh_to_face_first_idx) || !gsr::aligned8(num_faces_per_mesh) || !gsr::aligned256(plan))
        return fail(GSR_ERR_INVALID_ARG, "gsr_mesh_raster_count: misaligned pointer (face_verts: 4 bytes, the index arrays: 8, plan: 256)");
    const size_t need = gsr_mesh_raster_plan_bytes(F, N, H, W);
    if (plan_bytes < need) return fail(GSR_ERR_INVALID_ARG, "gsr_mesh_raster_count: scratch too small (%zu of %zu bytes)", plan_bytes, need);
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t tiles = N * (int64_t)gsr::tiles_of(H) * gsr::tiles_of(W);
    const gsr::MeshPlan L = gsr::plan_layout(F, tiles, plan);
    gsr::MeshBinArgs a{};
    a.F = (int)F, a.N = (int)N, a.H = H, a.W = W, a.tiles_x = gsr::tiles_of(W), a.tiles_y = gsr::tiles_of(H), a.cull_backfaces = cull_backfaces != 0;
    a.face_verts = face_verts;
    a.first_idx = reinterpret_cast<const long long*>(mesh_to_face_first_idx), a.num_faces = reinterpret_cast<const long long*>(num_faces_per_mesh);
    a.rects = L.rects, a.mesh = L.mesh, a.counts = L.counts;
    GSR_HIP(hipMemsetAsync(L.counts, 0, (size_t)tiles * sizeof(uint32_t), stream));
    const unsigned blocks = (unsigned)((F + gsr::kMeshThreads - 1) / gsr::kMeshThreads);
    hipLaunchKernelGGL(gsr::mesh_count_kernel, dim3(blocks), dim3(gsr::kMeshThreads), 0, stream, a);
    hipLaunchKernelGGL(gsr::mesh_scan_kernel, dim3(1), dim3(gsr::kMeshThreads), 0, stream, L.counts, L.offsets, (long long)tiles, L.header);
    GSR_HIP(hipGetLastError());
    unsigned long long total = 0;
    GSR_HIP(hipMemcpyAsync(&total, &L.header->pair_total, sizeof(total), hipMemcpyDeviceToHost, stream));
    GSR_HIP(hipStreamSynchronize(stream));
    *pair_total = (int64_t)total;
    return GSR_OK;
}

int gsr_mesh_raster(int64_t F, int64_t N, const float* face_verts, const int64_t* mesh_to_face_first_idx, const int64_t* num_faces_per_mesh,
                    const int64_t* clipped_faces_neighbor_idx, int H, int W, float blur_radius, int K, int perspective_correct,
                    int clip_barycentric_coords, int cull_backfaces, void* plan, size_t plan_bytes, int64_t pair_total, void* pairs,
                    size_t pair_bytes, int64_t* pix_to_face, float* zbuf, float* bary_coords, float* dists, void* stream_) {
    if (K < 1 || K > gsr::kMeshMaxK) return fail(GSR_ERR_INVALID_ARG, "gsr_mesh_raster: K = %d (1 to %d)", K, gsr::kMeshMaxK);
    if (!(blur_radius == 0.0f)) return fail(GSR_ERR_INVALID_ARG, "gsr_mesh_raster: blur_radius = %g (only 0 is built)", (double)blur_radius);
    if (const char* why = gsr::bad_sizes(F, N, H, W)) return fail(GSR_ERR_INVALID_ARG, "gsr_mesh_raster: %s", why);
    if (pair_total < 0) return fail(GSR_ERR_INVALID_ARG, "gsr_mesh_raster: negative count (pair_total)");
    if (pair_total >= ((int64_t)1 << 31)) return fail(GSR_ERR_INVALID_ARG, "gsr_mesh_raster: %lld (tile, face) pairs (at most 2^31 - 1)", (long long)pair_total);
    if (N == 0) return GSR_OK;
    if (!pix_to_face || !zbuf || !bary_coords || !dists) return fail(GSR_ERR_INVALID_ARG, "gsr_mesh_raster: null pointer (outputs)");
    if (!gsr::aligned8(pix_to_face) || ((uintptr_t)zbuf & 3u) != 0u || ((uintptr_t)bary_coords & 3u) != 0u || ((uintptr_t)dists & 3u) != 0u)
        return fail(GSR_ERR_INVALID_ARG, "gsr_mesh_raster: misaligned pointer (pix_to_face: 8 bytes, zbuf / bary_coords / dists: 4)");
    hipStream_t stream = (hipStream_t)stream_;
    if (F == 0) {
        const size_t slots = (size_t)N * H * W * K;
        const unsigned blocks = (unsigned)((slots + gsr::kMeshThreads - 1) / gsr::kMeshThreads < 4096 ? (slots + gsr::kMeshThreads - 1) / gsr::kMeshThreads : 4096);
        hipLaunchKernelGGL(gsr::mesh_empty_kernel, dim3(blocks), dim3(gsr::kMeshThreads), 0, stream, slots, reinterpret_cast<long long*>(pix_to_face),
                           zbuf, bary_coords, dists);
        GSR_HIP(hipGetLastError());
        return GSR_OK;
    }
    if (!face_verts || !mesh_to_face_first_idx || !num_faces_per_mesh || !clipped_faces_neighbor_idx || !plan || !pairs)
        return fail(GSR_ERR_INVALID_ARG, "gsr_mesh_raster: null pointer");
    if (((uintptr_t)face_verts & 3u) != 0u || !gsr::aligned8(mesh_to_face_first_idx) || !gsr::aligned8(num_faces_per_mesh) ||
        !gsr::aligned8(clipped_faces_neighbor_idx) || !gsr::aligned256(plan) || !gsr::aligned256(pairs))
        return fail(GSR_ERR_INVALID_ARG, "gsr_mesh_raster: misaligned pointer (face_verts: 4 bytes, the index arrays: 8, plan / pairs: 256)");
    const size_t need_plan = gsr_mesh_raster_plan_bytes(F, N, H, W), need_pairs = gsr_mesh_raster_pair_bytes(pair_total);
    if (plan_bytes < need_plan) return fail(GSR_ERR_INVALID_ARG, "gsr_mesh_raster: plan scratch too small (%zu of %zu bytes)", plan_bytes, need_plan);
    if (pair_bytes < need_pairs) return fail(GSR_ERR_INVALID_ARG, "gsr_mesh_raster: pair scratch too small (%zu of %zu bytes)", pair_bytes, need_pairs);

    const int64_t tiles = N * (int64_t)gsr::tiles_of(H) * gsr::tiles_of(W);
    const gsr::MeshPlan L = gsr::plan_layout(F, tiles, plan);
    gsr::MeshBinArgs b{};
    b.F = (int)F, b.N = (int)N, b.H = H, b.W = W, b.tiles_x = gsr::tiles_of(W), b.tiles_y = gsr::tiles_of(H), b.cull_backfaces = cull_backfaces != 0;
    b.face_verts = face_verts;
    b.rects = L.rects, b.mesh = L.mesh, b.counts = L.counts, b.offsets = L.offsets;
    b.pairs = static_cast<uint32_t*>(pairs), b.pair_total = (uint32_t)pair_total;
    if (pair_total > 0) {
        const unsigned blocks = (unsigned)((F + gsr::kMeshThreads - 1) / gsr::kMeshThreads);
        hipLaunchKernelGGL(gsr::mesh_fill_kernel, dim3(blocks), dim3(gsr::kMeshThreads), 0, stream, b);
    }
    gsr::MeshRasterArgs a{};
    a.F = (int)F, a.N = (int)N, a.H = H, a.W = W, a.K = K, a.tiles_x = b.tiles_x, a.tiles_y = b.tiles_y;
    a.perspective = perspective_correct != 0, a.clip = clip_barycentric_coords != 0, a.cull_backfaces = cull_backfaces != 0;
    a.face_verts = face_verts;
    a.first_idx = reinterpret_cast<const long long*>(mesh_to_face_first_idx), a.num_faces = reinterpret_cast<const long long*>(num_faces_per_mesh);
    a.nbr = reinterpret_cast<const long long*>(clipped_faces_neighbor_idx);
    a.offsets = L.offsets, a.cursors = L.counts, a.pairs = b.pairs, a.pair_total = b.pair_total;
    a.pix_to_face = reinterpret_cast<long long*>(pix_to_face), a.zbuf = zbuf, a.bary = bary_coords, a.dists = dists;
    const dim3 grid((unsigned)tiles), block(gsr::kMeshThreads);
    if (K == 1) hipLaunchKernelGGL(gsr::mesh_raster_kernel<1>, grid, block, 0, stream, a);
    else if (K <= 4) hipLaunchKernelGGL(gsr::mesh_raster_kernel<4>, grid, block, 0, stream, a);
    else if (K <= 8) hipLaunchKernelGGL(gsr::mesh_raster_kernel<8>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(gsr::mesh_raster_kernel<16>, grid, block, 0, stream, a);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

}  // extern "C"
