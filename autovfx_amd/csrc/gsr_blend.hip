// gsr_blend.hip -- front-to-back alpha compositing of the per-tile lists, for gfx950.
//
//   blend_quadrant_kernel <- renderCUDA   DGR/cuda_rasterizer/forward.cu:261-378
//   (DGR = sugar/gaussian_splatting/submodules/diff-gaussian-rasterization, under /root/reference)
//
// One wave64 per 8x8 QUADRANT of a 16x16 tile (4 single-wave workgroups per tile), one pixel per lane; no workgroup
// barriers.  Per (pixel, entry) the arithmetic is the reference's (forward.cu:331-364), op for op; the shape of the
// work is not:
//   * a quadrant stops as soon as ITS 64 pixels are done, and a tile whose list is long or never saturates does not
//     pin one 256-thread block for the whole launch;
//   * while staging a batch of 64 list entries each lane runs the conservative reach test of its entry against the
//     quadrant (gsr_device.h: splat_reaches_rect, the minimum of q over the two lines of the quadrant the centre can see;
//     balloted per comparison, so which entries reach, which are staged in this round and which are left are scalar masks
//     from the start); the wave then walks only the set bits, so entries that cannot touch the quadrant cost no LDS read
//     and no per-pixel work at all;
//   * the entries that reach are parked in LDS slots in list order, each with the terms of `power` that depend only on
//     the pixel's column or only on its row (gsr_device.h: blend_power_terms), computed by the entry's own lane while it
//     stages: the walk reads its column's pair and its row's pair and is left with an add, a multiply and a subtract
//     per (entry, pixel); slots are addressed by the reads' immediate offsets in a body unrolled over kWalkUnroll slots;
//   * which pixels have stopped is a wave-uniform 64-bit mask in scalar registers, combined only in uniform control
//     flow, so "any pixel live?" / "all done?" cost no vector instructions and the accumulate block is gated through
//     the exec mask (inverse_ballot);
//   * `power < skip_below` (skip_below = -ln(255 o) - 1e-4) skips expf for pairs that cannot reach alpha >= 1/255:
//     below it o * exp(power) is < 1/255 by a margin ~100x the combined rounding error of logf / expf / the products,
//     so the reference's `alpha < 1/255` test would have skipped the pair too;
//   * optionally a second per-Gaussian feature triple is composited in the same walk (kExtra).
//
// Depth slabs (inference calls, gsr_api.hip): the list of a tile arrives in up to kMaxSlabs segments, front to back,
// and a launch walks a range of them.  Between two launches the pixel state lives in the output images themselves --
// accumulated colour / depth / second feature set without the background term, the transmittance T in the alpha plane
// with its sign set once the pixel has stopped, the last contributor in n_contrib -- and a quadrant whose 64 pixels
// have all stopped writes its final values at once, marks itself in `quad_done` (later launches leave after one
// scalar load) and, when it completes its tile, the tile in `done_rows`, which is what lets the next slab drop that
// tile's pairs before they are expanded.  A pixel's sequence of operations is exactly that of one walk over the
// concatenated list: same bits.
// Defines the entry point gsr_selftest_exp.
#include "gsr_device.h"

// Profiling aid (python -m autovfx_amd.build --trace, scripts/kernel_trace.py --blend): every single-wave workgroup stamps the
// 100 MHz wall clock at its start and end.  Compiled out of the normal library.
#ifdef GSR_KERNEL_TRACE
__device__ unsigned long long* g_blend_trace = nullptr;
extern "C" __attribute__((visibility("default"))) int gsr_debug_set_blend_trace(void* device_words) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_blend_trace), &device_words, sizeof device_words);
}
#define GSR_LTRACE(id, slot) do { if (threadIdx.x == 0 && g_blend_trace) g_blend_trace[(size_t)(id) * 2 + (slot)] = wall_clock64(); } while (0)
#else
#define GSR_LTRACE(id, slot) do { } while (0)
#endif

namespace gsr {
namespace {

// C += feature * alpha * T (forward.cu:357-360) with the last product fused into the addition, fma(feature * alpha,
// T, C): what nvcc, which contracts by default, makes of that line on the reference's own hardware, and one
// full-rate fused instruction in place of a multiply and an add.  This library is otherwise built without
// contraction; this is the one place it is written out, because it is on the per-pair-per-pixel path and touches
// only the float images (transmittance, the stopping rule and every integer output do not depend on it).
//
// GSR_UNFUSED_BLEND (python -m autovfx_amd.build --unfused -> lib/libgsr_hip_unfused.so, a TEST build): the same line as the
// reference's sources say it when compiled without contraction -- multiply, multiply, add.  The reference's own kernels
// compiled for gfx950 with -ffp-contract=off (oracle/_ref/libgsr_ref_hip.so) then produce the SAME BITS in every image, which
// turns the image tolerance of the parity tests into an equality once per suite run (tests/test_parity_gpu.py:
// test_unfused_blend_build_equals_the_reference_kernels_bit_for_bit).
__device__ __forceinline__ float composite(float C, float feature, float alpha, float T) {
#ifdef GSR_UNFUSED_BLEND
    return C + (feature * alpha) * T;
#else
    return __builtin_fmaf(feature * alpha, T, C);
#endif
}
// Two channels at once: v_pk_mul_f32 + v_pk_fma_f32, written with a vector type so that the pairing does not depend
// on what the SLP vectorizer decides.  Same roundings as two calls of composite().
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f composite2(v2f C, v2f feature, float alpha, float T) {
#ifdef GSR_UNFUSED_BLEND
    return C + (feature * alpha) * (v2f){T, T};
#else
    return __builtin_elementwise_fma(feature * alpha, (v2f){T, T}, C);
#endif
}

__global__ void exp_selftest_kernel(uint32_t first_bits, uint32_t count, unsigned long long* mismatches) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float x = __uint_as_float(first_bits + i);
    const float a = expf(x), b = exp_nonpositive(x);
    if (__float_as_uint(a) != __float_as_uint(b) && !(a != a && b != b)) atomicAdd(mismatches, 1ull);
}

struct BlendArgs {
    int W, H, grid_x, num_tiles;
    BlendOrder order;
    BlendSegments segs;
    int seg_begin, seg_end;
    int fresh, final;
    const SplatRaster* raster;
    const float* features;
    const float* extra_features;
    const float* background;
    float* out_color;
    float* out_depth;
    float* out_alpha;
    float* out_extra;
    uint32_t* n_contrib;
    uint32_t* quad_done;
    uint32_t* done_rows;
    int row_words;
};

// This quadrant is finished for good: later launches skip it; the quadrant that completes a tile marks the tile.
__device__ __forceinline__ void mark_quadrant_done(const BlendArgs& a, int item) {
    if (threadIdx.x != 0) return;
    const uint32_t bit = 1u << (item & 31);
    const uint32_t old = atomicOr(&a.quad_done[item >> 5], bit);
    const int shift = (item & 31) & ~3;  // the four quadrants of a tile share one aligned nibble
    if ((((old | bit) >> shift) & 0xFu) == 0xFu) {
        const int tile = item >> 2, tx = tile % a.grid_x, ty = tile / a.grid_x;
        atomicOr(&a.done_rows[ty * a.row_words + (tx >> 5)], 1u << (tx & 31));
    }
}

// The LDS of one single-wave workgroup: kCount slots of kStride bytes, then one tail word (or, with the second feature set,
// one 16-byte tail record) per slot.
//   slot  +0    eight column pairs ((mh_cxx dx) dx, cxy dx)     one 8-byte read per lane, address by lane & 7
//         +64   eight row pairs    ((mh_cyy dy) dy, dy)         one 8-byte read per lane, address by lane >> 3
//         +128  skip_below, opacity                             broadcast, every processed entry
//         +136  r, g   +144  b, z                               broadcast, contributing entries only
//   tail  the entry's index in its batch of 64 (with the second set: ex, ey, ez, index)
// 32 workgroups share a CU's 160 KiB at eight waves per SIMD: 5 120 bytes each.  kStride = 152 bytes = 38 dwords, and
// 38 mod 32 = 6 = 2 * 3: the 8-byte stores of 16 consecutive slots (one store group) fall on 16 different bank pairs, and the
// walk's reads are 8 neighbouring pairs or one address.  152 is not a multiple of 16, so (r, g, b, z) is read as two 8-byte halves.
template <bool kExtra>
struct BlendSlots {
    static constexpr int kCount = kExtra ? 30 : 32;
    static constexpr int kStride = 152;
    static constexpr int kCol = 0, kRow = 64, kGate = 128, kRG = 136, kBZ = 144;
    static constexpr int kTail = kCount * kStride;
    static constexpr int kTailStride = kExtra ? 16 : 4;
    static constexpr int kBytes = kTail + kCount * kTailStride;
    static_assert(kStride % 8 == 0 && (kStride / 4) % 4 == 2 && kTail % 16 == 0, "8-byte slots on distinct bank pairs; aligned tail");
    static_assert(32 * kBytes <= 160 * 1024 && kCount <= 64, "32 single-wave workgroups per CU");
};
constexpr int kWalkUnroll = 8;

// kExtra: a second per-Gaussian feature triple (extra_features[P,3] -> out_extra[3,H,W]) is composited in the
// same walk with the same alpha and transmittance -- what the reference's render() obtains from a second full
// rasterizer pass for its normal map (gaussian_renderer/__init__.py:176-184): identical arithmetic per channel,
// one list walk instead of two.
template <bool kExtra>
__global__ void __launch_bounds__(64, 8) blend_quadrant_kernel(BlendArgs a) {
    using Slots = BlendSlots<kExtra>;
    __shared__ __attribute__((aligned(16))) char s_slots[Slots::kBytes];

    constexpr int kQ = kQuad;
    const int W = a.W, H = a.H;
    // the 4 quadrants of a tile share an XCD; large images: longest lists first inside the XCD's band (BlendOrder)
    const int item = a.order.counts == nullptr ? xcd_band_tile(blockIdx.x, 4 * a.num_tiles) : ordered_item(a.order, blockIdx.x);
    if (item < 0) return;   // (the ordered grid is padded to the largest band)
    const int tile = item >> 2, quad = item & 3;
    const int lane = threadIdx.x;
    const bool fresh = a.fresh != 0, final = a.final != 0;
    GSR_LTRACE(a.seg_begin * 40960 + blockIdx.x, 0);
    if (!fresh && ((a.quad_done[item >> 5] >> (item & 31)) & 1u)) return;  // finished by an earlier launch
    const int qx0 = (tile % a.grid_x) * kTile + kQ * (quad & 1);
    const int qy0 = (tile / a.grid_x) * kTile + kQ * (quad >> 1);
    const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const bool inside = px < W && py < H;
    const size_t plane = (size_t)W * (size_t)H;
    const size_t pid = (size_t)W * (size_t)py + (size_t)px;
    // Which pixels have stopped is a wave-uniform 64-bit mask in scalar registers: tests on it ("any pixel
    // live?", "all done?") cost no vector instructions, and it gates the per-pixel block through the
    // execution mask directly.
    unsigned long long done_mask = __ballot(!inside);
    if (done_mask == ~0ull) {  // quadrant entirely outside the image: nothing to write
        if (!final) mark_quadrant_done(a, item);
        return;
    }

    float T = 1.f, Eb = 0.f;
    v2f Crg = {0.f, 0.f}, Cbz = {0.f, 0.f}, Erg = {0.f, 0.f};  // red|green, blue|depth, second set red|green
    uint32_t last = 0u;
    if (!fresh) {  // resume the state an earlier launch parked in the output images
        bool stopped = false;
        if (inside) {
            const float ts = a.out_alpha[pid];
            stopped = (__float_as_uint(ts) >> 31) != 0u;
            T = fabsf(ts);
            Crg = (v2f){a.out_color[pid], a.out_color[plane + pid]};
            Cbz = (v2f){a.out_color[2 * plane + pid], a.out_depth[pid]};
            last = a.n_contrib[pid];
            if (kExtra) {
                Erg = (v2f){a.out_extra[pid], a.out_extra[plane + pid]};
                Eb = a.out_extra[2 * plane + pid];
            }
        }
        done_mask |= __ballot(stopped);
    }

    // The pixel coordinates of the quadrant's eight columns and eight rows, wave-uniform, in scalar registers for the staging
    // lanes; the two lane-constant LDS offsets of the walk (this lane's column pair and row pair inside a slot).
    float qfx[kQ], qfy[kQ];
#pragma unroll
    for (int i = 0; i < kQ; ++i) {
        qfx[i] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint((float)(qx0 + i))));
        qfy[i] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint((float)(qy0 + i))));
    }
    const uint32_t lane_col = Slots::kCol + 8u * ((uint32_t)lane & 7u), lane_row = Slots::kRow + 8u * ((uint32_t)lane >> 3);

    uint32_t seg_base = 0u;  // list positions of earlier segments (n_contrib counts through the concatenation)
    for (int seg = 0; seg < a.seg_begin; ++seg) {  // ... also of the segments earlier launches walked
        const uint2 earlier = a.segs.ranges[seg][tile];
        seg_base += earlier.y - earlier.x;
    }
    for (int seg = a.seg_begin; seg < a.seg_end && done_mask != ~0ull; ++seg) {
        const uint2 range = a.segs.ranges[seg][tile];
        const uint32_t count = range.y - range.x;
        const uint32_t* __restrict__ point_list = a.segs.point_list[seg] + range.x;

        float2 g_xy = make_float2(0.f, 0.f);
        float4 g_co = make_float4(0.f, 0.f, 0.f, 0.f);
        F3 g_rgb = {0.f, 0.f, 0.f}, g_ext = {0.f, 0.f, 0.f};
        float g_z = 0.f, g_skip = 0.f;
        auto gather = [&](uint32_t first) {
            const uint32_t e = first + (uint32_t)lane;
            if (e < count) {
                const uint32_t id = point_list[e];
                const float4* rec = reinterpret_cast<const float4*>(a.raster + id);  // 32 bytes, one cache line
                const float4 r0 = rec[0], r1 = rec[1];
                g_xy = make_float2(r0.x, r0.y);
                g_co = make_float4(r0.z, r0.w, r1.x, r1.y);
                g_z = r1.z;
                g_skip = r1.w;
                g_rgb = ld3(a.features + 3 * (size_t)id);
                if (kExtra) g_ext = ld3(a.extra_features + 3 * (size_t)id);
            }
        };
        if (count > 0) gather(0);

        for (uint32_t first = 0; first < count; first += 64) {
            // (the masks stay wave-uniform scalars: ballots of single comparisons, combined and consumed without a vector register)
            unsigned long long todo = __ballot(first + (uint32_t)lane < count) &
                                      splat_reaches_rect_ballot(g_co, g_skip, g_xy, qfx[0], qfx[kQ - 1], qfy[0], qfy[kQ - 1]);
            // The reaching entries are walked in rounds of at most Slots::kCount (C3: about 22 of a batch's 64 reach, so nearly
            // always one round); a later round builds its slots from the same g_* registers, which is why the next batch is
            // prefetched into them only once the batch's LAST round is built.
            for (;;) {
                uint32_t n = 0u;
                if (todo != 0ull) {
                    // lane = entry: a reaching entry takes the slot of its rank among the reaching ones, so slots are in list order
                    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(todo >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)todo, 0u));
                    const unsigned long long taken = todo & __ballot(rank < (uint32_t)Slots::kCount);
                    __syncthreads();  // single-wave workgroup: orders this wave's LDS reads / writes only
                    if (__builtin_amdgcn_inverse_ballot_w64(taken)) {
                        char* slot = s_slots + rank * (uint32_t)Slots::kStride;
                        // The conic's diagonal goes in already multiplied by -0.5: scaling by a power of two commutes with every
                        // rounding of -0.5 * (cxx*dx*dx + cyy*dy*dy), so the terms give the same bits with one multiply less.
                        blend_power_terms(g_xy.x, g_xy.y, -0.5f * g_co.x, g_co.y, -0.5f * g_co.z, qfx, qfy,
                                          reinterpret_cast<float2*>(slot + Slots::kCol), reinterpret_cast<float2*>(slot + Slots::kRow));
                        *reinterpret_cast<float2*>(slot + Slots::kGate) = make_float2(g_skip, g_co.w);
                        *reinterpret_cast<float2*>(slot + Slots::kRG) = make_float2(g_rgb.x, g_rgb.y);
                        *reinterpret_cast<float2*>(slot + Slots::kBZ) = make_float2(g_rgb.z, g_z);
                        char* tail = s_slots + Slots::kTail + rank * (uint32_t)Slots::kTailStride;
                        if (kExtra) *reinterpret_cast<float4*>(tail) = make_float4(g_ext.x, g_ext.y, g_ext.z, __uint_as_float((uint32_t)lane));
                        else *reinterpret_cast<uint32_t*>(tail) = (uint32_t)lane;
                    }
                    __syncthreads();
                    n = (uint32_t)__popcll(taken);
                    todo &= ~taken;
                }
                if (todo == 0ull && first + 64 < count) gather(first + 64);

                for (uint32_t s = 0u; s < n; s += kWalkUnroll) {
                    // The addresses of slot s for this lane, parked in vector registers the compiler cannot see through: the
                    // kWalkUnroll slots of the body below differ only in the immediate offsets of their reads.
                    uint32_t col_a = lane_col + s * (uint32_t)Slots::kStride, row_a = lane_row + s * (uint32_t)Slots::kStride;
                    uint32_t slot_a = s * (uint32_t)Slots::kStride, tail_a = (uint32_t)Slots::kTail + s * (uint32_t)Slots::kTailStride;
                    asm("" : "+v"(col_a), "+v"(row_a), "+v"(slot_a), "+v"(tail_a));
#pragma unroll
                    for (int u = 0; u < kWalkUnroll; ++u) {
                        if (s + (uint32_t)u >= n) break;
                        const char* slot_u = s_slots + u * Slots::kStride;
                        const char* tail_u = s_slots + u * Slots::kTailStride + tail_a;
                        // The LDS unit is this kernel's second limiter after vector issue (profiles/r09_blend_terms.md): every
                        // read of an entry is issued here, in one round trip, each as ONE 8-byte read of two LDS cycles.  The
                        // empty asm statements keep it so: the compiler would read skip_below and opacity as two halves (the
                        // second behind the first early exit: a second round trip), pair neighbouring 8-byte reads into one
                        // 8-cycle ds_read2_b64, and sink the colour reads behind the last early exit (a third round trip).
                        const float2 cp = *reinterpret_cast<const float2*>(slot_u + col_a);
                        const float2 rp = *reinterpret_cast<const float2*>(slot_u + row_a);
                        unsigned long long gate_bits = *reinterpret_cast<const unsigned long long*>(slot_u + Slots::kGate + slot_a);
                        asm("" : "+v"(gate_bits));
                        const float skip_below = __uint_as_float((uint32_t)gate_bits), opacity = __uint_as_float((uint32_t)(gate_bits >> 32));
                        // (with the second feature set there are no registers to hold an entry's colours across its early
                        // exits at eight waves per SIMD: that kernel reads them where it accumulates)
                        float2 rg = make_float2(0.f, 0.f), bz = rg;
                        uint32_t j = 0u;  // the entry's index in its batch of 64
                        if (!kExtra) {
                            asm volatile("" ::: "memory");
                            rg = *reinterpret_cast<const float2*>(slot_u + Slots::kRG + slot_a);
                            asm volatile("" ::: "memory");
                            bz = *reinterpret_cast<const float2*>(slot_u + Slots::kBZ + slot_a);
                            j = *reinterpret_cast<const uint32_t*>(tail_u);
                        }
                        // One list entry against this lane's pixel: forward.cu:331-364, same bits as
                        // -0.5f * (cxx * dx * dx + cyy * dy * dy) - cxy * dx * dy.
                        const float power = blend_power(cp, rp);
                        if (!kExtra) asm("" : "+v"(rg.x), "+v"(rg.y), "+v"(bz.x), "+v"(bz.y), "+v"(j));
                        // (one ballot per comparison: the ballot of a conjunction goes through a vector register and back)
                        const unsigned long long live = __ballot(!(power > 0.0f)) & __ballot(!(power < skip_below)) & ~done_mask;
                        if (live == 0ull) continue;
                        // From here every lane computes (a vector instruction costs the same with 1 or 64 lanes enabled);
                        // the outcome of a lane that is not live is masked out below.  All masks stay wave-uniform scalars
                        // because they are only combined in uniform control flow.
                        const float alpha = fminf(0.99f, opacity * exp_nonpositive(power));
                        const unsigned long long blends = live & __ballot(!(alpha < 1.0f / 255.0f));
                        if (blends == 0ull) continue;
                        const float test_T = T * (1.f - alpha);
                        const unsigned long long stops = blends & __ballot(test_T < 0.0001f);
                        done_mask |= stops;
                        const unsigned long long adds = blends & ~stops;
                        if (adds != 0ull && __builtin_amdgcn_inverse_ballot_w64(adds)) {
                            if (kExtra) {
                                rg = *reinterpret_cast<const float2*>(slot_u + Slots::kRG + slot_a);
                                asm volatile("" ::: "memory");
                                bz = *reinterpret_cast<const float2*>(slot_u + Slots::kBZ + slot_a);
                                const float4 e = *reinterpret_cast<const float4*>(tail_u);
                                Erg = composite2(Erg, (v2f){e.x, e.y}, alpha, T);
                                Eb = composite(Eb, e.z, alpha, T);
                                j = __float_as_uint(e.w);
                            }
                            Crg = composite2(Crg, (v2f){rg.x, rg.y}, alpha, T);
                            Cbz = composite2(Cbz, (v2f){bz.x, bz.y}, alpha, T);
                            T = test_T;
                            last = (seg_base + first + 1u) + j;
                        }
                        // Every pixel of the quadrant has stopped: the walk ends at the next slot's bound, which keeps it a loop
                        // with ONE way out (opaque, or the compiler threads the jump and pays a second exit with a state
                        // variable after every entry).
                        n = done_mask == ~0ull ? 0u : n;
                        asm("" : "+s"(n));
                    }
                }
                if (done_mask == ~0ull) goto walked;
                if (todo == 0ull) break;
            }
        }
        seg_base += count;
    }
walked:

    const bool all_done = done_mask == ~0ull;
    if (final || all_done) {
        if (inside) {
            a.out_alpha[pid] = 1.f - T;
            if (a.n_contrib != nullptr) a.n_contrib[pid] = last;
            a.out_color[pid] = Crg.x + T * a.background[0];
            a.out_color[plane + pid] = Crg.y + T * a.background[1];
            a.out_color[2 * plane + pid] = Cbz.x + T * a.background[2];
            a.out_depth[pid] = Cbz.y;
            if (kExtra) {
                a.out_extra[pid] = Erg.x + T * a.background[0];
                a.out_extra[plane + pid] = Erg.y + T * a.background[1];
                a.out_extra[2 * plane + pid] = Eb + T * a.background[2];
            }
        }
        if (!final) mark_quadrant_done(a, item);
    } else if (inside) {  // park the state for the next slab's launch (T > 0 always: the sign is free)
        const bool stopped = (done_mask >> lane) & 1ull;
        a.out_alpha[pid] = stopped ? -T : T;
        a.n_contrib[pid] = last;
        a.out_color[pid] = Crg.x;
        a.out_color[plane + pid] = Crg.y;
        a.out_color[2 * plane + pid] = Cbz.x;
        a.out_depth[pid] = Cbz.y;
        if (kExtra) {
            a.out_extra[pid] = Erg.x;
            a.out_extra[plane + pid] = Erg.y;
            a.out_extra[2 * plane + pid] = Eb;
        }
    }
    GSR_LTRACE(a.seg_begin * 40960 + blockIdx.x, 1);
}

} // namespace

hipError_t launch_blend(const Camera& cam, const BlendSegments& segs, int seg_begin, int seg_end, bool fresh, bool final,
                        const SplatRaster* raster, const float* features, const float* background, float* out_color,
                        float* out_depth, float* out_alpha, uint32_t* n_contrib, uint32_t* quad_done, uint32_t* done_rows,
                        int row_words, hipStream_t stream, const float* extra_features, float* out_extra, const BlendOrder* order) {
    BlendArgs a;
    a.W = cam.width; a.H = cam.height; a.grid_x = cam.grid_x; a.num_tiles = cam.grid_x * cam.grid_y;
    a.segs = segs; a.seg_begin = seg_begin; a.seg_end = seg_end; a.fresh = fresh ? 1 : 0; a.final = final ? 1 : 0;
    a.raster = raster; a.features = features; a.extra_features = extra_features; a.background = background;
    a.out_color = out_color; a.out_depth = out_depth; a.out_alpha = out_alpha; a.out_extra = out_extra;
    a.n_contrib = n_contrib; a.quad_done = quad_done; a.done_rows = done_rows; a.row_words = row_words;
    int blocks = 4 * a.num_tiles;
    a.order = BlendOrder{nullptr, nullptr, 0, 0, 0};
    if (order != nullptr && order->counts != nullptr) {
        a.order = *order;
        blocks = 8 * 4 * order->cap;   // every XCD gets workgroups for the largest band; the surplus leaves at once
    }
    if (extra_features != nullptr)
        hipLaunchKernelGGL(blend_quadrant_kernel<true>, dim3(blocks), dim3(64), 0, stream, a);
    else
        hipLaunchKernelGGL(blend_quadrant_kernel<false>, dim3(blocks), dim3(64), 0, stream, a);
    return hipGetLastError();
}

// counts the floats with bit patterns first_bits .. first_bits + count - 1 on which the blend's exp differs from expf
static hipError_t launch_exp_selftest(uint32_t first_bits, uint32_t count, unsigned long long* mismatches, hipStream_t stream) {
    hipLaunchKernelGGL(exp_selftest_kernel, dim3(div_up((int)count, 256)), dim3(256), 0, stream, first_bits, count, mismatches);
    return hipGetLastError();
}

} // namespace gsr

using gsr::fail;

extern "C" {

int gsr_selftest_exp(uint32_t first_bits, uint32_t count, unsigned long long* device_mismatches, void* stream_) {
    if (!device_mismatches || count > 0x7FFFFFFFu) return fail(GSR_ERR_INVALID_ARG, "bad selftest arguments");
    if (count == 0) return GSR_OK;
    GSR_HIP(gsr::launch_exp_selftest(first_bits, count, device_mismatches, (hipStream_t)stream_));
    return GSR_OK;
}

}  // extern "C"
