// gsr_wave.h -- the sums and scans over a wave64 and over a workgroup of whole waves that every kernel unit leans on, written once:
// the DPP wave scan and sum (32 and 64 bits), the xor-butterfly fold, and the workgroup sum and exclusive scan built on the first.
// Everything here is inline and lives in an unnamed namespace: each unit gets its own copy.
// What is NOT here on purpose, each for its own reason: the segmented __shfl_up scan of gsr_binning.hip (its add depends on the
// segment), every ballot-and-popcount rank (radix scatter, densify classify / scatter), gsr_backward.hip's dpp_add / fold32 /
// fold16 / row_sum_all_lanes and gsr_layerio.hip's dpp_keep (layout transforms, not sums to every lane), the fixed float tree of
// gsr_meshloss.hip (its order is the contract), and GSR_WAIT_LDS / wave_sync (two different waits).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {
namespace {

// ------------------------------------------------------------------------------------------------
// Wave64 inclusive scan and sum of one integer per lane, in six data-parallel-primitive (DPP) adds: four shifts inside
// the rows of 16 lanes (row_shr 1, 2, 4, 8), then lane 15 of rows 0 and 2 broadcast into rows 1 and 3 (row_bcast15, row
// mask 0b1010) and lane 31 into rows 2 and 3 (row_bcast31, row mask 0b1100).  A lane without a source, or in a row the
// mask leaves out, adds zero.  The __shfl_up form of the same scan costs a ds_bpermute_b32 with its address arithmetic,
// a compare and a select per step.  Every lane of the wave must be active.  Integer sums: the same result in any order.
//
// The steps are written once over a lane-move policy, so that a host program can run THESE steps on a 64-lane model
// of the moves (tests/test_wave_scan_host.py) and compare with a serial scan.
// ------------------------------------------------------------------------------------------------
constexpr int kDppRowShr = 0x110, kDppRowBcast15 = 0x142, kDppRowBcast31 = 0x143;   // dpp_ctrl encodings (gfx9)

struct WaveDpp {   // the hardware's moves: source lane's value, or zero
    template <int kCtrl, int kRowMask>
    static __device__ __forceinline__ uint32_t moved(uint32_t v) {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, kRowMask, 0xF, false);
    }
    // 64 bits: the two halves move separately (a move only carries data); the add behind it is a 64-bit add
    template <int kCtrl, int kRowMask>
    static __device__ __forceinline__ unsigned long long moved(unsigned long long v) {
        return (unsigned long long)moved<kCtrl, kRowMask>((uint32_t)v) | ((unsigned long long)moved<kCtrl, kRowMask>((uint32_t)(v >> 32)) << 32);
    }
};

template <class Moves, class T>
__host__ __device__ __forceinline__ T wave_scan_steps(T v) {
    v = v + Moves::template moved<kDppRowShr + 1, 0xF>(v);
    v = v + Moves::template moved<kDppRowShr + 2, 0xF>(v);
    v = v + Moves::template moved<kDppRowShr + 4, 0xF>(v);
    v = v + Moves::template moved<kDppRowShr + 8, 0xF>(v);
    v = v + Moves::template moved<kDppRowBcast15, 0xA>(v);
    v = v + Moves::template moved<kDppRowBcast31, 0xC>(v);
    return v;
}

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) { return wave_scan_steps<WaveDpp>(v); }
__device__ __forceinline__ unsigned long long wave_inclusive_scan(unsigned long long v) { return wave_scan_steps<WaveDpp>(v); }
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {   // to every lane
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan(v), 63);
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    v = wave_inclusive_scan(v);
    return (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63) |
           ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63) << 32);
}

// The xor butterfly: v = op(v, the value 32, 16, ... 1 lanes across), the result in every lane.  For uint32_t, unsigned long long
// and float.  The pairing is fixed, so a float fold gives the same bits wherever it is called; a float sum never goes through the
// DPP scan above, whose order is another one.  (Shuffles: a lane that is off contributes whatever its register holds.)
template <class T, class Op>
__device__ __forceinline__ T wave_fold(T v, Op op) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d, 64));
    return v;
}

// Sum over the workgroup's kWaves * 64 lanes (32 or 64 bits), returned to every lane; s_wave is kWaves words of LDS of the value's
// type.  Every lane of the workgroup must be active; both barriers are inside, so s_wave is free again on return.
template <int kWaves = 4, class T>
__device__ __forceinline__ T block_sum(T v, T* s_wave) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    T total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) total += s_wave[w];
    __syncthreads();
    return total;
}

// Scan of one value per lane over the workgroup; returns the exclusive prefix, *total = sum of all (to every lane).  As block_sum.
template <int kWaves = 4, class T>
__device__ __forceinline__ T block_exclusive_scan(T mine, T* s_wave, T* total = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_inclusive_scan(mine);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    T before = incl - mine, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) before += s_wave[w];
        all += s_wave[w];
    }
    __syncthreads();
    if (total) *total = all;
    return before;
}

} // namespace
} // namespace gsr
