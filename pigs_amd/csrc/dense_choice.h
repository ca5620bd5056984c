// Which kernel a dense launch takes (dense.hip): a pure function of the instantiation and the sizes.  No device code,
// no HIP call, no environment: launch_dense_forward / launch_dense_backward ask here, and tests/launch_choice_main.cpp
// puts the same functions in front of the CPU tests, so every threshold below is stated exactly once.
#pragma once
#include <stdint.h>

#include "instances.h"

namespace pigs {

// ---- the rows forward (few points): a workgroup of ROWS_WAVES waves takes 16 points, the Gaussians come through LDS
constexpr int ROWS_WAVES = 8;
constexpr int ROWS_CHUNK_BYTES = 36 * 1024;      // Gaussian parameters staged per chunk (1 536 Gaussians of d = 2, c = 1, float32)
constexpr int rows_chunk(int elem_bytes, int d, int c) { return ROWS_CHUNK_BYTES / ((d + d * (d + 1) / 2 + c) * elem_bytes); }

// FwdLayout<D, C, MASK>::N (pair_math.h) as a function: the accumulators of a forward lane (dense.hip asserts the two equal)
constexpr int fwd_accumulators(int d, int c, int mask) {
    const int nf = d * (d + 1) / 2, n3 = d * (d + 1) * (d + 2) / 6;
    const int m = mask == MASK_TERMS ? 19 : mask == MASK_COUPLED ? 17 : mask;      // u, grad u, trace; u and the trace
    return ((m & 1) ? c : 0) + ((m & 2) ? d * c : 0) + ((m & 4) ? nf * c : (m & 16) ? c : 0) + ((m & 8) ? n3 * c : 0) +
           ((m & MASK_RESIDUAL) ? c : 0) + ((m == MASK_VORTICITY || m == MASK_VORT_RESIDUAL || m == MASK_VORT_FIT) ? 7 : 0) +
           (m == MASK_NET_INPUTS ? 5 * c : m == MASK_NET_INPUTS_NS ? 13 : 0);      // u, grad u, u_xx, u_yy; + w_x, w_y, lap w
}

// ---- forward
constexpr int ROWS_MAX_WORDS = 28;               // accumulator words (4 bytes): beyond, the two records in flight spill even at 256 VGPRs
constexpr int64_t ROWS_MAX_BLOCKS = 256;         // 64-point blocks up to which rows spreads the Gaussians over the chip
constexpr int64_t ROWS_MIN_N = 128;
// sixteen waves: a 1 024-thread workgroup leaves 128 VGPRs per wave: the wide accumulator sets -- several channels,
// third derivatives, float64 -- spilled there, so they keep the four-wave variant
constexpr int W16_MAX_WORDS = 7;
constexpr int W16_MAX_LDS_BYTES = 60 * 1024;     // 15 waves' accumulators meet wave 0 in LDS
constexpr int64_t W16_BLOCKS_BELOW = 1024;
constexpr int64_t W16_MIN_N = 64;
constexpr int64_t GRID_X_MAX = 0x7fffffffLL, GRID_Y_MAX = 65535;
constexpr bool can_rows(int elem_bytes, int d, int c, int mask) { return fwd_accumulators(d, c, mask) * (elem_bytes / 4) <= ROWS_MAX_WORDS; }
constexpr bool can_w16(int elem_bytes, int d, int c, int mask) {
    return 15 * fwd_accumulators(d, c, mask) * 64 * elem_bytes <= W16_MAX_LDS_BYTES &&
           fwd_accumulators(d, c, mask) * (elem_bytes / 4) <= W16_MAX_WORDS;
}

enum class DenseForward { NOTHING, INVALID, ROWS, W16, W4 };      // NOTHING: no points; INVALID: more blocks than a grid holds
struct DenseForwardChoice {
    DenseForward variant;
    unsigned grid, block;
};
inline DenseForwardChoice choose_dense_forward(int elem_bytes, int d, int c, int mask, int64_t N, int64_t M) {
    const int64_t blocks = (M + 63) / 64;
    if (blocks == 0) return {DenseForward::NOTHING, 0, 0};
    if (blocks > GRID_X_MAX) return {DenseForward::INVALID, 0, 0};
    // few points (<= 256 of the 64-point blocks): 16 points per workgroup, the Gaussians in 32 slices
    if (can_rows(elem_bytes, d, c, mask) && blocks <= ROWS_MAX_BLOCKS && N >= ROWS_MIN_N)
        return {DenseForward::ROWS, (unsigned)((M + 15) / 16), 64 * ROWS_WAVES};
    // few point blocks: spread the Gaussian loop over 16 waves per workgroup
    if (can_w16(elem_bytes, d, c, mask) && blocks < W16_BLOCKS_BELOW && N >= W16_MIN_N)
        return {DenseForward::W16, (unsigned)blocks, 1024};
    return {DenseForward::W4, (unsigned)blocks, 256};
}

// ---- backward
constexpr int64_t STAGED_MAX_M = 16384;                // few points: 64-point slices staged in LDS, 256 Gaussians per workgroup
constexpr int64_t STAGED64_MIN_WORKGROUPS = 512;       // below, 32-point slices: 64 would leave most of the chip without a workgroup
constexpr int64_t SPLIT_WORKGROUPS = 2048;             // the split backward slices the points until about this many workgroups exist
constexpr uint64_t ZERO_MAX_BLOCKS = 2048;             // of zero_grads_kernel (1 024 words a block, grid-stride beyond)

enum class DenseBackward { NOTHING, INVALID, ZERO_ONLY, STAGED, SPLIT };      // ZERO_ONLY: no points, the gradients are zero
struct DenseBackwardChoice {
    DenseBackward variant;
    bool zero;            // the gradient buffers are zeroed first: the kernel adds into them
    unsigned gx, gy;
    int slice;            // STAGED: points per slice
};
inline DenseBackwardChoice choose_dense_backward(int64_t N, int64_t M) {
    const int64_t gblocks = (N + 63) / 64;
    if (gblocks == 0) return {DenseBackward::NOTHING, false, 0, 0, 0};
    if (gblocks > GRID_X_MAX) return {DenseBackward::INVALID, false, 0, 0, 0};
    if (M == 0) return {DenseBackward::ZERO_ONLY, true, 0, 0, 0};
    if (M <= STAGED_MAX_M && (M + 63) / 64 <= GRID_Y_MAX) {
        const int64_t gx = (N + 255) / 256;
        const int slice = gx * ((M + 63) / 64) < STAGED64_MIN_WORKGROUPS ? 32 : 64;      // N = 1 600, 1 024 points: 112 workgroups of 64-point slices
        return {DenseBackward::STAGED, true, (unsigned)gx, (unsigned)((M + slice - 1) / slice), slice};
    }
    // split the point range over gridDim.y so that ~2048 workgroups exist; each wave should still see >= 64 points
    int64_t ysplit = SPLIT_WORKGROUPS / gblocks;
    const int64_t max_split = (M + 4 * 64 - 1) / (4 * 64);
    if (ysplit > max_split) ysplit = max_split;
    if (ysplit < 1) ysplit = 1;
    if (ysplit > GRID_Y_MAX) ysplit = GRID_Y_MAX;
    return {DenseBackward::SPLIT, ysplit > 1, (unsigned)gblocks, (unsigned)ysplit, 0};
}

}  // namespace pigs
