// The aggregation's launch rules (aggregate.hip): sizes, occupancy and grids as pure functions of the problem.  No
// device code, no HIP call, no environment.  The four sampling launchers and aggregate_lists_t take every number from
// here, capi.hip its size rule, and tests/launch_choice_main.cpp puts the same functions in front of the CPU tests, so
// each rule is stated exactly once.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/pigs_amd.h"

namespace pigs {

constexpr int64_t AGG_BRUTE_MAX = 2048;          // up to here the list build tests every pair; beyond, it walks the grid
constexpr int PART = 136;                        // values of a wave's partial result: 128 components + scalars
constexpr int HMAX = PIGS_AGGREGATE_HEADS_MAX;
constexpr size_t AGG_LDS_MAX = 160 * 1024;       // LDS of a gfx950 CU: what one workgroup can ask for
constexpr size_t AGG_LDS_DEFAULT = 64 * 1024;    // beyond, the launch has to ask for it (hipFuncSetAttribute)
constexpr int AGG_CUS = 256;                     // compute units of an MI355X (the one device this library is built for)
constexpr int AGG_WORKGROUPS_PER_CU = 8;         // 32 waves a CU: eight workgroups of four

inline bool aggregate_lists_all_pairs(int64_t N) { return N <= AGG_BRUTE_MAX; }
inline size_t aggregate_elem_bytes(int dtype) { return dtype == PIGS_F64 ? 8 : 4; }

// A wave's region, in values: the forward parks [features_j ; 4F sin / cos] and merges H partials; the backward by rows
// keeps H dacc blocks and parks [H K keys ; F]; the backward by columns parks H (L + K) values.
inline size_t rows_region(int stride) { return (size_t)(64 * stride > PART ? 64 * stride : PART); }
inline size_t forward_region(int H, int L, int F) {
    const size_t r = rows_region((L + 4 * F) | 1);
    return r > (size_t)H * PART ? r : (size_t)H * PART;
}
inline size_t backward_rows_region(int H, int K, int F) { return (size_t)H * PART + rows_region((H * K + F) | 1); }
inline size_t backward_cols_region(int H, int L, int K) { return rows_region((H * (L + K)) | 1); }
// LDS of a sampling kernel: four wave regions of `region` values
inline size_t sampling_lds_bytes(int dtype, size_t region) { return aggregate_elem_bytes(dtype) * 4 * region; }
// the most dynamic LDS any of the three sampling kernels asks for at these sizes (a CU has AGG_LDS_MAX = 160 KB)
inline size_t aggregate_lds_bytes(int dtype, int H, int L, int K, int F) {
    const size_t a = forward_region(H, L, F), b = backward_rows_region(H, K, F), c = backward_cols_region(H, L, K);
    return sampling_lds_bytes(dtype, a > b ? (a > c ? a : c) : (b > c ? b : c));
}
// THE size rule of every sampling entry point, in one place: 1 <= H <= HMAX, at most 128 components per kernel (two per
// lane) and every kernel's LDS within a CU's.  A shape is admitted when neither H nor a component count is out of
// range and aggregate_lds_bytes <= AGG_LDS_MAX.  Anything beyond is refused, not attempted.
inline bool components_ok(int H, int L, int K, int F) {
    return H >= 1 && H <= HMAX && L + 2 * (4 * F + 1) <= 128 && H * K + F <= 128 && H * (L + K) <= 128;
}
inline size_t aggregate_heads_lds_bytes(int dtype, int H, int L, int K, int F) {      // 0: H or a component count out of range
    return components_ok(H, L, K, F) ? aggregate_lds_bytes(dtype, H, L, K, F) : 0;
}
inline bool aggregate_admitted(int dtype, int H, int L, int K, int F) {
    return components_ok(H, L, K, F) && aggregate_lds_bytes(dtype, H, L, K, F) <= AGG_LDS_MAX;
}
inline size_t aggregate_backward_scratch_bytes(int dtype, int64_t N, int H, int L, int F) {
    const int W = L + 2 * (4 * F + 1);
    // dacc [N][H][W], D [N][H], per-row d frequencies [N][F]; a multiple of 256 bytes
    return (aggregate_elem_bytes(dtype) * (size_t)N * (size_t)(H * (W + 1) + F) + 255) / 256 * 256;
}

// Waves per Gaussian, one head: a launch of few Gaussians is one generation of waves bound by a wave's serial life
// (split every Gaussian's rounds over four waves); many Gaussians are a throughput problem (no idle waves)
inline int waves_per_gaussian(int64_t N) { return N <= 4096 ? 4 : N <= 8192 ? 2 : 1; }

// Waves per Gaussian, H >= 2.  Up to AGG_BRUTE_MAX Gaussians (the model's sizes) a launch is bound by a wave's serial
// life, and several heads ask for more LDS than one, so fewer of their workgroups are resident at once: the waves per
// Gaussian are halved while the launch's workgroups exceed what the device holds (AGG_CUS compute units, per CU what
// the LDS request admits, at most the eight workgroups of 32 waves).
// What stands behind the rule is ONE sweep (profiles/aggregate_heads.txt "waves per Gaussian"):
// the model's shape, H = 2, N = 1 600, 4 / 2 / 1 waves, float32 and float64.  There it picks 1 wave for all three
// kernels in both dtypes; that is the best or within 1 us of it for the kernel by rows and for float64's forward and
// rows, and it passes over the better 2-wave launch of float32's forward (25.5 against 27.9 us), float32's columns
// (60.1 against 65.5) and float64's columns (117.7 against 123.9): 800 workgroups against 768 resident.  It is
// applied unmeasured to H = 3, 4 and to other shapes.  Beyond AGG_BRUTE_MAX: the one-head rule, as measured there.
// It stays keyed on H: applied to H = 1 it would halve the waves at the model's N = 1 600 (1 600 workgroups against
// 768 resident).
inline int heads_waves_per_gaussian(int64_t N, size_t lds_bytes) {
    int wpg = waves_per_gaussian(N);
    if (N > AGG_BRUTE_MAX) return wpg;
    size_t per_cu = AGG_LDS_MAX / (lds_bytes > 0 ? lds_bytes : 1);
    per_cu = per_cu > (size_t)AGG_WORKGROUPS_PER_CU ? (size_t)AGG_WORKGROUPS_PER_CU : per_cu < 1 ? 1 : per_cu;
    const int64_t resident = (int64_t)AGG_CUS * (int64_t)per_cu;
    while (wpg > 1 && (N * wpg + 3) / 4 > resident) wpg >>= 1;
    return wpg;
}

// the sums over N of the backward: one split per ~2048 Gaussians (a single split is a plain, deterministic sum; more
// add their partial sums atomically into outputs that a zero launch cleared)
inline int aggregate_splits(int64_t N) {
    const int64_t s = (N + 2047) / 2048;
    return (int)(s < 1 ? 1 : s > 64 ? 64 : s);
}

// One sampling kernel's launch: its dynamic LDS, the waves that share a Gaussian, and the grid of four-wave workgroups
struct AggregateLaunch {
    size_t lds;
    int wpg;
    unsigned grid;
};
inline AggregateLaunch aggregate_launch(int dtype, int H, int64_t N, size_t region) {
    AggregateLaunch k;
    k.lds = sampling_lds_bytes(dtype, region);
    k.wpg = H == 1 ? waves_per_gaussian(N) : heads_waves_per_gaussian(N, k.lds);
    const int gpw = 4 / k.wpg;
    k.grid = (unsigned)((N + gpw - 1) / gpw);
    return k;
}
inline AggregateLaunch choose_aggregate_forward(int dtype, int H, int64_t N, int L, int K, int F) {
    (void)K;
    return aggregate_launch(dtype, H, N, forward_region(H, L, F));
}
struct AggregateBackwardChoice {
    AggregateLaunch rows, cols;
    int splits;
    unsigned zero_grid;       // of aggregate_zero_kernel, launched when splits > 1
    unsigned outer_grid;      // of the outer-product kernel: a workgroup per (column, split)
};
inline AggregateBackwardChoice choose_aggregate_backward(int dtype, int H, int64_t N, int L, int K, int F) {
    const int E = 4 * F + 1, W = L + 2 * E;
    AggregateBackwardChoice b;
    b.rows = aggregate_launch(dtype, H, N, backward_rows_region(H, K, F));
    b.cols = aggregate_launch(dtype, H, N, backward_cols_region(H, L, K));
    b.splits = aggregate_splits(N);
    const int64_t mx = (int64_t)H * L * (2 * E > L ? 2 * E : L);
    b.zero_grid = (unsigned)((mx + 255) / 256);
    b.outer_grid = (unsigned)((H * W + F) * b.splits);
    return b;
}

}  // namespace pigs
