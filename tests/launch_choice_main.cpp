// The CPU side of the four matrix tests (tests/test_dense_matrix.py, test_aggregate_matrix.py, test_aggregate_heads_matrix.py,
// test_binned_matrix.py): the launchers' own choice functions (pigs_amd/csrc/dense_choice.h, aggregate_choice.h,
// instances.h, plan.h, build_choice.h) behind a text protocol, no GPU.  Compiled by tests/host_program.py with
// `hipcc -x hip --cuda-host-only`; reads commands from stdin, one per line, and prints one line for each:
//   D dtype d c mask N M    -> forward variant, grid, block, accumulators, can_rows, can_w16, rows chunk;
//                              backward variant, zeroed, grid x, grid y, slice            (dtype: 0 float32, 1 float64)
//   V mask                  -> covering_mask_of
//   A dtype H N L K F       -> forward / rows / cols: regions, LDS bytes, waves per Gaussian, grids; splits, the zero and
//                              the outer launch's grids; components_ok, admitted, aggregate_lds_bytes,
//                              aggregate_heads_lds_bytes, aggregate_backward_scratch_bytes
//   W N lds                 -> heads_waves_per_gaussian
//   B N                     -> the list build: all-pairs or grid
//   I dense d c | I binned c | I fused c     -> the compiled masks, in the lists' order
//   P N                     -> list_cap_for, the finest grid of make_plan_layout
//   K                       -> the constants, NAME=value
#include "../pigs_amd/csrc/aggregate_choice.h"
#include "../pigs_amd/csrc/build_choice.h"
#include "../pigs_amd/csrc/dense_choice.h"
#include "../pigs_amd/csrc/pair_math.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace pigs;

static const char* name_of(DenseForward v) {
    switch (v) {
        case DenseForward::ROWS: return "rows";
        case DenseForward::W16: return "w16";
        case DenseForward::W4: return "w4";
        case DenseForward::INVALID: return "invalid";
        default: return "nothing";
    }
}
static std::string name_of(const DenseBackwardChoice& b) {
    switch (b.variant) {
        case DenseBackward::STAGED: return "staged" + std::to_string(b.slice);
        case DenseBackward::SPLIT: return b.zero ? "split_atomic" : "split_store";
        case DenseBackward::ZERO_ONLY: return "zero_only";
        case DenseBackward::INVALID: return "invalid";
        default: return "nothing";
    }
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, sub;
        in >> cmd;
        if (cmd == "D") {
            int dtype = 0, d = 1, c = 1, mask = 1; int64_t N = 0, M = 0;
            in >> dtype >> d >> c >> mask >> N >> M;
            const int e = (int)aggregate_elem_bytes(dtype);
            const DenseForwardChoice f = choose_dense_forward(e, d, c, mask, N, M);
            const DenseBackwardChoice b = choose_dense_backward(N, M);
            printf("%s %u %u %d %d %d %d %s %d %u %u %d\n", name_of(f.variant), f.grid, f.block, fwd_accumulators(d, c, mask),
                   (int)can_rows(e, d, c, mask), (int)can_w16(e, d, c, mask), rows_chunk(e, d, c), name_of(b).c_str(), (int)b.zero, b.gx,
                   b.gy, b.slice);
        } else if (cmd == "V") {
            int mask = 0;
            in >> mask;
            printf("%d\n", covering_mask_of(mask));
        } else if (cmd == "A") {
            int dtype = 0, H = 1, L = 1, K = 1, F = 0; int64_t N = 0;
            in >> dtype >> H >> N >> L >> K >> F;
            const AggregateLaunch f = choose_aggregate_forward(dtype, H, N, L, K, F);
            const AggregateBackwardChoice b = choose_aggregate_backward(dtype, H, N, L, K, F);
            printf("%zu %zu %zu %zu %zu %zu %d %d %d %u %u %u %d %u %u %d %d %zu %zu %zu\n", forward_region(H, L, F),
                   backward_rows_region(H, K, F), backward_cols_region(H, L, K), f.lds, b.rows.lds, b.cols.lds, f.wpg, b.rows.wpg,
                   b.cols.wpg, f.grid, b.rows.grid, b.cols.grid, b.splits, b.zero_grid, b.outer_grid, (int)components_ok(H, L, K, F),
                   (int)aggregate_admitted(dtype, H, L, K, F), aggregate_lds_bytes(dtype, H, L, K, F),
                   aggregate_heads_lds_bytes(dtype, H, L, K, F), aggregate_backward_scratch_bytes(dtype, N, H, L, F));
        } else if (cmd == "W") {
            int64_t N = 0; size_t lds = 0;
            in >> N >> lds;
            printf("%d\n", heads_waves_per_gaussian(N, lds));
        } else if (cmd == "B") {
            int64_t N = 0;
            in >> N;
            printf("%s\n", aggregate_lists_all_pairs(N) ? "all-pairs" : "grid");
        } else if (cmd == "I") {
            int d = 0, c = 0;
            in >> sub;
            if (sub == "dense") in >> d >> c; else in >> c;
#define PIGS_PRINT_DENSE(MK) if (dense_compiled(d, c, MK)) printf("%d ", MK);
#define PIGS_PRINT_BINNED(MK) if (binned_compiled(c, MK)) printf("%d ", MK);
#define PIGS_PRINT_FUSED(MK) if (fused_first_compiled(c, MK)) printf("%d ", MK);
            if (sub == "dense") { PIGS_PLAIN_MASKS(PIGS_PRINT_DENSE) PIGS_DENSE_VORT_MASKS(PIGS_PRINT_DENSE) PIGS_DENSE_COUPLED_MASKS(PIGS_PRINT_DENSE) }
            else if (sub == "binned") { PIGS_PLAIN_MASKS(PIGS_PRINT_BINNED) PIGS_BINNED_C2_MASKS(PIGS_PRINT_BINNED) }
            else if (c == 1) { PIGS_FUSED_FIRST_C1_MASKS(PIGS_PRINT_FUSED) }
            else { PIGS_FUSED_FIRST_C2_MASKS(PIGS_PRINT_FUSED) }
            printf("\n");
        } else if (cmd == "P") {
            int64_t N = 0;
            in >> N;
            printf("%u %d\n", list_cap_for(N), make_plan_layout(N > 0 ? N : 1, 64, 1).G0);
        } else if (cmd == "K") {
            printf("ROWS_MAX_WORDS=%d ROWS_MAX_BLOCKS=%lld ROWS_MIN_N=%lld W16_MAX_WORDS=%d W16_BLOCKS_BELOW=%lld W16_MIN_N=%lld "
                   "STAGED_MAX_M=%lld STAGED64_MIN_WORKGROUPS=%lld ",
                   ROWS_MAX_WORDS, (long long)ROWS_MAX_BLOCKS, (long long)ROWS_MIN_N, W16_MAX_WORDS, (long long)W16_BLOCKS_BELOW,
                   (long long)W16_MIN_N, (long long)STAGED_MAX_M, (long long)STAGED64_MIN_WORKGROUPS);
            printf("AGG_BRUTE_MAX=%lld PART=%d HMAX=%d AGG_LDS_MAX=%zu AGG_LDS_DEFAULT=%zu AGG_CUS=%d AGG_WORKGROUPS_PER_CU=%d ",
                   (long long)AGG_BRUTE_MAX, PART, HMAX, AGG_LDS_MAX, AGG_LDS_DEFAULT, AGG_CUS, AGG_WORKGROUPS_PER_CU);
            printf("ORDR=%d ORDG=%d ORDV=%d ORDC=%d ORDN=%d LISTS_SMALL_TILES=%u POINTS_MODE_MIN_CELLS=%g POINTS_MODE_MIN_LIST=%u "
                   "POINTS_MODE_BLOCK_CELLS=%g POINT_HELPER_BLOCKS=%u TILE_MODE_LIST=%u TILE_MODE_RANGES=%u TILE_MODE_GROUPS=%u "
                   "TILE_MODE_POINTS=%u GRID_MARGIN=%.9g\n",
                   ORDR, ORDG, ORDV, ORDC, ORDN, LISTS_SMALL_TILES, POINTS_MODE_MIN_CELLS, POINTS_MODE_MIN_LIST, POINTS_MODE_BLOCK_CELLS,
                   POINT_HELPER_BLOCKS, TILE_MODE_LIST, TILE_MODE_RANGES, TILE_MODE_GROUPS, TILE_MODE_POINTS, (double)GRID_MARGIN);
        } else {
            printf("?\n");
        }
    }
    return 0;
}
