// One per-Gaussian tanh network (mlp.hip) whose input row lies in P arrays side by side, and optionally the block means
// of squares of those arrays: the cat in front of delta_net (model_pn.py:265-268) and magnitude_loss's head magnitudes
// (:892-901) without a cat, a slice or a reduction launch.
//
//   x[row] = (part_0[row], part_1[row], .., part_{P-1}[row]),  part_p [N][w_p],  sum_p w_p = w_0,  1 <= P <= MLP_PARTS
//   y = mlp.hip's net of x, bit for bit: the values land in the registers mlp_load_rows would put them in and run the
//       same mlp_layer / mlp_tanh.  Only the row's loader (mlp_load_parts, mlp_chain.h) differs.
//   m[j] = mean over the N rows and the block's columns of x^2, for part p's columns cut into blocks[p] equal blocks
//       (blocks[p] = 0: none of part p), j counting the blocks in the order of the parts.
//
// Forward, one launch, and a one-workgroup launch when block means are asked for.  A lane adds x^2 of its rows into
// MLP_TILES f4 accumulators over its tiles (rows past N and columns past w_0 are zeros); at the wave's end the 16 row lanes
// fold with mlp_record_layer's shuffle tree and the wave writes ONE record of w_0 column sums.  The second launch adds the
// records per column in DOUBLE, in a fixed order (16 interleaved partial sums, then a fixed tree), adds a block's columns
// in order, multiplies by 1 / (N w_p / b_p) (a double from the host) and rounds once.
//
// Backward, mlp.hip's two launches: the tile kernel runs the text of mlp_backward_body.h with the part loader and the
// part storer, then mlp.hip's mlp_finish_kernel adds the records.  The same wave-to-tile walk and record cap: every g_W /
// g_b has the bits of pigs_mlp_backward on the cat.  The block means' gradient adds no launch: where dA_0 is stored,
//   g_part_p[row][k] = dA_0[row][K_p + k] + (g_m[block] * 2 / (N w_p / b_p)) x[row][k]
// with x read back from tile 0 of the wave's LDS region (a_0, still there) and the factor from a table of w_0 floats the
// workgroup writes into LDS before the weights are staged.  Without g_m the term is not formed: every g_part has the bits
// of its slice of pigs_mlp_backward's g_x.  No float atomics anywhere.
//
// scratch (floats).  Forward with block means: min(ceil(N / 16), JOINED_FORWARD_WAVES) records of w_0.  Backward with a
// weight or bias gradient: mlp.hip's records.
#include <hip/hip_runtime.h>

#include <climits>

#include "launch.h"
#include "mlp_chain.h"

namespace pigs {

constexpr int JOINED_FORWARD_WAVES = 2048;     // as mlp.hip's forward (MLP_FORWARD_WAVES); here also the most records
constexpr int JOINED_BLOCKS = PIGS_MLP_JOINED_MAX_BLOCKS;
constexpr int MEANS_THREADS = 1024;            // the one workgroup of the means: 64 columns x 16 interleaved partial sums
static_assert(JOINED_FORWARD_WAVES % MLP_WAVES == 0 && PIGS_MLP_MAX_WIDTH <= 64, "record arithmetic");

struct MlpJoinRows {
    MlpJoin j;
    MlpPartPointers<const float> x;
};

struct MlpJoinGrads {
    MlpPartPointers<float> g;                  // null = not wanted
    const float* g_m;                          // null = zero
};

struct MlpBlocks {
    int count;                                 // sum of blocks[p]; 0 = no block means
    int start[JOINED_BLOCKS], cols[JOINED_BLOCKS];      // block j: columns start .. start + cols - 1 of the row
    float twice[JOINED_BLOCKS];                // 2 / (N cols), formed in double and rounded once: the gradient's factor
    double inv[JOINED_BLOCKS];                 // 1 / (N cols)
};

template <bool SUMS>
__global__ __launch_bounds__(64 * MLP_WAVES) void mlp_joined_forward_kernel(int64_t N, int64_t tiles, MlpNet n, MlpJoinRows in,
                                                                            float* __restrict__ y,
                                                                            float* __restrict__ sums) {
    extern __shared__ float joined_lds[];
    mlp_stage(n, joined_lds);
    f4 sq[MLP_TILES];
#pragma unroll
    for (int t = 0; t < MLP_TILES; ++t) sq[t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    mlp_forward_tiles(
        N, tiles, n, joined_lds,
        [&](f4 (&a)[MLP_TILES], int64_t row, bool live, int g) { mlp_load_parts(a, in.j, in.x, row, live, n.w[0], g); },
        [&](const f4 (&a)[MLP_TILES]) {
            if (!SUMS) return;
#pragma unroll
            for (int t = 0; t < MLP_TILES; ++t)
#pragma unroll
                for (int s = 0; s < 4; ++s) sq[t][s] = fmaf(a[t][s], a[t][s], sq[t][s]);
        },
        y, n.w[n.L]);
    if (!SUMS) return;
    // this wave's record of column sums; a wave without a tile (only past the last tile's wave) writes none
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int64_t first = (int64_t)blockIdx.x * MLP_WAVES + (threadIdx.x >> 6);
    if (first >= tiles) return;
#pragma unroll
    for (int t = 0; t < MLP_TILES; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float v = sq[t][s];
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m);      // the 16 row lanes of this g, a fixed tree
            const int k = 16 * t + 4 * g + s;
            if (r == 0 && k < n.w[0]) sums[first * n.w[0] + k] = v;
        }
}

// m from `records` records of w0 column sums, by one workgroup: thread (part, k) adds column k of records part, part + 16,
// ... in that order in double; the 16 partial sums of a column are added as a fixed tree; thread j < blocks.count adds its
// block's columns in order, multiplies by 1 / (N cols) and rounds once
__global__ __launch_bounds__(MEANS_THREADS) void mlp_joined_means_kernel(int records, int w0, MlpBlocks blocks,
                                                                         const float* __restrict__ sums,
                                                                         float* __restrict__ m) {
    __shared__ double col[MEANS_THREADS / 64][64];
    const int k = threadIdx.x & 63, part = threadIdx.x >> 6;
    double sum = 0.0;
    if (k < w0) {
#pragma unroll 8
        for (int rcd = part; rcd < records; rcd += MEANS_THREADS / 64) sum += (double)sums[(int64_t)rcd * w0 + k];
    }
    col[part][k] = sum;
    __syncthreads();
    for (int half = MEANS_THREADS / 128; half; half >>= 1) {
        if (part < half) col[part][k] += col[part + half][k];
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < JOINED_BLOCKS; ++j)
        if ((int)threadIdx.x == j && j < blocks.count) {
            double total = 0.0;
            for (int c = 0; c < blocks.cols[j]; ++c) total += col[0][blocks.start[j] + c];
            m[j] = (float)(total * blocks.inv[j]);
        }
}

__global__ __launch_bounds__(64 * MLP_WAVES) void mlp_joined_backward_kernel(int64_t N, int64_t tiles, MlpNet n, MlpGrads out,
                                                                             MlpJoinRows in, MlpJoinGrads jg, MlpBlocks blocks,
                                                                             const float* __restrict__ g_y,
                                                                             float* __restrict__ scratch) {
    extern __shared__ float joined_lds[];
    // the factor of x in a part's gradient, per column of the row; behind the waves' regions, published by mlp_stage's barrier
    float* __restrict__ factor = joined_lds + n.wave_off + MLP_WAVES * (n.L + 1) * 16 * MLP_ROW;
    if (jg.g_m && threadIdx.x < PIGS_MLP_MAX_WIDTH) {
        const int k = threadIdx.x;
        float f = 0.0f;
#pragma unroll
        for (int j = 0; j < JOINED_BLOCKS; ++j)
            if (j < blocks.count && k >= blocks.start[j] && k < blocks.start[j] + blocks.cols[j]) f = jg.g_m[j] * blocks.twice[j];
        factor[k] = f;
    }
    mlp_stage(n, joined_lds);
    const bool want_parts = jg.g.part[0] || jg.g.part[1] || jg.g.part[2] || jg.g.part[3];
    static_assert(MLP_PARTS == 4, "want_parts names every part");
#define MLP_BODY_T MLP_TILES
#define MLP_BODY_LDS joined_lds
#define MLP_BODY_LOAD_X(a, row, live, g) mlp_load_parts(a, in.j, in.x, row, live, n.w[0], g)
#define MLP_BODY_LOAD_GY(d, row, live, g) mlp_load_rows(d, g_y, row, live && g_y, n.w[n.L], n.w[n.L], g)
#define MLP_BODY_WANT_DA0 want_parts
#define MLP_BODY_STORE_DA0(d, row, live, g)                                                       \
    if (jg.g_m) {                                                                                 \
        _Pragma("unroll") for (int t = 0; t < MLP_TILES; ++t) {                                   \
            const f4 xv = *reinterpret_cast<const f4*>(acts + own + 16 * t);                      \
            const f4 fv = *reinterpret_cast<const f4*>(factor + 16 * t + 4 * g);                  \
            _Pragma("unroll") for (int s = 0; s < 4; ++s) d[t][s] = fmaf(fv[s], xv[s], d[t][s]);  \
        }                                                                                         \
    }                                                                                             \
    mlp_store_parts(jg.g, in.j, d, row, live, n.w[0], g)
#define MLP_BODY_RECORDS scratch
#include "mlp_backward_body.h"
#undef MLP_BODY_T
#undef MLP_BODY_LDS
#undef MLP_BODY_LOAD_X
#undef MLP_BODY_LOAD_GY
#undef MLP_BODY_WANT_DA0
#undef MLP_BODY_STORE_DA0
#undef MLP_BODY_RECORDS
}

// ---- host ----------------------------------------------------------------------------------------------------
static int64_t joined_sum_records(int64_t N) {
    const int64_t tiles = (N + 15) / 16;
    return tiles < JOINED_FORWARD_WAVES ? tiles : JOINED_FORWARD_WAVES;
}

static int joined_block_count(int P, const int* blocks) {
    int count = 0;
    for (int p = 0; blocks && p < P; ++p) count += blocks[p];
    return count;
}

size_t mlp_joined_scratch_bytes(int64_t N, int L, const int* widths, int P, const int* blocks, int backward) {
    if (backward) return mlp_scratch_bytes(N, L, widths);
    if (N <= 0 || !mlp_scratch_bytes(N, L, widths) || joined_block_count(P, blocks) <= 0) return 0;
    return (size_t)joined_sum_records(N) * widths[0] * sizeof(float);
}

static MlpJoin joined_describe(const MlpJoinedStep& s) {
    MlpJoin j{};
    int start = 0;
    for (int p = 0; p < MLP_PARTS; ++p) {
        const bool there = p < s.P;
        j.start[p] = there ? start : INT_MAX;
        j.width[p] = there ? s.part_widths[p] : 0;
        start += j.width[p];
    }
    j.tiles_whole = 1;
    for (int t = 0; t < MLP_TILES; ++t) {      // tile t's columns that exist: 16 t .. min(16 t + 15, w_0 - 1)
        const int lo = 16 * t, hi = s.widths[0] - 1 < lo + 15 ? s.widths[0] - 1 : lo + 15;
        int p = 0;
        while (p + 1 < s.P && j.start[p + 1] <= lo) ++p;
        if (lo <= hi && hi >= j.start[p] + j.width[p]) j.tiles_whole = 0;
        j.tile_start[t] = j.start[p];
        j.tile_width[t] = j.width[p];
    }
    return j;
}

// the parts' pointers, and with tiles_whole per tile its part's (null past the row's end)
template <class T, class V>
static MlpPartPointers<T> joined_pointers(const MlpJoinedStep& s, const MlpJoin& j, V* const* parts) {
    MlpPartPointers<T> x{};
    for (int p = 0; p < s.P; ++p) x.part[p] = parts ? (T*)parts[p] : nullptr;
    for (int t = 0; t < MLP_TILES; ++t)
        for (int p = 0; p < s.P; ++p)
            if (16 * t < s.widths[0] && j.tiles_whole && j.tile_start[t] == j.start[p]) x.tile[t] = x.part[p];
    return x;
}

static MlpJoinRows joined_rows(const MlpJoinedStep& s) {
    MlpJoinRows in{};
    in.j = joined_describe(s);
    in.x = joined_pointers<const float>(s, in.j, s.parts);
    return in;
}

static MlpBlocks joined_blocks(const MlpJoinedStep& s) {
    MlpBlocks b{};
    int start = 0;
    for (int p = 0; p < s.P; ++p) {
        const int nb = s.blocks ? s.blocks[p] : 0, cols = nb ? s.part_widths[p] / nb : 0;
        for (int j = 0; j < nb; ++j) {
            const double count = (double)s.N * (double)cols;
            b.start[b.count] = start + j * cols;
            b.cols[b.count] = cols;
            b.inv[b.count] = 1.0 / count;
            b.twice[b.count] = (float)(2.0 / count);
            ++b.count;
        }
        start += s.part_widths[p];
    }
    return b;
}

int mlp_joined_forward(const MlpJoinedStep& s, hipStream_t stream) {
    int lds_floats;
    const MlpNet n = mlp_describe(s.L, s.widths, s.weights, s.biases, &lds_floats);
    const MlpJoinRows in = joined_rows(s);
    const MlpBlocks blocks = joined_blocks(s);
    const int64_t tiles = (s.N + 15) / 16, waves = joined_sum_records(s.N);
    const unsigned groups = (unsigned)((waves + MLP_WAVES - 1) / MLP_WAVES);
    clear_hip_error();
    if (!blocks.count) {
        hipLaunchKernelGGL(mlp_joined_forward_kernel<false>, dim3(groups), dim3(64 * MLP_WAVES), lds_floats * sizeof(float),
                           stream, s.N, tiles, n, in, (float*)s.y, (float*)nullptr);
        return launch_status();
    }
    hipLaunchKernelGGL(mlp_joined_forward_kernel<true>, dim3(groups), dim3(64 * MLP_WAVES), lds_floats * sizeof(float),
                       stream, s.N, tiles, n, in, (float*)s.y, (float*)s.scratch);
    hipLaunchKernelGGL(mlp_joined_means_kernel, dim3(1), dim3(MEANS_THREADS), 0, stream, (int)waves, s.widths[0], blocks,
                       (const float*)s.scratch, (float*)s.m);
    return launch_status();
}

int mlp_joined_backward(const MlpJoinedStep& s, hipStream_t stream) {
    int lds_floats;
    const MlpNet n = mlp_describe(s.L, s.widths, s.weights, s.biases, &lds_floats);
    const MlpJoinRows in = joined_rows(s);
    const MlpBlocks blocks = joined_blocks(s);
    MlpGrads out{};
    MlpJoinGrads jg{};
    bool params = false;
    for (int l = 0; l < s.L; ++l) {
        out.g_W[l] = s.g_weights ? (float*)s.g_weights[l] : nullptr;
        out.g_b[l] = s.g_biases ? (float*)s.g_biases[l] : nullptr;
        params = params || out.g_W[l] || out.g_b[l];
    }
    jg.g = joined_pointers<float>(s, in.j, s.g_parts);
    jg.g_m = (const float*)s.g_m;
    const int64_t tiles = (s.N + 15) / 16, records = mlp_records(s.N);
    const unsigned groups = (unsigned)((records + MLP_WAVES - 1) / MLP_WAVES);
    // the images, the waves' regions, the factors
    const size_t lds = (size_t)(lds_floats + MLP_WAVES * (s.L + 1) * 16 * MLP_ROW + PIGS_MLP_MAX_WIDTH) * sizeof(float);
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)mlp_joined_backward_kernel,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            g_last_hip_error = e;
            return PIGS_ERR_LAUNCH;
        }
    }
    clear_hip_error();
    hipLaunchKernelGGL(mlp_joined_backward_kernel, dim3(groups), dim3(64 * MLP_WAVES), lds, stream, s.N, tiles, n, out, in, jg,
                       blocks, (const float*)s.g_y, (float*)s.scratch);
    if (params) mlp_finish_launch(n, out, (int)records, (const float*)s.scratch, stream);
    return launch_status();
}

}  // namespace pigs
