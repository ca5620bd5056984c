// The register-resident tanh chain on v_mfma_f32_16x16x4_f32, shared by mlp.hip (one per-Gaussian net per launch),
// mlp_bank.hip (several nets of one shape over one input per launch), mlp_joined.hip (one net whose input row lies in
// several arrays) and input_transform.hip (the latent net, whose rows
// are gathered from eight arrays and summed instead of stored).  It holds
// the backward as well: one layer's three products (mlp_backward_layer) and its part of a wave's record
// (mlp_record_layer), which mlp.hip instantiates at the widest net and input_transform.hip at the latent net's tile
// counts.  The operand layout and the padded LDS images are described at the head of mlp.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "launch.h"

namespace pigs {

constexpr int MLP_TILES = PIGS_MLP_MAX_WIDTH / 16;      // 16-feature tiles of the widest layer
constexpr int MLP_WAVES = 4;                            // waves (row tiles in flight) per workgroup
constexpr int MLP_ROW = PIGS_MLP_MAX_WIDTH + 4;         // floats per row of a wave's [16][.] LDS tile: 16-byte rows
static_assert(PIGS_MLP_MAX_WIDTH % 16 == 0 && PIGS_MLP_MAX_RECORDS % MLP_WAVES == 0, "tile arithmetic");

typedef float f4 __attribute__((ext_vector_type(4)));

struct MlpNet {
    int L, P;                                  // layers; floats per record
    int w[PIGS_MLP_MAX_LAYERS + 1];            // widths
    int woff[PIGS_MLP_MAX_LAYERS];             // LDS float offsets: layer l's weights [pad(w[l+1])][pad(w[l]) + 4]
    int boff[PIGS_MLP_MAX_LAYERS];             //   and its bias [pad(w[l+1])]
    int poff[PIGS_MLP_MAX_LAYERS];             // record float offsets: dW_l [w[l+1]][w[l]], then db_l [w[l+1]]
    int wave_off;                              // LDS float offset of the waves' regions (backward): (L + 1) tiles each
    const float* W[PIGS_MLP_MAX_LAYERS];
    const float* b[PIGS_MLP_MAX_LAYERS];
};

struct MlpGrads {
    float* g_x;                                // null = not wanted
    float* g_W[PIGS_MLP_MAX_LAYERS];
    float* g_b[PIGS_MLP_MAX_LAYERS];
};

// a row that is up to MLP_PARTS arrays side by side (mlp_joined.hip; mlp_load_parts below).  The host also says whether
// every 16-column tile's columns lie in ONE part, and which: the kernels then take each tile as mlp_load_rows would, from
// an address that is a kernel argument of its own.  (Found in the kernel by compares, the part became an index into the
// kernel's argument arrays: two dependent scalar loads per tile, waited for at one wave per SIMD.)
constexpr int MLP_PARTS = PIGS_MLP_JOINED_MAX_PARTS;
struct MlpJoin {
    int start[MLP_PARTS];                      // part p's first column in the row; INT_MAX for a part that is not there
    int width[MLP_PARTS];                      //   and its columns (0)
    int tiles_whole;                           // every 16-column tile lies in one part (or past the row's end)
    int tile_start[MLP_TILES];                 //   then: the first column of tile t's part
    int tile_width[MLP_TILES];                 //   and that part's columns
};

template <class T>
struct MlpPartPointers {
    T* part[MLP_PARTS];                        // null: a part that is not there, or not wanted
    T* tile[MLP_TILES];                        // with tiles_whole: the part of tile t
};

__host__ __device__ constexpr int mlp_tiles(int width) { return (width + 15) >> 4; }

// the net's description and the LDS floats of the weight and bias images
inline MlpNet mlp_describe(int L, const int* widths, const void* const* weights, const void* const* biases,
                           int* lds_floats) {
    MlpNet n{};
    n.L = L;
    int off = 0, p = 0;
    for (int l = 0; l <= L; ++l) n.w[l] = widths[l];
    for (int l = 0; l < L; ++l) {
        const int ip = 16 * mlp_tiles(n.w[l]), op = 16 * mlp_tiles(n.w[l + 1]);
        n.woff[l] = off;
        off += op * (ip + 4);
        n.boff[l] = off;
        off += op;
        n.poff[l] = p;
        p += n.w[l + 1] * (n.w[l] + 1);
        n.W[l] = (const float*)weights[l];
        n.b[l] = (const float*)biases[l];
    }
    n.P = p;
    n.wave_off = off;
    *lds_floats = off;
    return n;
}

// mlp.hip: the backward's records (one per wave, at most PIGS_MLP_MAX_RECORDS) and the floats of one; the launch that
// adds `records` records of n.P floats in a fixed order into out.g_W / out.g_b
int64_t mlp_records(int64_t N);
int mlp_record_floats(int L, const int* widths);
void mlp_finish_launch(const MlpNet& n, const MlpGrads& out, int records, const float* scratch, hipStream_t stream);

#if defined(__HIPCC__)
// orders this wave's LDS accesses for the compiler: lanes exchange data through LDS without a workgroup barrier (the
// LDS serves one wave's instructions in order)
__device__ __forceinline__ void mlp_wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the padded weight and bias images, by the whole workgroup
// A loop per layer over the padded image in chunks of 16 columns; every load is unconditional (a pad element reads
// element 0 and is replaced by zero), so that the loads of an unrolled body are issued together.  (Measured and dropped:
// ONE loop over the floats of all images with the layer found per element -- delta_net's forward at N = 1 600 took 18.4
// us against 16.5 us with a loop per layer.)
// (Ws, bs: the L weight and bias arrays -- n's own, or those of one net of a bank of n's shape, mlp_bank.hip)
__device__ __forceinline__ void mlp_stage(const MlpNet& n, const float* const* Ws, const float* const* bs,
                                          float* __restrict__ lds) {
    for (int l = 0; l < n.L; ++l) {
        const int in = n.w[l], out = n.w[l + 1], nti = mlp_tiles(in), op = 16 * mlp_tiles(out), S = 16 * nti + 4;
        const float* __restrict__ W = Ws[l];
        const float* __restrict__ b = bs[l];
        float* __restrict__ dst = lds + n.woff[l];
#pragma unroll 4
        for (int idx = threadIdx.x; idx < op * nti * 16; idx += 64 * MLP_WAVES) {
            const int chunk = idx >> 4, o = nti == 1 ? chunk : nti == 2 ? chunk >> 1 : chunk / 3;
            const int k = 16 * (chunk - o * nti) + (idx & 15);
            const bool real = o < out && k < in;
            const float v = W[real ? o * in + k : 0];
            dst[o * S + k] = real ? v : 0.0f;
        }
        for (int o = threadIdx.x; o < op; o += 64 * MLP_WAVES) lds[n.boff[l] + o] = o < out ? b[o] : 0.0f;
    }
    __syncthreads();
}

__device__ __forceinline__ void mlp_stage(const MlpNet& n, float* __restrict__ lds) { mlp_stage(n, n.W, n.b, lds); }

// a tile of 16 rows of `width` floats, `stride` floats apart ([N][width]: stride = width), in the accumulator layout:
// lane (r, g) holds features 16 t + 4 g + 0..3 of row r; rows past N and features past the width are zeros
__device__ __forceinline__ void mlp_load_rows(f4 (&a)[MLP_TILES], const float* __restrict__ src, int64_t row, bool live,
                                              int width, int stride, int g) {
#pragma unroll
    for (int t = 0; t < MLP_TILES; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = 16 * t + 4 * g + s;
            a[t][s] = (live && k < width) ? src[row * stride + k] : 0.0f;
        }
}

__device__ __forceinline__ void mlp_store_rows(float* __restrict__ dst, const f4 (&a)[MLP_TILES], int64_t row, bool live,
                                               int width, int stride, int g) {
#pragma unroll
    for (int t = 0; t < MLP_TILES; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = 16 * t + 4 * g + s;
            if (live && k < width) dst[row * stride + k] = a[t][s];
        }
}

// The same two for a row that is MLP_PARTS arrays side by side (mlp_joined.hip): part p is [N][width[p]] and holds
// columns start[p] .. start[p] + width[p] - 1 of the row.  Where every 16-column tile lies in ONE part (the model's
// (16, 32)), a row is loaded and stored as mlp_load_rows / mlp_store_rows would, each tile from its own pointer, all loads
// of a row in one basic block so that they are in flight together.  Otherwise every element chooses its part by compares
// against the parts' bounds: a lane's four columns may lie in two parts.  There a lane forms its row's address in each
// part once (the column's start taken off), and a column costs the selects and one add.  (Its four addresses are scalars,
// not an array: an array is kept in scratch memory and indexed.)
static_assert(MLP_PARTS == 4, "mlp_part_of names every part");
template <class T>
__device__ __forceinline__ T* mlp_part_of(int k, const MlpJoin& j, T* at0, T* at1, T* at2, T* at3) {
    T* p = at0;
    p = k >= j.start[1] ? at1 : p;
    p = k >= j.start[2] ? at2 : p;
    p = k >= j.start[3] ? at3 : p;
    return p;
}

// where column 0 of the row would lie if a part of `width` columns from column `start` on ran on from it: the
// result[k] is column k of the row; null stays null
template <class T>
__device__ __forceinline__ T* mlp_part_row(T* base, int width, int start, int64_t row) {
    return base ? base + (row * width - start) : nullptr;
}

__device__ __forceinline__ void mlp_load_parts(f4 (&a)[MLP_TILES], const MlpJoin& j, const MlpPartPointers<const float>& x,
                                               int64_t row, bool live, int width, int g) {
    if (j.tiles_whole) {
#pragma unroll
        for (int t = 0; t < MLP_TILES; ++t) {
            const float* const at = mlp_part_row(x.tile[t], j.tile_width[t], j.tile_start[t], row);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = 16 * t + 4 * g + s;
                a[t][s] = (live && k < width) ? at[k] : 0.0f;
            }
        }
        return;
    }
    const float* const at0 = mlp_part_row(x.part[0], j.width[0], 0, row);
    const float* const at1 = mlp_part_row(x.part[1], j.width[1], j.start[1], row);
    const float* const at2 = mlp_part_row(x.part[2], j.width[2], j.start[2], row);
    const float* const at3 = mlp_part_row(x.part[3], j.width[3], j.start[3], row);
#pragma unroll
    for (int t = 0; t < MLP_TILES; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = 16 * t + 4 * g + s;
            a[t][s] = (live && k < width) ? mlp_part_of(k, j, at0, at1, at2, at3)[k] : 0.0f;
        }
}

// a null pointer: that part is not written
__device__ __forceinline__ void mlp_store_parts(const MlpPartPointers<float>& dst, const MlpJoin& j, const f4 (&a)[MLP_TILES],
                                                int64_t row, bool live, int width, int g) {
    if (j.tiles_whole) {
#pragma unroll
        for (int t = 0; t < MLP_TILES; ++t) {
            float* const at = mlp_part_row(dst.tile[t], j.tile_width[t], j.tile_start[t], row);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = 16 * t + 4 * g + s;
                if (live && k < width && at) at[k] = a[t][s];
            }
        }
        return;
    }
    float* const at0 = mlp_part_row(dst.part[0], j.width[0], 0, row);
    float* const at1 = mlp_part_row(dst.part[1], j.width[1], j.start[1], row);
    float* const at2 = mlp_part_row(dst.part[2], j.width[2], j.start[2], row);
    float* const at3 = mlp_part_row(dst.part[3], j.width[3], j.start[3], row);
#pragma unroll
    for (int t = 0; t < MLP_TILES; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = 16 * t + 4 * g + s;
            float* const p = mlp_part_of(k, j, at0, at1, at2, at3);
            if (live && k < width && p) p[k] = a[t][s];
        }
}

// z = a W^T + b for one layer; W, bias: the layer's LDS images, S the image's row stride
__device__ __forceinline__ void mlp_layer(f4 (&z)[MLP_TILES], const f4 (&a)[MLP_TILES], const float* __restrict__ W,
                                          const float* __restrict__ bias, int S, int nti, int nto, int r, int g) {
#pragma unroll
    for (int to = 0; to < MLP_TILES; ++to) {
        f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        if (to < nto) {
            acc = *reinterpret_cast<const f4*>(bias + 16 * to + 4 * g);
#pragma unroll
            for (int ti = 0; ti < MLP_TILES; ++ti)
                if (ti < nti) {
                    const f4 w = *reinterpret_cast<const f4*>(W + (16 * to + r) * S + 16 * ti + 4 * g);
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[s], a[ti][s], acc, 0, 0, 0);
                }
        }
        z[to] = acc;
    }
}

__device__ __forceinline__ void mlp_tanh(f4 (&a)[MLP_TILES], const f4 (&z)[MLP_TILES]) {
#pragma unroll
    for (int t = 0; t < MLP_TILES; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s) a[t][s] = tanhf(z[t][s]);
}

// One layer of the backward on a wave's tile (the three products at the head of mlp.hip).  NTO x NTI are the tile counts
// of the accumulators, fixed at compile time so that a net of known widths holds the registers it needs and no more;
// nto <= NTO and nti <= NTI are the layer's real counts.  d: dZ_l on entry; on exit dZ_{l-1}, or dA_0 when `first`.
// a_l: the layer's input in this wave's LDS region as [row][feature]; dz_t: the tile dZ_l passes through; own: where this
// lane's four features of feature tile 0 lie in a tile.
template <int NTO, int NTI>
__device__ __forceinline__ void mlp_backward_layer(f4 (&d)[MLP_TILES], f4 (&acc_w)[NTO][NTI], f4 (&acc_b)[NTO], bool want_w,
                                                   bool want_b, bool want_da, bool first, const float* __restrict__ W, int nto,
                                                   int nti, const float* __restrict__ a_l, float* __restrict__ dz_t, int own,
                                                   int r, int g) {
    const int S = 16 * nti + 4;
    if (want_b) {
#pragma unroll
        for (int to = 0; to < NTO; ++to) acc_b[to] += d[to];
    }
    if (want_w) {                              // dW += dZ^T a: the row sits on the lane in both, dZ goes through LDS
        mlp_wave_fence();
#pragma unroll
        for (int t = 0; t < NTO; ++t) *reinterpret_cast<f4*>(dz_t + own + 16 * t) = d[t];
        mlp_wave_fence();
        f4 at[NTI];
#pragma unroll
        for (int ti = 0; ti < NTI; ++ti)
#pragma unroll
            for (int s = 0; s < 4; ++s) at[ti][s] = ti < nti ? a_l[(4 * s + g) * MLP_ROW + 16 * ti + r] : 0.0f;
#pragma unroll
        for (int to = 0; to < NTO; ++to)
            if (to < nto) {
                f4 dt;
#pragma unroll
                for (int s = 0; s < 4; ++s) dt[s] = dz_t[(4 * s + g) * MLP_ROW + 16 * to + r];
#pragma unroll
                for (int ti = 0; ti < NTI; ++ti)
                    if (ti < nti) {
#pragma unroll
                        for (int s = 0; s < 4; ++s)
                            acc_w[to][ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(dt[s], at[ti][s], acc_w[to][ti], 0, 0, 0);
                    }
            }
    }
    if (!want_da) return;
    f4 da[NTI];                                // dA^T = W^T dZ^T: the image read down a column
#pragma unroll
    for (int ti = 0; ti < NTI; ++ti) {
        f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        if (ti < nti) {
#pragma unroll
            for (int to = 0; to < NTO; ++to)
                if (to < nto) {
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(W[(16 * to + 4 * g + s) * S + 16 * ti + r], d[to][s], acc, 0,
                                                                   0, 0);
                }
        }
        da[ti] = acc;
    }
#pragma unroll
    for (int t = NTI; t < MLP_TILES; ++t) d[t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ti = 0; ti < NTI; ++ti) {
        if (first) {
            d[ti] = da[ti];
        } else {
            const f4 al = *reinterpret_cast<const f4*>(a_l + own + 16 * ti);
#pragma unroll
            for (int s = 0; s < 4; ++s) d[ti][s] = da[ti][s] * fmaf(-al[s], al[s], 1.0f);
        }
    }
}

// A layer's part of the wave's record, which starts at rec[base]: dW [out][in], then db [out].  An index is the lane's
// part (o, r), the same in every tile and layer, plus the tiles' part, which is uniform: mlp.hip's kernel writes its
// record with every accumulator still live, and has no registers for a lane's index per tile.
template <int NTO, int NTI>
__device__ __forceinline__ void mlp_record_layer(float* __restrict__ rec, int base, const f4 (&acc_w)[NTO][NTI],
                                                 const f4 (&acc_b)[NTO], bool want_w, bool want_b, int in, int outw, int r,
                                                 int g) {
    if (want_w) {
#pragma unroll
        for (int to = 0; to < NTO; ++to)
#pragma unroll
            for (int ti = 0; ti < NTI; ++ti)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int o = 4 * g + s;      // element [o][r] of tile (to, ti)
                    if (o < outw - 16 * to && r < in - 16 * ti)
                        rec[base + 16 * (to * in + ti) + o * in + r] = acc_w[to][ti][s];
                }
    }
    if (want_b) {
#pragma unroll
        for (int to = 0; to < NTO; ++to)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                float v = acc_b[to][s];
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m);      // the 16 row lanes of this g, a fixed tree
                const int o = 4 * g + s;
                if (r == 0 && o < outw - 16 * to) rec[base + outw * in + 16 * to + o] = v;
            }
    }
}

// ---- the bodies of mlp.hip's three kernels, shared with mlp_bank.hip (one net of a bank per workgroup) ------------
// The forward of the staged net over this workgroup's tiles: tile = blockIdx.x * MLP_WAVES + wave, + the grid's waves,
// ...  Rows of y lie y_stride floats apart (one net: w_L).  load(a, row, live, g) brings a_0 in mlp_load_rows's layout;
// seen(a) is called with it once per tile (mlp_joined.hip adds its squares there).
template <class Load, class Seen>
__device__ __forceinline__ void mlp_forward_tiles(int64_t N, int64_t tiles, const MlpNet& n, const float* __restrict__ lds,
                                                  Load load, Seen seen, float* __restrict__ y, int y_stride) {
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int64_t stride = (int64_t)gridDim.x * MLP_WAVES;
    for (int64_t tile = (int64_t)blockIdx.x * MLP_WAVES + (threadIdx.x >> 6); tile < tiles; tile += stride) {
        const int64_t row = tile * 16 + r;
        const bool live = row < N;
        f4 a[MLP_TILES], z[MLP_TILES];
        load(a, row, live, g);
        seen(a);
        for (int l = 0; l < n.L; ++l) {
            const int nti = mlp_tiles(n.w[l]), nto = mlp_tiles(n.w[l + 1]);
            mlp_layer(z, a, lds + n.woff[l], lds + n.boff[l], 16 * nti + 4, nti, nto, r, g);
            if (l + 1 < n.L) mlp_tanh(a, z);
        }
        mlp_store_rows(y, z, row, live, n.w[n.L], y_stride, g);
    }
}

// the same with x one array [N][w_0]
__device__ __forceinline__ void mlp_forward_tiles(int64_t N, int64_t tiles, const MlpNet& n, const float* __restrict__ lds,
                                                  const float* __restrict__ x, float* __restrict__ y, int y_stride) {
    mlp_forward_tiles(
        N, tiles, n, lds,
        [&](f4 (&a)[MLP_TILES], int64_t row, bool live, int g) { mlp_load_rows(a, x, row, live, n.w[0], n.w[0], g); },
        [](const f4 (&)[MLP_TILES]) {}, y, y_stride);
}

// The backward of the staged net over this wave's tiles (the same walk), and the wave's record at records[first * n.P].
// Rows of g_y lie gy_stride floats apart; out.g_x is [N][w_0].  T: the 16-feature tiles of the net's widest layer, or
// more -- the accumulators a wave holds are PIGS_MLP_MAX_LAYERS x T x T tiles of dW.  The body is the text of
// mlp_backward_body.h, which mlp.hip's mlp_backward_kernel includes as well: calling this function from there, the
// register allocator no longer fits that kernel into its registers (512 VGPRs and 32 spilled, against 488 and none).
template <int T>
__device__ __forceinline__ void mlp_backward_tiles(int64_t N, int64_t tiles, const MlpNet& n, const MlpGrads& out,
                                                   float* __restrict__ lds, const float* __restrict__ x,
                                                   const float* __restrict__ g_y, int gy_stride,
                                                   float* __restrict__ records) {
#define MLP_BODY_T T
#define MLP_BODY_LDS lds
#define MLP_BODY_LOAD_X(a, row, live, g) mlp_load_rows(a, x, row, live, n.w[0], n.w[0], g)
#define MLP_BODY_LOAD_GY(d, row, live, g) mlp_load_rows(d, g_y, row, live, n.w[n.L], gy_stride, g)
#define MLP_BODY_WANT_DA0 out.g_x
#define MLP_BODY_STORE_DA0(d, row, live, g) mlp_store_rows(out.g_x, d, row, live, n.w[0], n.w[0], g)
#define MLP_BODY_RECORDS records
#include "mlp_backward_body.h"
#undef MLP_BODY_T
#undef MLP_BODY_LDS
#undef MLP_BODY_LOAD_X
#undef MLP_BODY_LOAD_GY
#undef MLP_BODY_WANT_DA0
#undef MLP_BODY_STORE_DA0
#undef MLP_BODY_RECORDS
}

// Parameter e of the net from `records` records of n.P floats, by four lanes (lane = 16 part + e's low bits): lane `part`
// adds records part, part + 4, ... in that order, then the four partial sums are added as (p0 + p1) + (p2 + p3).  A
// fixed order, and four times as many loads in flight as one thread per parameter (measured, delta_net at N = 1 600, 100
// records: 24.4 us with one thread per parameter).  `block`: which 64 parameters this workgroup of 256 adds.
__device__ __forceinline__ void mlp_finish_block(const MlpNet& n, const MlpGrads& out, int records,
                                                 const float* __restrict__ scratch, int block) {
    const int lane = threadIdx.x & 63, part = lane >> 4;
    const int e = (block * 4 + (threadIdx.x >> 6)) * 16 + (lane & 15);
    const bool live = e < n.P;
    float sum = 0.0f;
    if (live) {
#pragma unroll 8
        for (int rcd = part; rcd < records; rcd += 4) sum += scratch[(int64_t)rcd * n.P + e];
    }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    if (!live || part) return;
    for (int l = 0; l < n.L; ++l) {
        const int k = e - n.poff[l], nw = n.w[l] * n.w[l + 1];
        if (k >= 0 && k < nw) {
            if (out.g_W[l]) out.g_W[l][k] = sum;
        } else if (k >= nw && k < nw + n.w[l + 1]) {
            if (out.g_b[l]) out.g_b[l][k - nw] = sum;
        }
    }
}

#endif  // __HIPCC__

}  // namespace pigs
