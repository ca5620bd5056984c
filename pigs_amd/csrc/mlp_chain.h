// The register-resident tanh chain on v_mfma_f32_16x16x4_f32, shared by mlp.hip (one per-Gaussian net per launch),
// mlp_bank.hip (several nets of one shape over one input per launch) and input_transform.hip (the latent net, whose rows
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
// ...  Rows of y lie y_stride floats apart (one net: w_L).
__device__ __forceinline__ void mlp_forward_tiles(int64_t N, int64_t tiles, const MlpNet& n, const float* __restrict__ lds,
                                                  const float* __restrict__ x, float* __restrict__ y, int y_stride) {
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int64_t stride = (int64_t)gridDim.x * MLP_WAVES;
    for (int64_t tile = (int64_t)blockIdx.x * MLP_WAVES + (threadIdx.x >> 6); tile < tiles; tile += stride) {
        const int64_t row = tile * 16 + r;
        const bool live = row < N;
        f4 a[MLP_TILES], z[MLP_TILES];
        mlp_load_rows(a, x, row, live, n.w[0], n.w[0], g);
        for (int l = 0; l < n.L; ++l) {
            const int nti = mlp_tiles(n.w[l]), nto = mlp_tiles(n.w[l + 1]);
            mlp_layer(z, a, lds + n.woff[l], lds + n.boff[l], 16 * nti + 4, nti, nto, r, g);
            if (l + 1 < n.L) mlp_tanh(a, z);
        }
        mlp_store_rows(y, z, row, live, n.w[n.L], y_stride, g);
    }
}

// The backward of the staged net over this wave's tiles (the same walk), and the wave's record at records[first * n.P].
// Rows of g_y lie gy_stride floats apart; out.g_x is [N][w_0].  T: the 16-feature tiles of the net's widest layer, or
// more -- the accumulators a wave holds are PIGS_MLP_MAX_LAYERS x T x T tiles of dW.  This is the text of mlp.hip's
// mlp_backward_kernel at T = MLP_TILES, which keeps its own copy: called from there, the register allocator no longer
// fits that kernel into its registers (512 VGPRs and 32 spilled, against 488 and none).
template <int T>
__device__ __forceinline__ void mlp_backward_tiles(int64_t N, int64_t tiles, const MlpNet& n, const MlpGrads& out,
                                                   float* __restrict__ lds, const float* __restrict__ x,
                                                   const float* __restrict__ g_y, int gy_stride,
                                                   float* __restrict__ records) {
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4, wave = threadIdx.x >> 6;
    float* __restrict__ acts = lds + n.wave_off + wave * (n.L + 1) * 16 * MLP_ROW;      // a_l: tile l; dZ: tile L
    float* __restrict__ dz_t = acts + n.L * 16 * MLP_ROW;
    const int own = r * MLP_ROW + 4 * g;       // where this lane's four features of feature tile 0 lie in a tile

    f4 acc_w[PIGS_MLP_MAX_LAYERS][T][T], acc_b[PIGS_MLP_MAX_LAYERS][T];
#pragma unroll
    for (int l = 0; l < PIGS_MLP_MAX_LAYERS; ++l)
#pragma unroll
        for (int to = 0; to < T; ++to) {
            acc_b[l][to] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int ti = 0; ti < T; ++ti) acc_w[l][to][ti] = f4{0.0f, 0.0f, 0.0f, 0.0f};
        }

    const int64_t first = (int64_t)blockIdx.x * MLP_WAVES + wave, stride = (int64_t)gridDim.x * MLP_WAVES;
    for (int64_t tile = first; tile < tiles; tile += stride) {
        const int64_t row = tile * 16 + r;
        const bool live = row < N;
        f4 a[MLP_TILES], d[MLP_TILES];
        mlp_wave_fence();                      // the previous tile's reads of this region are done
        mlp_load_rows(a, x, row, live, n.w[0], n.w[0], g);
        for (int l = 0; l < n.L; ++l) {        // a_l to LDS, then a_{l+1}; y itself is not needed
#pragma unroll
            for (int t = 0; t < MLP_TILES; ++t) *reinterpret_cast<f4*>(acts + l * 16 * MLP_ROW + own + 16 * t) = a[t];
            if (l + 1 < n.L) {
                const int nti = mlp_tiles(n.w[l]), nto = mlp_tiles(n.w[l + 1]);
                mlp_layer(d, a, lds + n.woff[l], lds + n.boff[l], 16 * nti + 4, nti, nto, r, g);
                mlp_tanh(a, d);
            }
        }
        mlp_load_rows(d, g_y, row, live, n.w[n.L], gy_stride, g);      // dZ of the last layer
#pragma unroll
        for (int l = PIGS_MLP_MAX_LAYERS - 1; l >= 0; --l) {
            if (l >= n.L) continue;
            const bool want_da = l > 0 || out.g_x;
            mlp_backward_layer<T, T>(d, acc_w[l], acc_b[l], out.g_W[l] != nullptr, out.g_b[l] != nullptr,
                                                     want_da, l == 0, lds + n.woff[l], mlp_tiles(n.w[l + 1]),
                                                     mlp_tiles(n.w[l]), acts + l * 16 * MLP_ROW, dz_t, own, r, g);
            if (l == 0 && want_da) mlp_store_rows(out.g_x, d, row, live, n.w[0], n.w[0], g);
        }
    }

    // this wave's record; a wave without a tile (only past the last tile's wave) writes none
    if (first >= tiles) return;
    float* __restrict__ rec = records + first * n.P;
#pragma unroll
    for (int l = 0; l < PIGS_MLP_MAX_LAYERS; ++l) {
        if (l >= n.L) continue;
        mlp_record_layer<T, T>(rec, n.poff[l], acc_w[l], acc_b[l], out.g_W[l] != nullptr,
                                               out.g_b[l] != nullptr, n.w[l], n.w[l + 1], r, g);
    }
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
