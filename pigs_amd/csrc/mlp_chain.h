// The register-resident tanh chain on v_mfma_f32_16x16x4_f32, shared by mlp.hip (one per-Gaussian net per launch) and
// input_transform.hip (the latent net, whose rows are gathered from eight arrays and summed instead of stored).  It holds
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
__device__ __forceinline__ void mlp_stage(const MlpNet& n, float* __restrict__ lds) {
    for (int l = 0; l < n.L; ++l) {
        const int in = n.w[l], out = n.w[l + 1], nti = mlp_tiles(in), op = 16 * mlp_tiles(out), S = 16 * nti + 4;
        const float* __restrict__ W = n.W[l];
        const float* __restrict__ b = n.b[l];
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

// a tile of 16 rows of a [N][width] array in the accumulator layout: lane (r, g) holds features 16 t + 4 g + 0..3 of
// row r; rows past N and features past the width are zeros
__device__ __forceinline__ void mlp_load_rows(f4 (&a)[MLP_TILES], const float* __restrict__ src, int64_t row, bool live,
                                              int width, int g) {
#pragma unroll
    for (int t = 0; t < MLP_TILES; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = 16 * t + 4 * g + s;
            a[t][s] = (live && k < width) ? src[row * width + k] : 0.0f;
        }
}

__device__ __forceinline__ void mlp_store_rows(float* __restrict__ dst, const f4 (&a)[MLP_TILES], int64_t row, bool live,
                                               int width, int g) {
#pragma unroll
    for (int t = 0; t < MLP_TILES; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = 16 * t + 4 * g + s;
            if (live && k < width) dst[row * width + k] = a[t][s];
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

#endif  // __HIPCC__

}  // namespace pigs
