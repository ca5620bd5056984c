// The register-resident tanh chain on v_mfma_f32_16x16x4_f32, shared by mlp.hip (one per-Gaussian net per launch) and
// input_transform.hip (the latent net, whose rows are gathered from eight arrays and summed instead of stored).  The
// operand layout and the padded LDS images are described at the head of mlp.hip.
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

// mlp.hip: the launch that adds `records` records of n.P floats in a fixed order into out.g_W / out.g_b
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

#endif  // __HIPCC__

}  // namespace pigs
