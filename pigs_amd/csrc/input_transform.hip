// InputTransform (model_pn.py:51-152, called at :237-249): the dynamics network's t_params in THREE launches forward
// and at most FIVE backward.  d = 2, c = 1..4 channels, p = pde_size = 1..4, float32.
//
//   x_n      = (means 2, full_covariances 4, u c, boundaries 1, sample_u c, sample_ux 2c, sample_uxx 2c, sample_pde p)
//   a_n      = tanh(W3 tanh(W2 tanh(W1 x_n + b1) + b2) + b3)            the latent net, (7 + 6c + p) -> 16 -> 32 -> 16
//   latent   = (1 / N) sum_n a_n
//   T_j      = I + reshape(net_j(latent), k_j, k_j)                      16 -> 48 -> 32 -> k_j^2, k = (2, c, 2c, 2c, p)
//   t_params = (T Sigma_n row-major, T_u u_n, boundaries_n, T_u sample_u_n, T_ux ux_n, T_uxx uxx_n, T_pde pde_n)
//
// The matrices are packed as T [4], T_u [c^2], T_ux [4c^2], T_uxx [4c^2], T_pde [p^2], each row-major.
// `params` is 36 pointers: net * 6 + (W1, b1, W2, b2, W3, b3), net 0 the latent net, 1..5 the five matrices' nets.
//
// Forward
//   it_latent_kernel     the chain of mlp_chain.h, x gathered from the eight arrays at the permuted column; a wave sums
//                        the 16 latent values of its LIVE rows (a row past N is loaded as zeros, but tanh(b) != 0) over
//                        its tiles and writes one record of 16 floats; at most IT_FORWARD_WAVES waves
//   it_matrices_kernel   one workgroup: the records in a fixed order (in double), / N, the five nets, the packed matrices
//   it_apply_kernel      one thread per output element, the matrices in LDS, coalesced stores
// Backward
//   it_apply_backward_kernel     per row g_Sigma = T^T g and g_u = T_u^T g; lane e of a wave owns matrix elements e, e + 64,
//                                e + 128 and adds g_n x_n^T over the wave's rows in double: one record per wave, then
//   it_sum_records_kernel        the records in a fixed order (in double)
//   it_matrices_backward_kernel  one workgroup recomputes the nets from `latent`; outer products give the 30 parameter
//                                gradients, transposed products g_latent / N
//   it_latent_backward_kernel    the backward of mlp.hip's chain with the net's tile counts fixed at compile time: every live
//                                row's upstream gradient is g_latent / N; the input gradient goes to the means, covariance
//                                and u columns; then mlp.hip's finishing launch
// The scratch is 16 floats (g_latent / N) followed by the records.  No float atomics, no ticket: the same inputs give
// the same bits on every call; nothing allocates, synchronises or reads back.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "mlp_chain.h"

namespace pigs {

constexpr int IT_LATENT = 16, IT_H1 = 48, IT_H2 = 32;      // LATENT_SIZE, L3_SIZE, L2_SIZE of TransformNet
constexpr int IT_NETS = 5, IT_PARAMS = 6 * (IT_NETS + 1);
constexpr int IT_MAX_MATRICES = 4 + 9 * 16 + 16;            // packed floats at c = p = 4
constexpr int IT_HEAD = 16;                                  // scratch floats in front of the records
// waves of the latent forward: its records are 16 floats, so its cap is the forward's of mlp.hip (which measured 94 us
// with 256 waves against 31 us with 2 048 at N = 65 536), not the backward's; 2 048 x 16 floats fit wherever the
// backward's 256 records of the latent net's 1 300 and more parameters do
constexpr int IT_FORWARD_WAVES = 2048;

struct ItRows {          // means, full_covariances, u, boundaries, sample_u, sample_ux, sample_uxx, sample_pde
    const float* src[8];
    int c, p;
};
struct ItParams {
    const float* p[IT_PARAMS];
};
struct ItParamGrads {
    float* p[IT_PARAMS];
};

__host__ __device__ constexpr int it_in_width(int j, int c, int p) {
    return j == 0 ? 2 : j == 1 ? 4 : j == 3 ? 1 : j == 7 ? p : (j == 2 || j == 4) ? c : 2 * c;
}
__host__ __device__ constexpr int it_x_width(int c, int p) { return 7 + 6 * c + p; }
__host__ __device__ constexpr int it_out_width(int c, int p) { return 5 + 6 * c + p; }
__host__ __device__ constexpr int it_matrix_k(int j, int c, int p) { return j == 0 ? 2 : j == 1 ? c : j == 4 ? p : 2 * c; }
__host__ __device__ constexpr int it_matrix_off(int j, int c) {
    return j == 0 ? 0 : j == 1 ? 4 : j == 2 ? 4 + c * c : j == 3 ? 4 + 5 * c * c : 4 + 9 * c * c;
}
__host__ __device__ constexpr int it_matrix_floats(int c, int p) { return 4 + 9 * c * c + p * p; }

// column k < it_x_width of row `row` of x, from the array that holds it
__device__ __forceinline__ float it_x(const ItRows& in, int k, int64_t row) {
    const float* ptr = in.src[0];
    int stride = 2, off = k, start = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int w = it_in_width(j, in.c, in.p);
        if (k >= start && k < start + w) {
            ptr = in.src[j];
            stride = w;
            off = k - start;
        }
        start += w;
    }
    return ptr[row * stride + off];
}

__device__ __forceinline__ void it_load_x(f4 (&a)[MLP_TILES], const ItRows& in, int64_t row, bool live, int width, int g) {
#pragma unroll
    for (int t = 0; t < MLP_TILES; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = 16 * t + 4 * g + s;
            a[t][s] = (live && k < width) ? it_x(in, k, row) : 0.0f;
        }
}

__global__ __launch_bounds__(64 * MLP_WAVES) void it_latent_kernel(int64_t N, int64_t tiles, MlpNet n, ItRows in,
                                                                   float* __restrict__ records) {
    extern __shared__ float it_lds[];
    mlp_stage(n, it_lds);
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int64_t first = (int64_t)blockIdx.x * MLP_WAVES + (threadIdx.x >> 6), stride = (int64_t)gridDim.x * MLP_WAVES;
    f4 sum = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t tile = first; tile < tiles; tile += stride) {
        const int64_t row = tile * 16 + r;
        const bool live = row < N;
        f4 a[MLP_TILES], z[MLP_TILES];
        it_load_x(a, in, row, live, n.w[0], g);
        for (int l = 0; l < n.L; ++l) {
            const int nti = mlp_tiles(n.w[l]), nto = mlp_tiles(n.w[l + 1]);
            mlp_layer(z, a, it_lds + n.woff[l], it_lds + n.boff[l], 16 * nti + 4, nti, nto, r, g);
            mlp_tanh(a, z);
        }
        if (live) sum += a[0];                 // a dead row holds tanh(bias chain), not zero: it stays out of the mean
    }
    if (first >= tiles) return;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        float v = sum[s];
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m);      // the 16 row lanes of this g, a fixed tree
        if (r == 0) records[first * IT_LATENT + 4 * g + s] = v;
    }
}

// h1 = tanh(W1 latent + b1), h2 = tanh(W2 h1 + b2) of the five nets, by one workgroup of 256.  In double: some four
// hundred tanh in all, and T = I + net(latent) may cancel (a diagonal element near -1 of the net gives a small T[i][i] whose
// product with the rows is then held to the scale of a small tensor), so the nets add no rounding of their own to latent's.
__device__ __forceinline__ void it_nets_hidden(const ItParams& prm, const float* lat, double (*h1)[IT_H1], double (*h2)[IT_H2]) {
    for (int e = threadIdx.x; e < IT_NETS * IT_H1; e += 256) {
        const int j = e / IT_H1, o = e - j * IT_H1;
        const float* __restrict__ W = prm.p[6 * (j + 1)] + o * IT_LATENT;
        double acc = (double)prm.p[6 * (j + 1) + 1][o];
#pragma unroll
        for (int i = 0; i < IT_LATENT; ++i) acc = fma((double)W[i], (double)lat[i], acc);
        h1[j][o] = tanh(acc);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < IT_NETS * IT_H2; e += 256) {
        const int j = e / IT_H2, o = e - j * IT_H2;
        const float* __restrict__ W = prm.p[6 * (j + 1) + 2] + o * IT_H1;
        double acc = (double)prm.p[6 * (j + 1) + 3][o];
#pragma unroll 16
        for (int i = 0; i < IT_H1; ++i) acc = fma((double)W[i], h1[j][i], acc);
        h2[j][o] = tanh(acc);
    }
    __syncthreads();
}

// the net (0..4) that packed matrix element e belongs to
__device__ __forceinline__ int it_matrix_of(int e, int c) {
    return e < 4 ? 0 : e < 4 + c * c ? 1 : e < 4 + 5 * c * c ? 2 : e < 4 + 9 * c * c ? 3 : 4;
}

__global__ __launch_bounds__(256) void it_matrices_kernel(int64_t N, int records, int c, int p, ItParams prm,
                                                          const float* __restrict__ recs, float* __restrict__ latent,
                                                          float* __restrict__ matrices) {
    __shared__ double part[16][IT_LATENT];
    __shared__ double h1[IT_NETS][IT_H1], h2[IT_NETS][IT_H2];
    __shared__ float lat[IT_LATENT];
    const int t = threadIdx.x;
    {
        const int e = t & 15, q = t >> 4;      // thread (q, e) adds records q, q + 16, ... of feature e, in that order
        double s = 0.0;
        for (int rcd = q; rcd < records; rcd += 16) s += (double)recs[rcd * IT_LATENT + e];
        part[q][e] = s;
    }
    __syncthreads();
    if (t < IT_LATENT) {
        double s = 0.0;
        for (int q = 0; q < 16; ++q) s += part[q][t];
        const float v = (float)(s / (double)N);
        lat[t] = v;
        latent[t] = v;
    }
    __syncthreads();
    it_nets_hidden(prm, lat, h1, h2);
    for (int e = t; e < it_matrix_floats(c, p); e += 256) {
        const int j = it_matrix_of(e, c), o = e - it_matrix_off(j, c), k = it_matrix_k(j, c, p);
        const float* __restrict__ W = prm.p[6 * (j + 1) + 4] + o * IT_H2;
        double acc = (double)prm.p[6 * (j + 1) + 5][o];
#pragma unroll 16
        for (int i = 0; i < IT_H2; ++i) acc = fma((double)W[i], h2[j][i], acc);
        matrices[e] = (float)(acc + (o / k == o % k ? 1.0 : 0.0));
    }
}

__device__ __forceinline__ float it_dot(const float* T, const float* __restrict__ x, int k) {
    float v = 0.0f;
    for (int i = 0; i < k; ++i) v = fmaf(T[i], x[i], v);
    return v;
}

__global__ __launch_bounds__(256) void it_apply_kernel(int64_t N, int c, int p, const float* __restrict__ matrices, ItRows in,
                                                       float* __restrict__ out) {
    __shared__ float T[IT_MAX_MATRICES];
    for (int i = threadIdx.x; i < it_matrix_floats(c, p); i += 256) T[i] = matrices[i];
    __syncthreads();
    const int D = it_out_width(c, p), cc = c * c;
    const int64_t total = N * D, step = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += step) {
        const int64_t row = e / D;
        const int col = (int)(e - row * D);
        float v;
        if (col < 4) {
            const float* __restrict__ cov = in.src[1] + row * 4;
            const int i = col >> 1, j = col & 1;
            v = fmaf(T[2 * i + 1], cov[2 + j], T[2 * i] * cov[j]);
        } else if (col < 4 + c) {
            v = it_dot(T + 4 + (col - 4) * c, in.src[2] + row * c, c);
        } else if (col == 4 + c) {
            v = in.src[3] ? in.src[3][row] : 0.0f;
        } else if (col < 5 + 2 * c) {
            v = it_dot(T + 4 + (col - 5 - c) * c, in.src[4] + row * c, c);
        } else if (col < 5 + 4 * c) {
            v = it_dot(T + 4 + cc + (col - 5 - 2 * c) * 2 * c, in.src[5] + row * 2 * c, 2 * c);
        } else if (col < 5 + 6 * c) {
            v = it_dot(T + 4 + 5 * cc + (col - 5 - 4 * c) * 2 * c, in.src[6] + row * 2 * c, 2 * c);
        } else {
            v = it_dot(T + 4 + 9 * cc + (col - 5 - 6 * c) * p, in.src[7] + row * p, p);
        }
        out[e] = v;
    }
}

__global__ __launch_bounds__(64 * MLP_WAVES) void it_apply_backward_kernel(int64_t N, int64_t tiles, int c, int p,
                                                                           const float* __restrict__ matrices, ItRows in,
                                                                           const float* __restrict__ g_t,
                                                                           float* __restrict__ g_cov, float* __restrict__ g_u,
                                                                           float* __restrict__ records) {
    __shared__ float T[IT_MAX_MATRICES];
    const int PM = it_matrix_floats(c, p), D = it_out_width(c, p);
    for (int i = threadIdx.x; i < PM; i += 64 * MLP_WAVES) T[i] = matrices[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, r = lane & 15, gq = lane >> 4;

    // matrix elements lane, lane + 64, lane + 128: dT[i][k] = sum_n g[n][col0] x0[n] (+ g[n][col1] x1[n])
    int col0[3], col1[3], s0[3];
    const float *x0[3], *x1[3];
    bool own[3];
    double acc[3] = {0.0, 0.0, 0.0};           // g x is exact in double: the sum over the rows keeps what a sum that
#pragma unroll                                 // cancels (g and x of either sign) would lose in float
    for (int q = 0; q < 3; ++q) {
        const int e = lane + 64 * q;
        own[q] = records != nullptr && e < PM;
        const int j = it_matrix_of(own[q] ? e : 0, c), k = it_matrix_k(j, c, p), o = (own[q] ? e : 0) - it_matrix_off(j, c);
        const int i = o / k, kk = o - i * k;
        x1[q] = nullptr;
        col1[q] = 0;
        s0[q] = k;
        if (j == 0) {                          // T Sigma: g columns 2 i + j', Sigma[kk][j']
            col0[q] = 2 * i; x0[q] = in.src[1] + 2 * kk; s0[q] = 4;
            col1[q] = 2 * i + 1; x1[q] = in.src[1] + 2 * kk + 1;
        } else if (j == 1) {                   // T_u on u and on sample_u
            col0[q] = 4 + i; x0[q] = in.src[2] + kk;
            col1[q] = 5 + c + i; x1[q] = in.src[4] + kk;
        } else if (j == 2) {
            col0[q] = 5 + 2 * c + i; x0[q] = in.src[5] + kk;
        } else if (j == 3) {
            col0[q] = 5 + 4 * c + i; x0[q] = in.src[6] + kk;
        } else {
            col0[q] = 5 + 6 * c + i; x0[q] = in.src[7] + kk;
        }
    }

    const int64_t first = (int64_t)blockIdx.x * MLP_WAVES + (threadIdx.x >> 6), stride = (int64_t)gridDim.x * MLP_WAVES;
    for (int64_t tile = first; tile < tiles; tile += stride) {
        const int64_t row = tile * 16 + r;
        if (row < N) {                         // lane (r, gq): outputs gq and gq + 4 of (g_Sigma 4, g_u c) of row r
            const float* __restrict__ g = g_t + row * D;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int o = gq + 4 * h;
                if (o < 4) {
                    if (g_cov) g_cov[row * 4 + o] = fmaf(T[2 + (o >> 1)], g[2 + (o & 1)], T[o >> 1] * g[o & 1]);
                } else if (o - 4 < c && g_u) {
                    float v = 0.0f;
                    for (int i = 0; i < c; ++i) v = fmaf(T[4 + i * c + (o - 4)], g[4 + i], v);
                    g_u[row * c + (o - 4)] = v;
                }
            }
        }
        if (records) {
            const int64_t base = tile * 16;
            const int rows = N - base < 16 ? (int)(N - base) : 16;
            for (int rr = 0; rr < rows; ++rr) {
                const int64_t rw = base + rr;
                const float* __restrict__ g = g_t + rw * D;
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    if (own[q]) {
                        acc[q] = fma((double)g[col0[q]], (double)x0[q][rw * s0[q]], acc[q]);
                        if (x1[q]) acc[q] = fma((double)g[col1[q]], (double)x1[q][rw * s0[q]], acc[q]);
                    }
            }
        }
    }
    if (!records || first >= tiles) return;
#pragma unroll
    for (int q = 0; q < 3; ++q)
        if (own[q]) {                          // a record is PM pairs (head, rest) of floats: the scratch is 4-byte aligned
            const float head = (float)acc[q];
            float* __restrict__ rec = records + (first * PM + lane + 64 * q) * 2;
            rec[0] = head;
            rec[1] = (float)(acc[q] - (double)head);
        }
}

// Four lanes per element as mlp_finish_kernel: lane `part` adds records part, part + 4, ..., then (p0 + p1) + (p2 + p3);
// the records are pairs of floats (head, rest) and the sums are kept in double
__global__ __launch_bounds__(256) void it_sum_records_kernel(int P, int records, const float* __restrict__ recs,
                                                             float* __restrict__ out) {
    const int lane = threadIdx.x & 63, part = lane >> 4;
    const int e = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16 + (lane & 15);
    const bool live = e < P;
    double sum = 0.0;
    if (live) {
#pragma unroll 8
        for (int rcd = part; rcd < records; rcd += 4) {
            const float* __restrict__ rec = recs + ((int64_t)rcd * P + e) * 2;
            sum += (double)rec[0] + (double)rec[1];
        }
    }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    if (live && part == 0) out[e] = (float)sum;
}

__global__ __launch_bounds__(256) void it_matrices_backward_kernel(int64_t N, int c, int p, ItParams prm, ItParamGrads out,
                                                                   const float* __restrict__ latent,
                                                                   const float* __restrict__ g_matrices,
                                                                   float* __restrict__ g_latent) {
    __shared__ double h1d[IT_NETS][IT_H1], h2d[IT_NETS][IT_H2];
    __shared__ float lat[IT_LATENT], h1[IT_NETS][IT_H1], h2[IT_NETS][IT_H2], gm[IT_MAX_MATRICES];
    __shared__ float dz2[IT_NETS][IT_H2], dz1[IT_NETS][IT_H1], dl[IT_NETS][IT_LATENT];
    const int t = threadIdx.x;
    if (t < IT_LATENT) lat[t] = latent[t];
    for (int e = t; e < it_matrix_floats(c, p); e += 256) gm[e] = g_matrices[e];
    __syncthreads();
    it_nets_hidden(prm, lat, h1d, h2d);
    for (int e = t; e < IT_NETS * IT_H1; e += 256) h1[e / IT_H1][e % IT_H1] = (float)h1d[e / IT_H1][e % IT_H1];
    for (int e = t; e < IT_NETS * IT_H2; e += 256) h2[e / IT_H2][e % IT_H2] = (float)h2d[e / IT_H2][e % IT_H2];
    __syncthreads();
    for (int e = t; e < IT_NETS * IT_H2; e += 256) {         // dZ2 = (W3^T g) (1 - h2^2)
        const int j = e / IT_H2, i = e - j * IT_H2, k = it_matrix_k(j, c, p);
        const float* __restrict__ W = prm.p[6 * (j + 1) + 4];
        const float* g = gm + it_matrix_off(j, c);
        float s = 0.0f;
        for (int o = 0; o < k * k; ++o) s = fmaf(W[o * IT_H2 + i], g[o], s);
        dz2[j][i] = s * fmaf(-h2[j][i], h2[j][i], 1.0f);
    }
    __syncthreads();
    for (int e = t; e < IT_NETS * IT_H1; e += 256) {         // dZ1 = (W2^T dZ2) (1 - h1^2)
        const int j = e / IT_H1, i = e - j * IT_H1;
        const float* __restrict__ W = prm.p[6 * (j + 1) + 2];
        float s = 0.0f;
#pragma unroll 8
        for (int o = 0; o < IT_H2; ++o) s = fmaf(W[o * IT_H1 + i], dz2[j][o], s);
        dz1[j][i] = s * fmaf(-h1[j][i], h1[j][i], 1.0f);
    }
    __syncthreads();
    if (g_latent) {
        for (int e = t; e < IT_NETS * IT_LATENT; e += 256) {
            const int j = e / IT_LATENT, i = e - j * IT_LATENT;
            const float* __restrict__ W = prm.p[6 * (j + 1)];
            float s = 0.0f;
#pragma unroll 8
            for (int o = 0; o < IT_H1; ++o) s = fmaf(W[o * IT_LATENT + i], dz1[j][o], s);
            dl[j][i] = s;
        }
        __syncthreads();
        if (t < IT_LATENT) g_latent[t] = ((((dl[0][t] + dl[1][t]) + dl[2][t]) + dl[3][t]) + dl[4][t]) / (float)N;
    }
    for (int j = 0; j < IT_NETS; ++j) {                      // the outer products
        float* const* o = out.p + 6 * (j + 1);
        const int kk = it_matrix_k(j, c, p) * it_matrix_k(j, c, p);
        const float* g = gm + it_matrix_off(j, c);
        if (o[0])
            for (int e = t; e < IT_H1 * IT_LATENT; e += 256) o[0][e] = dz1[j][e / IT_LATENT] * lat[e % IT_LATENT];
        if (o[1] && t < IT_H1) o[1][t] = dz1[j][t];
        if (o[2])
            for (int e = t; e < IT_H2 * IT_H1; e += 256) o[2][e] = dz2[j][e / IT_H1] * h1[j][e % IT_H1];
        if (o[3] && t < IT_H2) o[3][t] = dz2[j][t];
        if (o[4])
            for (int e = t; e < kk * IT_H2; e += 256) o[4][e] = g[e / IT_H2] * h2[j][e % IT_H2];
        if (o[5] && t < kk) o[5][t] = g[t];
    }
}

// The latent net's backward.  It recomputes the activations (a_0, a_1, a_2 to this wave's LDS tiles, the output in
// registers); every live row's dZ of the last layer is (g_latent / N) (1 - a_3^2), a dead row's is zero; dW and db stay in
// registers, one record per wave (mlp.hip's finishing launch adds them); dA_0 goes to the means, covariance and u columns.
__global__ __launch_bounds__(64 * MLP_WAVES) void it_latent_backward_kernel(int64_t N, int64_t tiles, MlpNet n, MlpGrads out,
                                                                            ItRows in, const float* __restrict__ g_latent,
                                                                            float* __restrict__ g_means,
                                                                            float* __restrict__ g_cov, float* __restrict__ g_u,
                                                                            float* __restrict__ records) {
    extern __shared__ float it_lds[];
    mlp_stage(n, it_lds);
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4, wave = threadIdx.x >> 6;
    constexpr int TILE = 16 * MLP_ROW;
    float* __restrict__ acts = it_lds + n.wave_off + wave * 4 * TILE;      // a_l: tile l; dZ: tile 3
    float* __restrict__ dz_t = acts + 3 * TILE;
    const int own = r * MLP_ROW + 4 * g, nti0 = mlp_tiles(n.w[0]);
    const bool want_x = g_means || g_cov || g_u;
    f4 gl;
#pragma unroll
    for (int s = 0; s < 4; ++s) gl[s] = g_latent[4 * g + s];

    f4 w0[1][MLP_TILES] = {}, w1[2][1] = {}, w2[1][2] = {}, b0[1] = {}, b1[2] = {}, b2[1] = {};
    const int64_t first = (int64_t)blockIdx.x * MLP_WAVES + wave, stride = (int64_t)gridDim.x * MLP_WAVES;
    for (int64_t tile = first; tile < tiles; tile += stride) {
        const int64_t row = tile * 16 + r;
        const bool live = row < N;
        f4 a[MLP_TILES], d[MLP_TILES];
        mlp_wave_fence();                      // the previous tile's reads of this region are done
        it_load_x(a, in, row, live, n.w[0], g);
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            const int nti = l == 0 ? nti0 : l, nto = l == 1 ? 2 : 1;
#pragma unroll
            for (int t = 0; t < MLP_TILES; ++t)
                if (l == 0 || t < l) *reinterpret_cast<f4*>(acts + l * TILE + own + 16 * t) = a[t];
            mlp_layer(d, a, it_lds + n.woff[l], it_lds + n.boff[l], 16 * nti + 4, nti, nto, r, g);
            mlp_tanh(a, d);
        }
#pragma unroll
        for (int t = 0; t < MLP_TILES; ++t) d[t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < 4; ++s) d[0][s] = live ? gl[s] * fmaf(-a[0][s], a[0][s], 1.0f) : 0.0f;
        mlp_backward_layer<1, 2>(d, w2, b2, out.g_W[2] != nullptr, out.g_b[2] != nullptr, true, false, it_lds + n.woff[2], 1, 2,
                                 acts + 2 * TILE, dz_t, own, r, g);
        mlp_backward_layer<2, 1>(d, w1, b1, out.g_W[1] != nullptr, out.g_b[1] != nullptr, true, false, it_lds + n.woff[1], 2, 1,
                                 acts + TILE, dz_t, own, r, g);
        mlp_backward_layer<1, MLP_TILES>(d, w0, b0, out.g_W[0] != nullptr, out.g_b[0] != nullptr, want_x, true,
                                         it_lds + n.woff[0], 1, nti0, acts, dz_t, own, r, g);
        if (want_x && live) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {      // columns 0 .. 5 + c < 16: feature tile 0 only
                const int k = 4 * g + s;
                if (k < 2) {
                    if (g_means) g_means[row * 2 + k] = d[0][s];
                } else if (k < 6) {
                    if (g_cov) g_cov[row * 4 + k - 2] = d[0][s];
                } else if (k < 6 + in.c) {
                    if (g_u) g_u[row * in.c + k - 6] = d[0][s];
                }
            }
        }
    }

    // this wave's record; a wave without a tile (only past the last tile's wave) writes none
    if (first >= tiles) return;
    float* __restrict__ rec = records + first * n.P;
    mlp_record_layer<1, MLP_TILES>(rec, n.poff[0], w0, b0, out.g_W[0] != nullptr, out.g_b[0] != nullptr, n.w[0], IT_LATENT, r, g);
    mlp_record_layer<2, 1>(rec, n.poff[1], w1, b1, out.g_W[1] != nullptr, out.g_b[1] != nullptr, IT_LATENT, IT_H2, r, g);
    mlp_record_layer<1, 2>(rec, n.poff[2], w2, b2, out.g_W[2] != nullptr, out.g_b[2] != nullptr, IT_H2, IT_LATENT, r, g);
}

// ---- host ----------------------------------------------------------------------------------------------------
struct ItWidths {
    int w[4];
};
static ItWidths it_latent_widths(int c, int p) { return {{it_x_width(c, p), IT_LATENT, IT_H2, IT_LATENT}}; }

static bool it_sizes_supported(int dtype, int c, int p) { return dtype == PIGS_F32 && c >= 1 && c <= 4 && p >= 1 && p <= 4; }

static size_t it_scratch_bytes(int64_t N, int c, int p) {
    if (N < 1 || c < 1 || c > 4 || p < 1 || p > 4) return 0;
    return (size_t)(IT_HEAD + mlp_records(N) * mlp_record_floats(3, it_latent_widths(c, p).w)) * sizeof(float);
}

static bool it_scratch_ok(const void* scratch, size_t bytes, int64_t N, int c, int p) {
    return scratch && !((uintptr_t)scratch & 3u) && bytes >= it_scratch_bytes(N, c, p);
}

static ItRows it_rows(int c, int p, const void* const (&in)[8]) {
    ItRows r{};
    for (int j = 0; j < 8; ++j) r.src[j] = (const float*)in[j];
    r.c = c;
    r.p = p;
    return r;
}

static MlpNet it_latent_net(int c, int p, const void* const* params, int* lds_floats) {
    const void* const W[3] = {params[0], params[2], params[4]};
    const void* const b[3] = {params[1], params[3], params[5]};
    return mlp_describe(3, it_latent_widths(c, p).w, W, b, lds_floats);
}

static bool it_params_missing(const void* const* params) {
    if (!params) return true;
    for (int i = 0; i < IT_PARAMS; ++i)
        if (!params[i]) return true;
    return false;
}

}  // namespace pigs

using namespace pigs;

extern "C" {

size_t pigs_input_transform_scratch_bytes(int64_t N, int c, int p) { return it_scratch_bytes(N, c, p); }

int pigs_input_transform_matrices_forward(int dtype, int64_t N, int c, int p, const void* means,
                                          const void* full_covariances, const void* u, const void* boundaries,
                                          const void* sample_u, const void* sample_ux, const void* sample_uxx,
                                          const void* sample_pde, const void* const* params, void* scratch,
                                          size_t scratch_bytes, void* latent, void* matrices, void* stream) {
    if (!it_sizes_supported(dtype, c, p)) return PIGS_ERR_UNSUPPORTED;
    if (N < 1) return PIGS_ERR_INVALID;
    const void* const in[8] = {means, full_covariances, u, boundaries, sample_u, sample_ux, sample_uxx, sample_pde};
    for (const void* a : in)
        if (!a) return PIGS_ERR_INVALID;
    if (it_params_missing(params) || !latent || !matrices) return PIGS_ERR_INVALID;
    if (!it_scratch_ok(scratch, scratch_bytes, N, c, p)) return PIGS_ERR_INVALID;
    int lds_floats;
    const MlpNet n = it_latent_net(c, p, params, &lds_floats);
    ItParams prm{};
    for (int i = 0; i < IT_PARAMS; ++i) prm.p[i] = (const float*)params[i];
    const int64_t tiles = (N + 15) / 16, records = tiles < IT_FORWARD_WAVES ? tiles : IT_FORWARD_WAVES;
    static_assert(IT_FORWARD_WAVES * IT_LATENT <= PIGS_MLP_MAX_RECORDS * (IT_H2 * (IT_LATENT + 1) + IT_LATENT * (IT_H2 + 1)),
                  "the forward's records fit in the backward's");
    float* recs = (float*)scratch + IT_HEAD;
    clear_hip_error();
    hipLaunchKernelGGL(it_latent_kernel, dim3((unsigned)((records + MLP_WAVES - 1) / MLP_WAVES)), dim3(64 * MLP_WAVES),
                       lds_floats * sizeof(float), (hipStream_t)stream, N, tiles, n, it_rows(c, p, in), recs);
    hipLaunchKernelGGL(it_matrices_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, N, (int)records, c, p, prm,
                       (const float*)recs, (float*)latent, (float*)matrices);
    return launch_status();
}

int pigs_input_transform_matrices_backward(int dtype, int64_t N, int c, int p, const void* means,
                                           const void* full_covariances, const void* u, const void* boundaries,
                                           const void* sample_u, const void* sample_ux, const void* sample_uxx,
                                           const void* sample_pde, const void* const* params, const void* latent,
                                           const void* g_matrices, void* scratch, size_t scratch_bytes, void* g_means,
                                           void* g_full_covariances, void* g_u, void* const* g_params, void* stream) {
    if (!it_sizes_supported(dtype, c, p)) return PIGS_ERR_UNSUPPORTED;
    if (N < 1) return PIGS_ERR_INVALID;
    const void* const in[8] = {means, full_covariances, u, boundaries, sample_u, sample_ux, sample_uxx, sample_pde};
    for (const void* a : in)
        if (!a) return PIGS_ERR_INVALID;
    if (it_params_missing(params) || !latent || !g_matrices) return PIGS_ERR_INVALID;
    bool latent_params = false, net_params = false;
    for (int i = 0; g_params && i < IT_PARAMS; ++i) (i < 6 ? latent_params : net_params) |= g_params[i] != nullptr;
    const bool rows = g_means || g_full_covariances || g_u;
    if (!rows && !latent_params && !net_params) return PIGS_ERR_INVALID;
    if (!it_scratch_ok(scratch, scratch_bytes, N, c, p)) return PIGS_ERR_INVALID;
    int lds_floats;
    const MlpNet n = it_latent_net(c, p, params, &lds_floats);
    ItParams prm{};
    ItParamGrads out{};
    for (int i = 0; i < IT_PARAMS; ++i) {
        prm.p[i] = (const float*)params[i];
        out.p[i] = g_params ? (float*)g_params[i] : nullptr;
    }
    const bool through_latent = rows || latent_params;
    float* head = (float*)scratch;
    clear_hip_error();
    hipLaunchKernelGGL(it_matrices_backward_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, N, c, p, prm, out,
                       (const float*)latent, (const float*)g_matrices, through_latent ? head : nullptr);
    if (through_latent) {
        MlpGrads grads{};
        for (int l = 0; l < 3; ++l) {
            grads.g_W[l] = out.p[2 * l];
            grads.g_b[l] = out.p[2 * l + 1];
        }
        const int64_t tiles = (N + 15) / 16, records = mlp_records(N);
        const size_t lds = (size_t)(lds_floats + MLP_WAVES * 4 * 16 * MLP_ROW) * sizeof(float);      // images, 4 tiles a wave
        static_assert((848 + 672 + 592 + MLP_WAVES * 4 * 16 * MLP_ROW) * sizeof(float) <= 64 * 1024, "the default LDS limit");
        hipLaunchKernelGGL(it_latent_backward_kernel, dim3((unsigned)((records + MLP_WAVES - 1) / MLP_WAVES)),
                           dim3(64 * MLP_WAVES), lds, (hipStream_t)stream, N, tiles, n, grads, it_rows(c, p, in),
                           (const float*)head, (float*)g_means, (float*)g_full_covariances, (float*)g_u, head + IT_HEAD);
        if (latent_params) mlp_finish_launch(n, grads, (int)records, head + IT_HEAD, (hipStream_t)stream);
    }
    return launch_status();
}

int pigs_input_transform_apply_forward(int dtype, int64_t N, int c, int p, const void* matrices,
                                       const void* full_covariances, const void* u, const void* boundaries,
                                       const void* sample_u, const void* sample_ux, const void* sample_uxx,
                                       const void* sample_pde, void* t_params, void* stream) {
    if (!it_sizes_supported(dtype, c, p)) return PIGS_ERR_UNSUPPORTED;
    if (N < 1) return PIGS_ERR_INVALID;
    if (!matrices || !full_covariances || !u || !sample_u || !sample_ux || !sample_uxx || !sample_pde || !t_params)
        return PIGS_ERR_INVALID;
    const void* const in[8] = {nullptr, full_covariances, u, boundaries, sample_u, sample_ux, sample_uxx, sample_pde};
    const int64_t blocks = (N * it_out_width(c, p) + 255) / 256;
    clear_hip_error();
    hipLaunchKernelGGL(it_apply_kernel, dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(256), 0,
                       (hipStream_t)stream, N, c, p, (const float*)matrices, it_rows(c, p, in), (float*)t_params);
    return launch_status();
}

int pigs_input_transform_apply_backward(int dtype, int64_t N, int c, int p, const void* matrices,
                                        const void* full_covariances, const void* u, const void* sample_u,
                                        const void* sample_ux, const void* sample_uxx, const void* sample_pde,
                                        const void* g_t_params, void* scratch, size_t scratch_bytes,
                                        void* g_full_covariances, void* g_u, void* g_matrices, void* stream) {
    if (!it_sizes_supported(dtype, c, p)) return PIGS_ERR_UNSUPPORTED;
    if (N < 1) return PIGS_ERR_INVALID;
    if (!matrices || !full_covariances || !u || !sample_u || !sample_ux || !sample_uxx || !sample_pde || !g_t_params)
        return PIGS_ERR_INVALID;
    if (!g_full_covariances && !g_u && !g_matrices) return PIGS_ERR_INVALID;
    if (g_matrices && !it_scratch_ok(scratch, scratch_bytes, N, c, p)) return PIGS_ERR_INVALID;
    const void* const in[8] = {nullptr, full_covariances, u, nullptr, sample_u, sample_ux, sample_uxx, sample_pde};
    const int64_t tiles = (N + 15) / 16, records = mlp_records(N);
    float* recs = g_matrices ? (float*)scratch + IT_HEAD : nullptr;
    clear_hip_error();
    hipLaunchKernelGGL(it_apply_backward_kernel, dim3((unsigned)((records + MLP_WAVES - 1) / MLP_WAVES)), dim3(64 * MLP_WAVES),
                       0, (hipStream_t)stream, N, tiles, c, p, (const float*)matrices, it_rows(c, p, in),
                       (const float*)g_t_params, (float*)g_full_covariances, (float*)g_u, recs);
    if (g_matrices) {
        const int PM = it_matrix_floats(c, p);
        hipLaunchKernelGGL(it_sum_records_kernel, dim3((unsigned)((PM + 63) / 64)), dim3(256), 0, (hipStream_t)stream, PM,
                           (int)records, (const float*)recs, (float*)g_matrices);
    }
    return launch_status();
}

}  // extern "C"
