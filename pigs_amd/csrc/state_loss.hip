// The TEST problem's state terms: the eight unweighted terms of pde_loss, bc_loss and conservation_loss that read the
// Gaussians' new state and the network's deltas, in ONE launch forward (two above STATE_LOSS_ONE_LAUNCH_ROWS rows) and
// ONE backward.  No host decision, nothing read back.
//
// Replaces, per time step of Problem.TEST, model_pn.py:851-852 (pde_loss), :854-861 (bc_loss, two `if torch.any`) and
// :866-876 (conservation_loss, one `if torch.any`): about seventeen boolean indexings with a host wait each.
//
//   over the FREE rows (boundary_mask nonzero), F their count, y = means[:, 1], dx, dy = deltas[:, 0], deltas[:, 1],
//   du = deltas[:, 5:5 + c], u0 = u[:, 0];  LOW = {y < -wall}, HIGH = {y > wall}, MID = {|y| < wall}, compared in the
//   dtype with wall rounded to it (a row at +-wall or with a NaN height is in no set):
//   terms[0] drift          sum (dy - u0 / drift)^2 / F                    (the division in the dtype)
//   terms[1] wall_low       sum_LOW sum_c (u - 1)^2 / (|LOW| c)            0 when LOW is empty
//   terms[2] wall_high      sum_HIGH sum_c (u + 1)^2 / (|HIGH| c)          0 when HIGH is empty
//   terms[3] dmeans_x       sum dx^2 / F
//   terms[4] dmeans_spread  sum [(dx - mean dx)^2 + (dy - mean dy)^2] / (2 F)
//   terms[5] height_spread  sum (y - mean y)^2 / F
//   terms[6] unit_u         sum_MID (|u0| - 1)^2 / |MID|                   0 when MID is empty
//   terms[7] du_mid         sum_MID sum_c du^2 / (|MID| c)                 0 when MID is empty
// With F = 0 the entries 0, 3, 4, 5 are NaN (0 / 0, torch.mean of nothing).  A boundary row is branched around: its
// state and deltas take part in no arithmetic.
//
// The three spreads are CENTRED sums.  A workgroup first adds F and the plain sums of dx, dy, y (pass 1), takes
// K = sum / F as its centre, and then adds A1 = sum (x - K) and A2 = sum (x - K)^2 over the same rows, which it kept in
// registers (pass 2).  sum (x - mean)^2 = A2 - A1^2 / F exactly, and with K within a rounding error of the mean A1^2 / F
// is a correction of second order, not a cancellation.  Records of several workgroups are moved to ONE common centre
// K' (d = K - K' is an exact difference of two nearby doubles): A1' = A1 + n d, A2' = A2 + 2 d A1 + n d^2.  All
// accumulators are double; sums go across a wave by shuffles, across the waves through LDS in wave order, across
// workgroups in record order.  No float atomics: the same inputs give the same bits.
//
// scratch (doubles): [0, 8) the statistics record F, |LOW|, |HIGH|, |MID|, mean dx, mean dy, mean y, 0 (the backward
// reads it); above the one-launch bound, then one record of STATE_LOSS_RECORD doubles per workgroup of 256 rows:
// F, K[3], then the 15 sums of pass 2.
#include <hip/hip_runtime.h>

#include "launch.h"

namespace pigs {

constexpr int SL_STATS = PIGS_STATE_LOSS_STATS;
constexpr int SL_RECORD = PIGS_STATE_LOSS_RECORD;
constexpr int SL_P = 4;       // pass 1: F, sum dx, sum dy, sum y
constexpr int SL_Q = 15;      // pass 2: |LOW|, |HIGH|, |MID|, the six plain sums (terms 0, 1, 2, 3, 6, 7), A1[3], A2[3]
enum { Q_LOW = 0, Q_HIGH, Q_MID, Q_DRIFT, Q_WALL_LOW, Q_WALL_HIGH, Q_DX2, Q_UNIT, Q_DU, Q_A1, Q_A2 = Q_A1 + 3 };
static_assert(Q_A2 + 3 == SL_Q && 1 + 3 + SL_Q <= SL_RECORD, "the record holds F, K[3] and the sums of pass 2");

template <typename T>
struct StateLossForward {
    const T *means, *u, *deltas;
    const uint8_t* mask;
    double* scratch;
    T* terms;
    double wall, drift;
    int c;
};

template <typename T>
struct StateLossBackward {
    const T *means, *u, *deltas, *g;
    const uint8_t* mask;
    const double* stats;
    T *g_means, *g_u, *g_deltas;      // null = not wanted
    double wall, drift;
    int c;
};

// the sum of `v` over the workgroup in EVERY thread: across each wave by shuffles, then thread k adds entry k of the
// waves' partial sums in wave order and every thread reads the K totals back
template <int K, int WAVES>
__device__ __forceinline__ void block_sum_all(double (&v)[K], double (*lds)[K], double* total) {
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) lds[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double s = lds[0][threadIdx.x];
        for (int w = 1; w < WAVES; ++w) s += lds[w][threadIdx.x];
        total[threadIdx.x] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = total[k];
}

template <typename T>
struct Membership {
    bool low, high, mid;
    __device__ __forceinline__ Membership(T y, T wall) {      // strict, in the dtype; NaN fails all three
        low = y < -wall;
        high = y > wall;
        mid = (y < T(0) ? -y : y) < wall;
    }
};

// the eight terms and the statistics record from the totals about the centre K; one thread
template <typename T>
__device__ void state_loss_finish(double F, const double (&K)[3], const double (&q)[SL_Q], int c,
                                  double* __restrict__ stats, T* __restrict__ terms) {
    double m2[3], mean[3];
    for (int v = 0; v < 3; ++v) {
        const double a1 = q[Q_A1 + v];
        m2[v] = q[Q_A2 + v] - a1 * a1 / F;       // F = 0: NaN, as torch.mean of nothing
        if (m2[v] < 0.0) m2[v] = 0.0;            // a rounding error below zero; NaN stays
        mean[v] = K[v] + a1 / F;
    }
    const double n_low = q[Q_LOW], n_high = q[Q_HIGH], n_mid = q[Q_MID], width = (double)c;
    terms[0] = T(q[Q_DRIFT] / F);
    terms[1] = n_low > 0.0 ? T(q[Q_WALL_LOW] / (n_low * width)) : T(0);
    terms[2] = n_high > 0.0 ? T(q[Q_WALL_HIGH] / (n_high * width)) : T(0);
    terms[3] = T(q[Q_DX2] / F);
    terms[4] = T((m2[0] + m2[1]) / (2.0 * F));
    terms[5] = T(m2[2] / F);
    terms[6] = n_mid > 0.0 ? T(q[Q_UNIT] / n_mid) : T(0);
    terms[7] = n_mid > 0.0 ? T(q[Q_DU] / (n_mid * width)) : T(0);
    stats[0] = F;
    stats[1] = n_low;
    stats[2] = n_high;
    stats[3] = n_mid;
    stats[4] = mean[0];
    stats[5] = mean[1];
    stats[6] = mean[2];
    stats[7] = 0.0;
}

// THREADS x R rows per workgroup.  SINGLE: the only workgroup, it finishes; otherwise it writes record blockIdx.x.
template <typename T, int THREADS, int R, bool SINGLE>
__global__ __launch_bounds__(THREADS) void state_loss_rows_kernel(int64_t N, StateLossForward<T> a) {
    constexpr int WAVES = THREADS / 64;
    __shared__ double lds_p[WAVES][SL_P], total_p[SL_P];
    __shared__ double lds_q[WAVES][SL_Q], total_q[SL_Q];
    const int c = a.c, w = 5 + c;
    const T wall = T(a.wall), drift = T(a.drift);
    const int64_t first = (int64_t)blockIdx.x * (THREADS * R) + threadIdx.x;
    bool free_row[R];
    T x[R][3], u0s[R];                           // dx, dy, y (kept for pass 2) and u0 of this thread's rows
    double p[SL_P], q[SL_Q];
    for (int k = 0; k < SL_P; ++k) p[k] = 0.0;
    for (int k = 0; k < SL_Q; ++k) q[k] = 0.0;
    // every row's loads first, whatever its mask says, so that they are in flight together (a row past the end reads
    // row N - 1); a boundary row's values are loaded and then take part in no arithmetic
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t i = first + (int64_t)r * THREADS, j = i < N ? i : N - 1;
        free_row[r] = a.mask[j] != 0 && i < N;
        x[r][0] = a.deltas[j * w];
        x[r][1] = a.deltas[j * w + 1];
        x[r][2] = a.means[2 * j + 1];
        u0s[r] = a.u[j * c];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (!free_row[r]) continue;
        const int64_t i = first + (int64_t)r * THREADS;
        const T* __restrict__ d = a.deltas + i * w;
        const T* __restrict__ ur = a.u + i * c;
        const T dx = x[r][0], dy = x[r][1], y = x[r][2], u0 = u0s[r];
        p[0] += 1.0;
        p[1] += (double)dx;
        p[2] += (double)dy;
        p[3] += (double)y;
        const double e = (double)dy - (double)(u0 / drift);
        q[Q_DRIFT] = fma(e, e, q[Q_DRIFT]);
        q[Q_DX2] = fma((double)dx, (double)dx, q[Q_DX2]);
        const Membership<T> in(y, wall);
        if (in.low) {
            q[Q_LOW] += 1.0;
            for (int j = 0; j < c; ++j) {
                const double t = (double)ur[j] - 1.0;
                q[Q_WALL_LOW] = fma(t, t, q[Q_WALL_LOW]);
            }
        }
        if (in.high) {
            q[Q_HIGH] += 1.0;
            for (int j = 0; j < c; ++j) {
                const double t = (double)ur[j] + 1.0;
                q[Q_WALL_HIGH] = fma(t, t, q[Q_WALL_HIGH]);
            }
        }
        if (in.mid) {
            q[Q_MID] += 1.0;
            const double t = fabs((double)u0) - 1.0;
            q[Q_UNIT] = fma(t, t, q[Q_UNIT]);
            for (int j = 0; j < c; ++j) {
                const double du = (double)d[5 + j];
                q[Q_DU] = fma(du, du, q[Q_DU]);
            }
        }
    }
    block_sum_all<SL_P, WAVES>(p, lds_p, total_p);
    const double F = p[0];
    const double K[3] = {p[1] / F, p[2] / F, p[3] / F};      // no free row here: NaN, and no row below reads it
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (!free_row[r]) continue;
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const double t = (double)x[r][v] - K[v];
            q[Q_A1 + v] += t;
            q[Q_A2 + v] = fma(t, t, q[Q_A2 + v]);
        }
    }
    block_sum_all<SL_Q, WAVES>(q, lds_q, total_q);
    if (threadIdx.x != 0) return;
    if (SINGLE) {
        state_loss_finish<T>(F, K, q, c, a.scratch, a.terms);
    } else {
        double* __restrict__ rec = a.scratch + SL_STATS + (int64_t)blockIdx.x * SL_RECORD;
        rec[0] = F;
        for (int v = 0; v < 3; ++v) rec[1 + v] = K[v];
        for (int k = 0; k < SL_Q; ++k) rec[4 + k] = q[k];
        for (int k = 4 + SL_Q; k < SL_RECORD; ++k) rec[k] = 0.0;
    }
}

// one workgroup: thread t takes records t, t + 256, ... in that order.  First the common centre K' = sum n K / sum n
// over the records that hold a free row, then every record moved to it.
template <typename T>
__global__ __launch_bounds__(256) void state_loss_finish_kernel(int64_t blocks, int c, double* __restrict__ scratch,
                                                                T* __restrict__ terms) {
    __shared__ double lds_p[4][SL_P], total_p[SL_P];
    __shared__ double lds_q[4][SL_Q], total_q[SL_Q];
    const double* __restrict__ recs = scratch + SL_STATS;
    double p[SL_P], q[SL_Q];
    for (int k = 0; k < SL_P; ++k) p[k] = 0.0;
    for (int k = 0; k < SL_Q; ++k) q[k] = 0.0;
    for (int64_t b = threadIdx.x; b < blocks; b += 256) {
        const double* rec = recs + b * SL_RECORD;
        const double n = rec[0];
        if (n > 0.0) {
            p[0] += n;
#pragma unroll
            for (int v = 0; v < 3; ++v) p[1 + v] = fma(n, rec[1 + v], p[1 + v]);
        }
    }
    block_sum_all<SL_P, 4>(p, lds_p, total_p);
    const double F = p[0];
    const double K[3] = {p[1] / F, p[2] / F, p[3] / F};
    for (int64_t b = threadIdx.x; b < blocks; b += 256) {
        const double* rec = recs + b * SL_RECORD;
        const double n = rec[0];
        if (!(n > 0.0)) continue;                 // no free row: every sum of the record is zero and its K is NaN
#pragma unroll
        for (int k = 0; k < Q_A1; ++k) q[k] += rec[4 + k];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const double d = rec[1 + v] - K[v], a1 = rec[4 + Q_A1 + v], a2 = rec[4 + Q_A2 + v];
            q[Q_A1 + v] += fma(n, d, a1);
            q[Q_A2 + v] += a2 + d * fma(n, d, 2.0 * a1);
        }
    }
    block_sum_all<SL_Q, 4>(q, lds_q, total_q);
    if (threadIdx.x == 0) state_loss_finish<T>(F, K, q, c, scratch, terms);
}

template <typename T>
__global__ __launch_bounds__(256) void state_loss_backward_kernel(int64_t N, StateLossBackward<T> a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int c = a.c, w = 5 + c;
    if (a.mask[i] == 0) {                         // a boundary row: exact zeros, whatever its state and deltas hold
        if (a.g_means) a.g_means[2 * i] = a.g_means[2 * i + 1] = T(0);
        if (a.g_u)
            for (int j = 0; j < c; ++j) a.g_u[i * c + j] = T(0);
        if (a.g_deltas)
            for (int j = 0; j < w; ++j) a.g_deltas[i * w + j] = T(0);
        return;
    }
    const double F = a.stats[0], n_low = a.stats[1], n_high = a.stats[2], n_mid = a.stats[3];
    const double mean_dx = a.stats[4], mean_dy = a.stats[5], mean_y = a.stats[6];
    const T drift = T(a.drift);
    const T* __restrict__ d = a.deltas + i * w;
    const T* __restrict__ ur = a.u + i * c;
    const T y = a.means[2 * i + 1], u0 = ur[0];
    const double dx = (double)d[0], dy = (double)d[1], width = (double)c;
    const double e = dy - (double)(u0 / drift);
    const Membership<T> in(y, T(a.wall));
    if (a.g_means) {
        a.g_means[2 * i] = T(0);
        a.g_means[2 * i + 1] = T(2.0 * (double)a.g[5] * ((double)y - mean_y) / F);
    }
    if (a.g_deltas) {
        T* __restrict__ g = a.g_deltas + i * w;
        const double g4 = (double)a.g[4];
        g[0] = T((2.0 * (double)a.g[3] * dx + g4 * (dx - mean_dx)) / F);
        g[1] = T((2.0 * (double)a.g[0] * e + g4 * (dy - mean_dy)) / F);
        g[2] = g[3] = g[4] = T(0);
        const double k7 = in.mid ? 2.0 * (double)a.g[7] / (n_mid * width) : 0.0;
        for (int j = 0; j < c; ++j) g[5 + j] = in.mid ? T(k7 * (double)d[5 + j]) : T(0);
    }
    if (a.g_u) {
        const double k1 = in.low ? 2.0 * (double)a.g[1] / (n_low * width) : 0.0;
        const double k2 = in.high ? 2.0 * (double)a.g[2] / (n_high * width) : 0.0;
        for (int j = 0; j < c; ++j) {
            const double uj = (double)ur[j];
            double v = 0.0;
            if (in.low) v += k1 * (uj - 1.0);
            if (in.high) v += k2 * (uj + 1.0);
            if (j == 0) {
                v -= 2.0 * (double)a.g[0] * e / ((double)drift * F);
                if (in.mid) {
                    const double sign = uj > 0.0 ? 1.0 : (uj < 0.0 ? -1.0 : 0.0);      // sign(0) = 0, as torch
                    v += 2.0 * (double)a.g[6] * (fabs(uj) - 1.0) * sign / n_mid;
                }
            }
            a.g_u[i * c + j] = T(v);
        }
    }
}

size_t state_loss_scratch_bytes(int64_t N) {
    if (N <= 0) return 0;
    const int64_t records = N <= STATE_LOSS_ONE_LAUNCH_ROWS ? 0 : (N + 255) / 256;
    return (size_t)(SL_STATS + records * SL_RECORD) * sizeof(double);
}

template <typename T>
static int launch_forward(const StateLossStep& s, hipStream_t stream) {
    const int64_t blocks = (s.N + 255) / 256;
    if (blocks > 0x7fffffffLL) return PIGS_ERR_INVALID;
    StateLossForward<T> a;
    a.means = (const T*)s.means; a.u = (const T*)s.u; a.deltas = (const T*)s.deltas;
    a.mask = s.mask;
    a.scratch = (double*)s.scratch;
    a.terms = (T*)s.terms;
    a.wall = s.wall; a.drift = s.drift; a.c = s.c;
    clear_hip_error();
    if (s.N <= 256) {
        hipLaunchKernelGGL((state_loss_rows_kernel<T, 256, 1, true>), dim3(1), dim3(256), 0, stream, s.N, a);
    } else if (s.N <= STATE_LOSS_ONE_LAUNCH_ROWS) {
        hipLaunchKernelGGL((state_loss_rows_kernel<T, 1024, 4, true>), dim3(1), dim3(1024), 0, stream, s.N, a);
    } else {
        hipLaunchKernelGGL((state_loss_rows_kernel<T, 256, 1, false>), dim3((unsigned)blocks), dim3(256), 0, stream, s.N, a);
        hipLaunchKernelGGL(state_loss_finish_kernel<T>, dim3(1), dim3(256), 0, stream, blocks, s.c, a.scratch, a.terms);
    }
    return launch_status();
}

int state_loss_forward(const StateLossStep& s, hipStream_t stream) {
    if (s.dtype == PIGS_F32) return launch_forward<float>(s, stream);
    if (s.dtype == PIGS_F64) return launch_forward<double>(s, stream);
    return PIGS_ERR_UNSUPPORTED;
}

template <typename T>
static int launch_backward(const StateLossStep& s, hipStream_t stream) {
    const int64_t blocks = (s.N + 255) / 256;
    if (blocks > 0x7fffffffLL) return PIGS_ERR_INVALID;
    StateLossBackward<T> a;
    a.means = (const T*)s.means; a.u = (const T*)s.u; a.deltas = (const T*)s.deltas; a.g = (const T*)s.g_terms;
    a.mask = s.mask;
    a.stats = (const double*)s.scratch;
    a.g_means = (T*)s.g_means; a.g_u = (T*)s.g_u; a.g_deltas = (T*)s.g_deltas;
    a.wall = s.wall; a.drift = s.drift; a.c = s.c;
    clear_hip_error();
    hipLaunchKernelGGL(state_loss_backward_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, stream, s.N, a);
    return launch_status();
}

int state_loss_backward(const StateLossStep& s, hipStream_t stream) {
    if (s.dtype == PIGS_F32) return launch_backward<float>(s, stream);
    if (s.dtype == PIGS_F64) return launch_backward<double>(s, stream);
    return PIGS_ERR_UNSUPPORTED;
}

}  // namespace pigs
