// The model's state update: the network's deltas applied to the Gaussians, the next covariances and the conservation
// penalty in TWO launches forward and ONE backward.
//
// Replaces, per time step, the tail of Model.forward and the delta terms of compute_loss in model_pn.py: the four
// strided column slices of the network's output (:270-273), six detach().clone() of the previous state (:677-682; the
// inputs are never written, so they ARE the previous state), the masked update (:684-687), the periodic wrap of the
// means (:689-693, two boolean-index writes with a host wait each), build_full_covariances + flatten_covariances
// (:695-698) and the four masked mean squares (:878-882, four boolean indexings with a host wait each).
//
//   m = 1 on a free row (boundary_mask true), 0 on a boundary row; deltas row = (dmeans[2], dscaling[2], dtransforms[1], du[c])
//   means' = means + dmeans m       scaling' = scaling exp(dscaling m)
//   transforms' = transforms + dtransforms m       u' = u + du m
//   wrap: a coordinate of means' > hi is lowered by hi - lo, one < lo raised by it (one shift, strict inequalities)
//   covariances / conics of (scaling', transforms'): cov_terms.h with the expressions of covariances.hip, flat and 2 x 2
//   penalty[k] = sum over free rows of the squares of block k / (n_free width_k),  k = dmeans, dscaling, dtransforms, du
// A boundary row copies its inputs bit for bit; its deltas are never used in arithmetic (they may be NaN or Inf).
//
// The penalty: every thread accumulates its row's four squared sums and its free flag in double; a workgroup adds them
// across each wave, then across its four waves through LDS, and writes ONE record of 5 doubles; the finishing launch
// (one workgroup) adds the records in a fixed order.  No float atomics: the penalty is a pure function of the inputs.
// scratch: record 0 = the totals (4 sums, n_free; the backward reads n_free there), record 1 + b = workgroup b's.
#include <hip/hip_runtime.h>

#include "cov_terms.h"
#include "launch.h"

namespace pigs {

constexpr int ADVANCE_RECORD = PIGS_ADVANCE_RECORD;      // doubles per record: four squared sums and the free-row count

template <typename T>
struct alignas(2 * sizeof(T)) Pair {     // a means / scaling row: one 8-byte (float) or 16-byte (double) access
    T x, y;
};

template <typename T>
struct AdvanceForward {
    const T *means, *u, *scaling, *transforms, *deltas;
    const uint8_t* mask;
    T *o_means, *o_u, *o_scaling, *o_transforms, *o_cov, *o_conic, *o_full_cov, *o_full_conic, *penalty;
    double* scratch;
    double lo, hi;
    int wrap, c;
};

template <typename T>
struct AdvanceBackward {
    const T *o_scaling, *o_transforms, *deltas;
    const uint8_t* mask;
    const double* scratch;
    // incoming gradients, null = zero
    const T *go_means, *go_u, *go_scaling, *go_transforms, *go_cov, *go_conic, *go_full_cov, *go_full_conic, *go_penalty;
    T *g_means, *g_u, *g_scaling, *g_transforms, *g_deltas;      // null = not wanted
    int c;
};

// the sum of `v` over the workgroup's 256 threads in thread 0: across each wave, then the four waves in order
__device__ __forceinline__ void block_sum(double (&v)[ADVANCE_RECORD], double (*lds)[ADVANCE_RECORD]) {
    for (int k = 0; k < ADVANCE_RECORD; ++k)
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < ADVANCE_RECORD; ++k) lds[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < ADVANCE_RECORD; ++k) v[k] = ((lds[0][k] + lds[1][k]) + lds[2][k]) + lds[3][k];
}

template <typename T>
__global__ __launch_bounds__(256) void advance_forward_kernel(int64_t N, AdvanceForward<T> a) {
    __shared__ double lds[4][ADVANCE_RECORD];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double acc[ADVANCE_RECORD] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < N) {
        const int c = a.c, w = 5 + c;
        const bool free_row = a.mask[i] != 0;
        Pair<T> mu = reinterpret_cast<const Pair<T>*>(a.means)[i];
        Pair<T> s = reinterpret_cast<const Pair<T>*>(a.scaling)[i];
        T t = a.transforms[i];
        const T* __restrict__ d = a.deltas + i * w;
        if (free_row) {
            const T dmx = d[0], dmy = d[1], dsx = d[2], dsy = d[3], dt = d[4];
            mu.x += dmx;
            mu.y += dmy;
            s.x *= exp(dsx);
            s.y *= exp(dsy);
            t += dt;
            acc[0] = fma((double)dmx, (double)dmx, (double)dmy * (double)dmy);
            acc[1] = fma((double)dsx, (double)dsx, (double)dsy * (double)dsy);
            acc[2] = (double)dt * (double)dt;
            acc[4] = 1.0;
            for (int j = 0; j < c; ++j) {
                const T du = d[5 + j];
                a.o_u[i * c + j] = a.u[i * c + j] + du;
                acc[3] = fma((double)du, (double)du, acc[3]);
            }
        } else {
            for (int j = 0; j < c; ++j) a.o_u[i * c + j] = a.u[i * c + j];
        }
        if (a.wrap) {                                           // one shift, strict inequalities (model_pn.py:689-693)
            const T lo = T(a.lo), hi = T(a.hi), period = T(a.hi - a.lo);
            if (mu.x > hi) mu.x -= period;
            if (mu.x < lo) mu.x += period;
            if (mu.y > hi) mu.y -= period;
            if (mu.y < lo) mu.y += period;
        }
        reinterpret_cast<Pair<T>*>(a.o_means)[i] = mu;
        reinterpret_cast<Pair<T>*>(a.o_scaling)[i] = s;
        a.o_transforms[i] = t;
        const T sv[2] = {s.x, s.y};
        const CovTerms<T> k(sv, &t, 0);
        const T cxy = k.h * k.r, qxx = k.k / k.s0, qxy = -k.h * k.k / k.r, qyy = k.k / k.s1;
        a.o_cov[3 * i] = k.s0;
        a.o_cov[3 * i + 1] = cxy;
        a.o_cov[3 * i + 2] = k.s1;
        a.o_conic[3 * i] = qxx;
        a.o_conic[3 * i + 1] = qxy;
        a.o_conic[3 * i + 2] = qyy;
        a.o_full_cov[4 * i] = k.s0;                             // the symmetric entry twice: no stack launches
        a.o_full_cov[4 * i + 1] = cxy;
        a.o_full_cov[4 * i + 2] = cxy;
        a.o_full_cov[4 * i + 3] = k.s1;
        a.o_full_conic[4 * i] = qxx;
        a.o_full_conic[4 * i + 1] = qxy;
        a.o_full_conic[4 * i + 2] = qxy;
        a.o_full_conic[4 * i + 3] = qyy;
    }
    block_sum(acc, lds);
    if (threadIdx.x == 0)
        for (int k = 0; k < ADVANCE_RECORD; ++k) a.scratch[((int64_t)blockIdx.x + 1) * ADVANCE_RECORD + k] = acc[k];
}

// one workgroup: thread t adds records 1 + t, 1 + t + 256, ... in that order, then the workgroup's sum as above
template <typename T>
__global__ __launch_bounds__(256) void advance_finish_kernel(int64_t blocks, int c, double* __restrict__ scratch,
                                                             T* __restrict__ penalty) {
    __shared__ double lds[4][ADVANCE_RECORD];
    double acc[ADVANCE_RECORD] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t b = threadIdx.x; b < blocks; b += 256)
        for (int k = 0; k < ADVANCE_RECORD; ++k) acc[k] += scratch[(b + 1) * ADVANCE_RECORD + k];
    block_sum(acc, lds);
    if (threadIdx.x == 0) {
        const double width[4] = {2.0, 2.0, 1.0, (double)c};
        for (int k = 0; k < ADVANCE_RECORD; ++k) scratch[k] = acc[k];
        for (int k = 0; k < 4; ++k) penalty[k] = T(acc[k] / (acc[4] * width[k]));      // no free row: 0 / 0 = NaN, as torch
    }
}

template <typename T>
__global__ __launch_bounds__(256) void advance_backward_kernel(int64_t N, AdvanceBackward<T> a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int c = a.c, w = 5 + c;
    const bool free_row = a.mask[i] != 0;
    Pair<T> g_mu{T(0), T(0)}, g_s{T(0), T(0)};
    T g_t = T(0);
    if (a.go_means) g_mu = reinterpret_cast<const Pair<T>*>(a.go_means)[i];
    if (a.go_scaling) g_s = reinterpret_cast<const Pair<T>*>(a.go_scaling)[i];
    if (a.go_transforms) g_t = a.go_transforms[i];
    const Pair<T> s = reinterpret_cast<const Pair<T>*>(a.o_scaling)[i];      // scaling'

    if (a.go_cov || a.go_conic || a.go_full_cov || a.go_full_conic) {
        // gradients of <g_cov, cov> + <g_conic, conic> wrt scaling' and transforms': the arithmetic of
        // build_covariances_backward_kernel; a full matrix folds into the flat triple, xy receives both off-diagonals
        const T t = a.o_transforms[i];
        const T sv[2] = {s.x, s.y};
        const CovTerms<T> k(sv, &t, 0);
        T gxx = 0, gxy = 0, gyy = 0, qxx = 0, qxy = 0, qyy = 0;
        if (a.go_cov) { gxx = a.go_cov[3 * i]; gxy = a.go_cov[3 * i + 1]; gyy = a.go_cov[3 * i + 2]; }
        if (a.go_full_cov) {
            gxx += a.go_full_cov[4 * i];
            gxy += a.go_full_cov[4 * i + 1] + a.go_full_cov[4 * i + 2];
            gyy += a.go_full_cov[4 * i + 3];
        }
        if (a.go_conic) { qxx = a.go_conic[3 * i]; qxy = a.go_conic[3 * i + 1]; qyy = a.go_conic[3 * i + 2]; }
        if (a.go_full_conic) {
            qxx += a.go_full_conic[4 * i];
            qxy += a.go_full_conic[4 * i + 1] + a.go_full_conic[4 * i + 2];
            qyy += a.go_full_conic[4 * i + 3];
        }
        const T tau = k.h * k.r, hk = k.h * k.k;
        const T half = T(0.5);
        g_s.x += gxx + half * gxy * tau / k.s0 - qxx * k.k / (k.s0 * k.s0) + half * qxy * hk / (k.r * k.s0);
        g_s.y += gyy + half * gxy * tau / k.s1 - qyy * k.k / (k.s1 * k.s1) + half * qxy * hk / (k.r * k.s1);
        const T g_h = gxy * k.r + T(2) * hk * k.k * (qxx / k.s0 + qyy / k.s1) - qxy * k.k * k.k * (T(1) + k.h * k.h) / k.r;
        g_t += g_h / k.k;                                       // dh/dt = 1 - h^2
    }

    const T* __restrict__ d = a.deltas + i * w;
    if (a.g_means) reinterpret_cast<Pair<T>*>(a.g_means)[i] = g_mu;      // the wrap passes the gradient through
    if (a.g_transforms) a.g_transforms[i] = g_t;
    if (a.g_scaling) {                                          // d scaling' / d scaling = exp(dscaling m)
        Pair<T> g = g_s;
        if (free_row) {
            g.x *= exp(d[2]);
            g.y *= exp(d[3]);
        }
        reinterpret_cast<Pair<T>*>(a.g_scaling)[i] = g;
    }
    if (a.g_u)
        for (int j = 0; j < c; ++j) a.g_u[i * c + j] = a.go_u ? a.go_u[i * c + j] : T(0);
    if (a.g_deltas) {
        T* __restrict__ g = a.g_deltas + i * w;
        if (!free_row) {                                        // m = 0: nothing reaches the deltas, whatever they hold
            for (int j = 0; j < w; ++j) g[j] = T(0);
            return;
        }
        T pen[4] = {T(0), T(0), T(0), T(0)};                    // 2 g_penalty[k] / (n_free width_k)
        if (a.go_penalty) {
            const double n_free = a.scratch[4];
            const double width[4] = {2.0, 2.0, 1.0, (double)c};
            for (int k = 0; k < 4; ++k) pen[k] = T(2.0 * (double)a.go_penalty[k] / (n_free * width[k]));
        }
        g[0] = g_mu.x + pen[0] * d[0];
        g[1] = g_mu.y + pen[0] * d[1];
        g[2] = g_s.x * s.x + pen[1] * d[2];                     // d scaling' / d dscaling = scaling'
        g[3] = g_s.y * s.y + pen[1] * d[3];
        g[4] = g_t + pen[2] * d[4];
        for (int j = 0; j < c; ++j) g[5 + j] = (a.go_u ? a.go_u[i * c + j] : T(0)) + pen[3] * d[5 + j];
    }
}

size_t advance_scratch_bytes(int64_t N) {
    if (N <= 0) return 0;
    return (size_t)((N + 255) / 256 + 1) * ADVANCE_RECORD * sizeof(double);
}

template <typename T>
static int launch_forward(const AdvanceStep& s, hipStream_t stream) {
    const int64_t blocks = (s.N + 255) / 256;
    if (blocks > 0x7fffffffLL) return PIGS_ERR_INVALID;
    AdvanceForward<T> a;
    a.means = (const T*)s.in[0]; a.u = (const T*)s.in[1]; a.scaling = (const T*)s.in[2]; a.transforms = (const T*)s.in[3];
    a.deltas = (const T*)s.deltas;
    a.mask = s.mask;
    a.o_means = (T*)s.out[0]; a.o_u = (T*)s.out[1]; a.o_scaling = (T*)s.out[2]; a.o_transforms = (T*)s.out[3];
    a.o_cov = (T*)s.out[4]; a.o_conic = (T*)s.out[5]; a.o_full_cov = (T*)s.out[6]; a.o_full_conic = (T*)s.out[7];
    a.penalty = (T*)s.out[8];
    a.scratch = (double*)s.scratch;
    a.lo = s.lo; a.hi = s.hi; a.wrap = s.wrap; a.c = s.c;
    clear_hip_error();
    hipLaunchKernelGGL(advance_forward_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, stream, s.N, a);
    hipLaunchKernelGGL(advance_finish_kernel<T>, dim3(1), dim3(256), 0, stream, blocks, s.c, a.scratch, a.penalty);
    return launch_status();
}

int advance_forward(const AdvanceStep& s, hipStream_t stream) {
    if (s.dtype == PIGS_F32) return launch_forward<float>(s, stream);
    if (s.dtype == PIGS_F64) return launch_forward<double>(s, stream);
    return PIGS_ERR_UNSUPPORTED;
}

template <typename T>
static int launch_backward(const AdvanceStep& s, hipStream_t stream) {
    const int64_t blocks = (s.N + 255) / 256;
    if (blocks > 0x7fffffffLL) return PIGS_ERR_INVALID;
    AdvanceBackward<T> a;
    a.o_scaling = (const T*)s.in[2]; a.o_transforms = (const T*)s.in[3];
    a.deltas = (const T*)s.deltas;
    a.mask = s.mask;
    a.scratch = (const double*)s.scratch;
    a.go_means = (const T*)s.gout[0]; a.go_u = (const T*)s.gout[1]; a.go_scaling = (const T*)s.gout[2];
    a.go_transforms = (const T*)s.gout[3]; a.go_cov = (const T*)s.gout[4]; a.go_conic = (const T*)s.gout[5];
    a.go_full_cov = (const T*)s.gout[6]; a.go_full_conic = (const T*)s.gout[7]; a.go_penalty = (const T*)s.gout[8];
    a.g_means = (T*)s.out[0]; a.g_u = (T*)s.out[1]; a.g_scaling = (T*)s.out[2]; a.g_transforms = (T*)s.out[3];
    a.g_deltas = (T*)s.out[4];
    a.c = s.c;
    clear_hip_error();
    hipLaunchKernelGGL(advance_backward_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, stream, s.N, a);
    return launch_status();
}

int advance_backward(const AdvanceStep& s, hipStream_t stream) {
    if (s.dtype == PIGS_F32) return launch_backward<float>(s, stream);
    if (s.dtype == PIGS_F64) return launch_backward<double>(s, stream);
    return PIGS_ERR_UNSUPPORTED;
}

}  // namespace pigs
