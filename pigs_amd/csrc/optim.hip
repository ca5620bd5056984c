// The optimiser of the MLP-free loops: the Gaussians' parameterisation, its chain rule and Adam in ONE launch.
//
// Replaces, per step, the chain around the sampler in test_no_mlp.py:99-104, 146, 185-186 and
// test_initialize.py:100-111, 151, 172-180: tanh(raw_means) * scale, exp(raw_scaling), build_covariances, the
// autograd backward of each, torch.optim.Adam over four tensors, zero_grad and the periodic wrap of the means.
//
//   mu = tanh(raw_means) * scale  (or raw_means)          s = exp(raw_scaling)
//   h = tanh(t), r = sqrt(s0 s1), k = 1 / (1 - h^2)       covariance = (s0, h r, s1), conic = (k / s0, -h k / r, k / s1)
// The step kernel, one thread per Gaussian: chain rule from (d mu, d cov or null, d conic or null) to the raw
// parameters, Adam as torch.optim.Adam defines it, the wrap, and the NEXT step's mu / covariance / conic from the
// updated parameters.  The materialising kernel is that last part alone (the same device function, so the two agree
// bit for bit).  1 / (1 - h^2) and sech^2 come from e = exp(-2 |x|), never from a cancelling subtraction.
//
// The four groups (means, values, scaling, transform) each have their own rate and their own running products
// beta1^t, beta2^t (doubles).  The products arrive in the kernel's argument block (host mode) or are read from a
// 12-double device state that a one-thread launch in front of the update advances (capturable mode); either way the
// bias corrections are formed from them on the device by the same double operations.
//
// Gradient statistics (optim_step_stats_kernel, and the 1-D kernels with STATS): the densification of the MLP-free
// loops thresholds sums of the RAW parameters' gradients (test_no_mlp.py:149-155, test_no_mlp_1d.py:156-162), which
// exist only in this kernel's registers.  With statistics a present group also keeps  last = G,  sum += G,
// norm += |sum| (the row norm of the sum AFTER adding), for G = d raw_means and G = d raw_scaling as Adam consumes them.
// The step body is one device function with a compile-time flag, so the kernels without statistics stay what they were.
//
// d = 1 (optim1d_*): mu = tanh(raw_means) * scale or raw_means, s = exp(raw_scaling), covariance = s, conic = 1 / s
// (test_no_mlp_1d.py:109-111); three groups (means, values, scaling) in slots 0..2 of the same argument block.
#include <hip/hip_runtime.h>

#include "adam_update.h"
#include "cov_terms.h"
#include "launch.h"

namespace pigs {

template <typename T>
struct alignas(2 * sizeof(T)) Pair {     // a raw_means / raw_scaling row: one 8-byte (float) or 16-byte (double) access
    T x, y;
};

struct AdamBlock {                       // the kernel's argument block: everything that is the same for every row
    double lr[4], pow1[4], pow2[4];      // per group: means, values, scaling, transform
    double beta1, beta2, eps, scale, lo, hi;
    const double* dev_lr;                // [4] or null: the rates on the device
    const double* dev_state;             // [12] or null: pow1[4], pow2[4], steps[4] on the device
    int tanh_map, wrap, c;
};

template <typename T>
struct OptimArrays {
    T *p[4], *m[4], *v[4];               // parameters, exp_avg, exp_avg_sq per group
    const T *g_means, *g_values, *g_cov, *g_conic;
    T *o_means, *o_cov, *o_conic;
};

template <typename T>
struct StatArrays {                      // per statistic: [0] of raw_means, [1] of raw_scaling (rows as the parameter's)
    T *sum[2], *norm[2], *last[2];
};

// sech(x)^2 = 4 e / (1 + e)^2 with e = exp(-2 |x|): no cancellation for large |x|
template <typename T>
__device__ __forceinline__ T sech2(T x) {
    const T e = exp(T(-2) * fabs(x));
    return T(4) * e / ((T(1) + e) * (T(1) + e));
}

// mu, covariance and conic of row i from its raw parameters: the forward of the parameterisation
template <typename T>
__device__ __forceinline__ void write_gaussian(int64_t i, Pair<T> rm, Pair<T> rs, T t, bool tanh_map, T scale,
                                               T* __restrict__ o_means, T* __restrict__ o_cov, T* __restrict__ o_conic) {
    Pair<T> mu = rm;
    if (tanh_map) mu = Pair<T>{tanh(rm.x) * scale, tanh(rm.y) * scale};
    reinterpret_cast<Pair<T>*>(o_means)[i] = mu;
    const T s[2] = {exp(rs.x), exp(rs.y)};
    const CovTerms<T> c(s, &t, 0);
    o_cov[3 * i] = c.s0;
    o_cov[3 * i + 1] = c.h * c.r;
    o_cov[3 * i + 2] = c.s1;
    o_conic[3 * i] = c.k / c.s0;
    o_conic[3 * i + 1] = -c.h * c.k / c.r;
    o_conic[3 * i + 2] = c.k / c.s1;
}

template <typename T>
__global__ __launch_bounds__(256) void optim_materialize_kernel(int64_t N, bool tanh_map, T scale,
                                                                const T* __restrict__ raw_means,
                                                                const T* __restrict__ raw_scaling,
                                                                const T* __restrict__ transform, T* __restrict__ o_means,
                                                                T* __restrict__ o_cov, T* __restrict__ o_conic) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    write_gaussian<T>(i, reinterpret_cast<const Pair<T>*>(raw_means)[i], reinterpret_cast<const Pair<T>*>(raw_scaling)[i],
                      transform[i], tanh_map, scale, o_means, o_cov, o_conic);
}

// One group's Adam constants, as torch.optim.Adam forms them: step_size = lr / (1 - beta1^t),
// denominator sqrt(v) / sqrt(1 - beta2^t) + eps.  Uniform over the launch.
template <typename T>
struct AdamGroup {
    T b1, omb1, b2, omb2, step_size, bc2_sqrt, eps;
    __device__ __forceinline__ AdamGroup(const AdamBlock& k, int g) {
        const double lr = k.dev_lr ? k.dev_lr[g] : k.lr[g];
        const double p1 = k.dev_state ? k.dev_state[g] : k.pow1[g];
        const double p2 = k.dev_state ? k.dev_state[4 + g] : k.pow2[g];
        b1 = T(k.beta1);
        omb1 = T(1.0 - k.beta1);
        b2 = T(k.beta2);
        omb2 = T(1.0 - k.beta2);
        step_size = T(lr / (1.0 - p1));
        bc2_sqrt = T(sqrt(1.0 - p2));
        eps = T(k.eps);
    }
    __device__ __forceinline__ T update(T p, T g, T& m, T& v) const {
        m = b1 * m + omb1 * g;
        v = b2 * v + omb2 * g * g;
        return p - step_size * (m / (sqrt(v) / bc2_sqrt + eps));
    }
};

// The same update with its multiply-adds written out is adam_update_fma(adam, p, g, m, v) of adam_update.h: the d = 1
// kernels with and without statistics must agree bit for bit.

// sum += g, norm += |sum| (of the sum after adding), last = g: one row of a group's statistics
template <typename T>
__device__ __forceinline__ void keep_stats(int64_t i, Pair<T> g, T* __restrict__ sum, T* __restrict__ norm,
                                           T* __restrict__ last) {
    Pair<T> acc = reinterpret_cast<Pair<T>*>(sum)[i];
    acc.x += g.x;
    acc.y += g.y;
    reinterpret_cast<Pair<T>*>(sum)[i] = acc;
    norm[i] += sqrt(acc.x * acc.x + acc.y * acc.y);
    reinterpret_cast<Pair<T>*>(last)[i] = g;
}

template <typename T, bool STATS>
__device__ __forceinline__ void optim_step_row(int64_t i, const AdamBlock& k, const OptimArrays<T>& a,
                                               const StatArrays<T>& st) {
    Pair<T> rm = reinterpret_cast<const Pair<T>*>(a.p[0])[i];
    Pair<T> rs = reinterpret_cast<const Pair<T>*>(a.p[2])[i];
    T t = a.p[3][i];

    if (a.g_means) {                                            // group 0: raw_means
        const AdamGroup<T> adam(k, 0);
        Pair<T> g = reinterpret_cast<const Pair<T>*>(a.g_means)[i];
        if (k.tanh_map) {
            g.x *= T(k.scale) * sech2(rm.x);
            g.y *= T(k.scale) * sech2(rm.y);
        }
        if constexpr (STATS) keep_stats<T>(i, g, st.sum[0], st.norm[0], st.last[0]);
        Pair<T> m = reinterpret_cast<Pair<T>*>(a.m[0])[i], v = reinterpret_cast<Pair<T>*>(a.v[0])[i];
        rm.x = adam.update(rm.x, g.x, m.x, v.x);
        rm.y = adam.update(rm.y, g.y, m.y, v.y);
        if (k.wrap) {                                           // one shift, strict inequalities (test_initialize.py:175-180)
            const T lo = T(k.lo), hi = T(k.hi), period = T(k.hi - k.lo);
            if (rm.x > hi) rm.x -= period;
            if (rm.x < lo) rm.x += period;
            if (rm.y > hi) rm.y -= period;
            if (rm.y < lo) rm.y += period;
        }
        reinterpret_cast<Pair<T>*>(a.p[0])[i] = rm;
        reinterpret_cast<Pair<T>*>(a.m[0])[i] = m;
        reinterpret_cast<Pair<T>*>(a.v[0])[i] = v;
    }

    if (a.g_values) {                                           // group 1: values pass through
        const AdamGroup<T> adam(k, 1);
        for (int j = 0; j < k.c; ++j) {
            const int64_t at = i * k.c + j;
            T m = a.m[1][at], v = a.v[1][at];
            a.p[1][at] = adam.update(a.p[1][at], a.g_values[at], m, v);
            a.m[1][at] = m;
            a.v[1][at] = v;
        }
    }

    if (a.g_cov || a.g_conic) {                                 // groups 2 and 3: raw_scaling, transform
        // gradients of <g_cov, cov> + <g_conic, conic> wrt s and t: the arithmetic of build_covariances_backward_kernel
        const T s[2] = {exp(rs.x), exp(rs.y)};
        const CovTerms<T> c(s, &t, 0);
        T gxx = 0, gxy = 0, gyy = 0, qxx = 0, qxy = 0, qyy = 0;
        if (a.g_cov) { gxx = a.g_cov[3 * i]; gxy = a.g_cov[3 * i + 1]; gyy = a.g_cov[3 * i + 2]; }
        if (a.g_conic) { qxx = a.g_conic[3 * i]; qxy = a.g_conic[3 * i + 1]; qyy = a.g_conic[3 * i + 2]; }
        const T tau = c.h * c.r, hk = c.h * c.k;
        const T half = T(0.5);
        const T g_s0 = gxx + half * gxy * tau / c.s0 - qxx * c.k / (c.s0 * c.s0) + half * qxy * hk / (c.r * c.s0);
        const T g_s1 = gyy + half * gxy * tau / c.s1 - qyy * c.k / (c.s1 * c.s1) + half * qxy * hk / (c.r * c.s1);
        const T g_h = gxy * c.r + T(2) * hk * c.k * (qxx / c.s0 + qyy / c.s1) - qxy * c.k * c.k * (T(1) + c.h * c.h) / c.r;
        const T g_t = g_h / c.k;                                // dh/dt = 1 - h^2
        {
            const AdamGroup<T> adam(k, 2);                      // ds/d raw_scaling = s
            if constexpr (STATS) keep_stats<T>(i, Pair<T>{g_s0 * c.s0, g_s1 * c.s1}, st.sum[1], st.norm[1], st.last[1]);
            Pair<T> m = reinterpret_cast<Pair<T>*>(a.m[2])[i], v = reinterpret_cast<Pair<T>*>(a.v[2])[i];
            rs.x = adam.update(rs.x, g_s0 * c.s0, m.x, v.x);
            rs.y = adam.update(rs.y, g_s1 * c.s1, m.y, v.y);
            reinterpret_cast<Pair<T>*>(a.p[2])[i] = rs;
            reinterpret_cast<Pair<T>*>(a.m[2])[i] = m;
            reinterpret_cast<Pair<T>*>(a.v[2])[i] = v;
        }
        {
            const AdamGroup<T> adam(k, 3);
            T m = a.m[3][i], v = a.v[3][i];
            t = adam.update(t, g_t, m, v);
            a.p[3][i] = t;
            a.m[3][i] = m;
            a.v[3][i] = v;
        }
    }

    write_gaussian<T>(i, rm, rs, t, k.tanh_map != 0, T(k.scale), a.o_means, a.o_cov, a.o_conic);
}

template <typename T>
__global__ __launch_bounds__(256) void optim_step_kernel(int64_t N, AdamBlock k, OptimArrays<T> a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    optim_step_row<T, false>(i, k, a, StatArrays<T>{});
}

template <typename T>
__global__ __launch_bounds__(256) void optim_step_stats_kernel(int64_t N, AdamBlock k, OptimArrays<T> a, StatArrays<T> st) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    optim_step_row<T, true>(i, k, a, st);
}

// ---- d = 1 ---------------------------------------------------------------------------------------------------
template <typename T>
struct Optim1dArrays {
    T *p[3], *m[3], *v[3];               // raw_means, values, raw_scaling; their exp_avg and exp_avg_sq
    const T *g_means, *g_values, *g_cov, *g_conic;
    T *o_means, *o_cov, *o_conic;
    T *sum[2], *norm[2], *last[2];       // STATS: [0] of raw_means, [1] of raw_scaling
};

template <typename T>
__device__ __forceinline__ void write_gaussian1d(int64_t i, T rm, T rs, bool tanh_map, T scale, T* __restrict__ o_means,
                                                 T* __restrict__ o_cov, T* __restrict__ o_conic) {
    o_means[i] = tanh_map ? tanh(rm) * scale : rm;
    const T s = exp(rs);
    o_cov[i] = s;
    o_conic[i] = T(1) / s;
}

template <typename T>
__global__ __launch_bounds__(256) void optim1d_materialize_kernel(int64_t N, bool tanh_map, T scale,
                                                                  const T* __restrict__ raw_means,
                                                                  const T* __restrict__ raw_scaling, T* __restrict__ o_means,
                                                                  T* __restrict__ o_cov, T* __restrict__ o_conic) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    write_gaussian1d<T>(i, raw_means[i], raw_scaling[i], tanh_map, scale, o_means, o_cov, o_conic);
}

template <typename T, bool STATS>
__global__ __launch_bounds__(256) void optim1d_step_kernel(int64_t N, AdamBlock k, Optim1dArrays<T> a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    T rm = a.p[0][i], rs = a.p[2][i];

    if (a.g_means) {                                            // group 0: raw_means
        const AdamGroup<T> adam(k, 0);
        T g = a.g_means[i];
        if (k.tanh_map) g *= T(k.scale) * sech2(rm);
        if constexpr (STATS) {
            const T acc = a.sum[0][i] + g;
            a.sum[0][i] = acc;
            a.norm[0][i] += fabs(acc);
            a.last[0][i] = g;
        }
        T m = a.m[0][i], v = a.v[0][i];
        rm = adam_update_fma(adam, rm, g, m, v);
        if (k.wrap) {
            const T lo = T(k.lo), hi = T(k.hi), period = T(k.hi - k.lo);
            if (rm > hi) rm -= period;
            if (rm < lo) rm += period;
        }
        a.p[0][i] = rm;
        a.m[0][i] = m;
        a.v[0][i] = v;
    }

    if (a.g_values) {                                           // group 1: values pass through
        const AdamGroup<T> adam(k, 1);
        for (int j = 0; j < k.c; ++j) {
            const int64_t at = i * k.c + j;
            T m = a.m[1][at], v = a.v[1][at];
            a.p[1][at] = adam_update_fma(adam, a.p[1][at], a.g_values[at], m, v);
            a.m[1][at] = m;
            a.v[1][at] = v;
        }
    }

    if (a.g_cov || a.g_conic) {                                 // group 2: raw_scaling; cov = s, conic = 1 / s, ds/d raw = s
        const AdamGroup<T> adam(k, 2);
        const T s = exp(rs);
        const T gc = a.g_cov ? a.g_cov[i] : T(0), gq = a.g_conic ? a.g_conic[i] : T(0);
        const T g = fma(gc, s, -(gq / s));
        if constexpr (STATS) {
            const T acc = a.sum[1][i] + g;
            a.sum[1][i] = acc;
            a.norm[1][i] += fabs(acc);
            a.last[1][i] = g;
        }
        T m = a.m[2][i], v = a.v[2][i];
        rs = adam_update_fma(adam, rs, g, m, v);
        a.p[2][i] = rs;
        a.m[2][i] = m;
        a.v[2][i] = v;
    }

    write_gaussian1d<T>(i, rm, rs, k.tanh_map != 0, T(k.scale), a.o_means, a.o_cov, a.o_conic);
}

// capturable mode: one thread advances the running products and the step counts of the groups that have a gradient
__global__ void optim_advance_kernel(double* __restrict__ state, double beta1, double beta2, int present) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int g = 0; g < 4; ++g) {
        if (!(present >> g & 1)) continue;
        state[g] *= beta1;
        state[4 + g] *= beta2;
        state[8 + g] += 1.0;
    }
}

// the same, and the statistics' counts [2] (means, scaling) when there are any; mask_means / mask_scaling: their bits
__global__ void optim_advance_stats_kernel(double* __restrict__ state, double* __restrict__ counts, double beta1,
                                           double beta2, int present, int mask_means, int mask_scaling) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int g = 0; g < 4; ++g) {
        if (!(present >> g & 1)) continue;
        state[g] *= beta1;
        state[4 + g] *= beta2;
        state[8 + g] += 1.0;
    }
    if (counts) {
        if (present & mask_means) counts[0] += 1.0;
        if (present & mask_scaling) counts[1] += 1.0;
    }
}

template <typename T>
static int launch_materialize(int64_t N, bool tanh_map, double scale, const void* raw_means, const void* raw_scaling,
                              const void* transform, void* o_means, void* o_cov, void* o_conic, hipStream_t stream) {
    const int64_t blocks = (N + 255) / 256;
    if (blocks > 0x7fffffffLL) return PIGS_ERR_INVALID;
    clear_hip_error();
    hipLaunchKernelGGL(optim_materialize_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, stream, N, tanh_map, (T)scale,
                       (const T*)raw_means, (const T*)raw_scaling, (const T*)transform, (T*)o_means, (T*)o_cov, (T*)o_conic);
    return launch_status();
}

int optim_materialize(int dtype, int64_t N, bool tanh_map, double scale, const void* raw_means, const void* raw_scaling,
                      const void* transform, void* o_means, void* o_cov, void* o_conic, hipStream_t stream) {
    if (dtype == PIGS_F32)
        return launch_materialize<float>(N, tanh_map, scale, raw_means, raw_scaling, transform, o_means, o_cov, o_conic, stream);
    if (dtype == PIGS_F64)
        return launch_materialize<double>(N, tanh_map, scale, raw_means, raw_scaling, transform, o_means, o_cov, o_conic, stream);
    return PIGS_ERR_UNSUPPORTED;
}

static AdamBlock adam_block(const PigsAdamStep& h, int c) {
    AdamBlock k;
    for (int g = 0; g < 4; ++g) {
        k.lr[g] = h.lr[g];
        k.pow1[g] = h.beta1_pow[g];
        k.pow2[g] = h.beta2_pow[g];
    }
    k.beta1 = h.beta1; k.beta2 = h.beta2; k.eps = h.eps;
    k.scale = h.scale; k.lo = h.wrap_lo; k.hi = h.wrap_hi;
    k.dev_lr = h.device_lr;
    k.dev_state = h.device_state;
    k.tanh_map = h.means_map == PIGS_OPTIM_MEANS_TANH;
    k.wrap = h.wrap;
    k.c = c;
    return k;
}

template <typename T>
static int launch_step(const OptimStep& o, hipStream_t stream) {
    const int64_t blocks = (o.N + 255) / 256;
    if (blocks > 0x7fffffffLL) return PIGS_ERR_INVALID;
    const PigsAdamStep& h = *o.hyper;
    const AdamBlock k = adam_block(h, o.c);
    OptimArrays<T> a;
    for (int g = 0; g < 4; ++g) {
        a.p[g] = (T*)o.params[g];
        a.m[g] = (T*)o.exp_avg[g];
        a.v[g] = (T*)o.exp_avg_sq[g];
    }
    a.g_means = (const T*)o.grads[0]; a.g_values = (const T*)o.grads[1];
    a.g_cov = (const T*)o.grads[2]; a.g_conic = (const T*)o.grads[3];
    a.o_means = (T*)o.out[0]; a.o_cov = (T*)o.out[1]; a.o_conic = (T*)o.out[2];
    const int covs = (o.grads[2] || o.grads[3]) ? 12 : 0;
    const int present = (o.grads[0] ? 1 : 0) | (o.grads[1] ? 2 : 0) | covs;
    clear_hip_error();
    if (!o.stats) {
        if (h.device_state)
            hipLaunchKernelGGL(optim_advance_kernel, dim3(1), dim3(1), 0, stream, h.device_state, h.beta1, h.beta2, present);
        hipLaunchKernelGGL(optim_step_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, stream, o.N, k, a);
        return launch_status();
    }
    const PigsGradStats& gs = *o.stats;
    StatArrays<T> st;
    st.sum[0] = (T*)gs.mean_grad; st.sum[1] = (T*)gs.scale_grad;
    st.norm[0] = (T*)gs.mean_grad_norm; st.norm[1] = (T*)gs.scale_grad_norm;
    st.last[0] = (T*)gs.last_mean_grad; st.last[1] = (T*)gs.last_scale_grad;
    if (h.device_state)
        hipLaunchKernelGGL(optim_advance_stats_kernel, dim3(1), dim3(1), 0, stream, h.device_state, gs.device_counts,
                           h.beta1, h.beta2, present, 1, 4);
    hipLaunchKernelGGL(optim_step_stats_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, stream, o.N, k, a, st);
    return launch_status();
}

int optim_step(const OptimStep& o, hipStream_t stream) {
    if (o.dtype == PIGS_F32) return launch_step<float>(o, stream);
    if (o.dtype == PIGS_F64) return launch_step<double>(o, stream);
    return PIGS_ERR_UNSUPPORTED;
}

template <typename T>
static int launch_materialize1d(int64_t N, bool tanh_map, double scale, const void* raw_means, const void* raw_scaling,
                                void* o_means, void* o_cov, void* o_conic, hipStream_t stream) {
    const int64_t blocks = (N + 255) / 256;
    if (blocks > 0x7fffffffLL) return PIGS_ERR_INVALID;
    clear_hip_error();
    hipLaunchKernelGGL(optim1d_materialize_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, stream, N, tanh_map, (T)scale,
                       (const T*)raw_means, (const T*)raw_scaling, (T*)o_means, (T*)o_cov, (T*)o_conic);
    return launch_status();
}

int optim1d_materialize(int dtype, int64_t N, bool tanh_map, double scale, const void* raw_means, const void* raw_scaling,
                        void* o_means, void* o_cov, void* o_conic, hipStream_t stream) {
    if (dtype == PIGS_F32)
        return launch_materialize1d<float>(N, tanh_map, scale, raw_means, raw_scaling, o_means, o_cov, o_conic, stream);
    if (dtype == PIGS_F64)
        return launch_materialize1d<double>(N, tanh_map, scale, raw_means, raw_scaling, o_means, o_cov, o_conic, stream);
    return PIGS_ERR_UNSUPPORTED;
}

// o.params / exp_avg / exp_avg_sq [0..2]: raw_means, values, raw_scaling; slot 3 is not read
template <typename T>
static int launch_step1d(const OptimStep& o, hipStream_t stream) {
    const int64_t blocks = (o.N + 255) / 256;
    if (blocks > 0x7fffffffLL) return PIGS_ERR_INVALID;
    const PigsAdamStep& h = *o.hyper;
    const AdamBlock k = adam_block(h, o.c);
    Optim1dArrays<T> a{};
    for (int g = 0; g < 3; ++g) {
        a.p[g] = (T*)o.params[g];
        a.m[g] = (T*)o.exp_avg[g];
        a.v[g] = (T*)o.exp_avg_sq[g];
    }
    a.g_means = (const T*)o.grads[0]; a.g_values = (const T*)o.grads[1];
    a.g_cov = (const T*)o.grads[2]; a.g_conic = (const T*)o.grads[3];
    a.o_means = (T*)o.out[0]; a.o_cov = (T*)o.out[1]; a.o_conic = (T*)o.out[2];
    const int present = (o.grads[0] ? 1 : 0) | (o.grads[1] ? 2 : 0) | ((o.grads[2] || o.grads[3]) ? 4 : 0);
    clear_hip_error();
    if (!o.stats) {
        if (h.device_state)
            hipLaunchKernelGGL(optim_advance_kernel, dim3(1), dim3(1), 0, stream, h.device_state, h.beta1, h.beta2, present);
        hipLaunchKernelGGL((optim1d_step_kernel<T, false>), dim3((unsigned)blocks), dim3(256), 0, stream, o.N, k, a);
        return launch_status();
    }
    const PigsGradStats& gs = *o.stats;
    a.sum[0] = (T*)gs.mean_grad; a.sum[1] = (T*)gs.scale_grad;
    a.norm[0] = (T*)gs.mean_grad_norm; a.norm[1] = (T*)gs.scale_grad_norm;
    a.last[0] = (T*)gs.last_mean_grad; a.last[1] = (T*)gs.last_scale_grad;
    if (h.device_state)
        hipLaunchKernelGGL(optim_advance_stats_kernel, dim3(1), dim3(1), 0, stream, h.device_state, gs.device_counts,
                           h.beta1, h.beta2, present, 1, 4);
    hipLaunchKernelGGL((optim1d_step_kernel<T, true>), dim3((unsigned)blocks), dim3(256), 0, stream, o.N, k, a);
    return launch_status();
}

int optim1d_step(const OptimStep& o, hipStream_t stream) {
    if (o.dtype == PIGS_F32) return launch_step1d<float>(o, stream);
    if (o.dtype == PIGS_F64) return launch_step1d<double>(o, stream);
    return PIGS_ERR_UNSUPPORTED;
}

}  // namespace pigs
