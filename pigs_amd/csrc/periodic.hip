// Periodic domain (ABI 10): the images of every Gaussian on the torus [lo, lo + L)^2, and the fold of their
// gradients back onto the originals.
//
// The reference's Navier-Stokes problem lives on a periodic box: Model.forward wraps the means back into
// [-1, 1] after every update (model_pn.py:689-693) and test_torus.py puts a column of Gaussians
// right at the seam.  A periodic sampler sums, for every point, the 3 x 3 shifted copies of every Gaussian:
//   u(x) = sum_n sum_{k in {-1,0,1}^2} v_n exp(-1/2 (x - mu'_n - kL)^T C_n (x - mu'_n - kL)),
//   mu'_n = lo + (mu_n - lo) - L floor((mu_n - lo) / L)          (d mu' / d mu = 1).
// In floating point mu'_n lies in the closed box [lo, lo + L]: a mean just below lo lands on lo + L, and a remainder
// that comes out negative ((mu - lo) / L underflowing to -0) gets one period.
// Nothing downstream changes: the images are an ordinary set of 9N Gaussians that preprocess() binds in place of
// the caller's N, and every sampling path (dense, binned, residual, captures) runs on them unchanged.
//
//   periodic_images_kernel  means / conics / values [N] -> image arrays [9N].  Image j of Gaussian n is row
//                           j*N + n: block 0 holds the wrapped originals, blocks 1..8 the shifts in row-major
//                           order of (ky, kx) with (0, 0) left out (image_shift below).  Every block keeps the
//                           caller's order, so a lattice of Gaussians stays a set of spatially coherent strips in
//                           every block (the binned build's strips, include/pigs_amd.h ABI 8).
//                           The same pass checks that the images suffice: every Gaussian's q <= q_cut ellipse
//                           must stay below one period on both axes (q_cut Sigma_ii < L^2, Sigma = C^-1) and its
//                           conic must be positive definite.  A wave with a failing Gaussian sets *flag with one
//                           atomic OR (ballot first); flag may be null.
//   periodic_fold_kernel    g[n] = sum_{j=0..8} g_img[j*N + n] for the means, conics and values gradients, in that
//                           fixed order and without atomics: deterministic, bitwise reproducible.
//
// Both are streams over rows: one thread per Gaussian; the nine rows it reads or writes lie N rows apart, so the
// lanes of a wave touch consecutive rows of one block at a time (coalesced).  Rows whose width allows (means: 2,
// values: c = 2 or 4) move as one vector when every pointer is aligned to it; the launcher checks.
#include <hip/hip_runtime.h>

#include "launch.h"

namespace pigs {

// (kx, ky) of image j: j = 0 -> (0, 0); j = 1..8 -> the other eight cells of the 3 x 3 block, row-major in
// (ky, kx) from (-1, -1): (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1).  include/pigs_amd.h repeats it.
__device__ __forceinline__ void image_shift(int j, int& kx, int& ky) {
    const int t = j == 0 ? 4 : (j <= 4 ? j - 1 : j);
    kx = t % 3 - 1;
    ky = t / 3 - 1;
}

template <typename T, int W, bool VEC>
__device__ __forceinline__ void load_row(const T* __restrict__ p, T (&r)[W]) {
    if constexpr (VEC && (W == 2 || W == 4)) {
        typedef T V __attribute__((ext_vector_type(W)));
        const V v = *reinterpret_cast<const V*>(p);
#pragma unroll
        for (int k = 0; k < W; ++k) r[k] = v[k];
    } else {
#pragma unroll
        for (int k = 0; k < W; ++k) r[k] = p[k];
    }
}

template <typename T, int W, bool VEC>
__device__ __forceinline__ void store_row(T* __restrict__ p, const T (&r)[W]) {
    if constexpr (VEC && (W == 2 || W == 4)) {
        typedef T V __attribute__((ext_vector_type(W)));
        V v;
#pragma unroll
        for (int k = 0; k < W; ++k) v[k] = r[k];
        *reinterpret_cast<V*>(p) = v;
    } else {
#pragma unroll
        for (int k = 0; k < W; ++k) p[k] = r[k];
    }
}

template <typename T, int C, bool VEC>
__global__ __launch_bounds__(256) void periodic_images_kernel(int64_t N, T lo, T period, T q_cut,
                                                              const T* __restrict__ means, const T* __restrict__ conics,
                                                              const T* __restrict__ values, T* __restrict__ img_means,
                                                              T* __restrict__ img_conics, T* __restrict__ img_values,
                                                              uint32_t* __restrict__ flag) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool fail = false;
    if (n < N) {
        T m[2], q[3], v[C];
        load_row<T, 2, VEC>(means + 2 * n, m);
        q[0] = conics[3 * n];
        q[1] = conics[3 * n + 1];
        q[2] = conics[3 * n + 2];
        load_row<T, C, VEC>(values + (int64_t)C * n, v);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const T r = m[a] - lo;
            T w = r - period * floor(r / period);
            // r / period of a mean a few denormals below lo underflows to -0 (lo = 0, L > 1): w = r < 0 and the
            // mean stayed outside the closed box.  One period more puts it on hi, where the rounding puts every
            // other mean just below lo.
            if (w < T(0)) w += period;
            m[a] = lo + w;
        }
        // the images suffice when the cut-off ellipse spans less than one period on each axis:
        // q_cut Sigma_xx = q_cut C_yy / det < L^2 (and likewise for y); the negated form fails on NaN too
        const T det = q[0] * q[2] - q[1] * q[1];
        const T lim = period * period * det;
        fail = !(q[0] > T(0) && q[2] > T(0) && det > T(0) && q_cut * q[2] < lim && q_cut * q[0] < lim &&
                 isfinite(m[0]) && isfinite(m[1]));
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            int kx, ky;
            image_shift(j, kx, ky);
            const int64_t row = (int64_t)j * N + n;
            const T mj[2] = {m[0] + T(kx) * period, m[1] + T(ky) * period};
            store_row<T, 2, VEC>(img_means + 2 * row, mj);
            img_conics[3 * row] = q[0];
            img_conics[3 * row + 1] = q[1];
            img_conics[3 * row + 2] = q[2];
            store_row<T, C, VEC>(img_values + (int64_t)C * row, v);
        }
    }
    // at most one atomic per wave: the first lane of a wave that holds a failing Gaussian reports for all of it
    const unsigned long long bad = __ballot(fail);
    if (flag && bad != 0ull && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)bad) - 1)) atomicOr(flag, 1u);
}

// acc = sum_{j=0..8} g[j*N + n] in that order; all nine loads are issued before the first add (summing as each row
// arrives made hipcc wait for every load in turn: 27 memory round trips per thread)
template <typename T, int W, bool VEC>
__device__ __forceinline__ void fold_rows(const T* __restrict__ g, int64_t N, int64_t n, T (&acc)[W]) {
    T r[9][W];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        if constexpr (W == 3) {
            const T* p = g + 3 * ((int64_t)j * N + n);
            r[j][0] = p[0];
            r[j][1] = p[1];
            r[j][2] = p[2];
        } else {
            load_row<T, W, VEC>(g + (int64_t)W * ((int64_t)j * N + n), r[j]);
        }
    }
#pragma unroll
    for (int k = 0; k < W; ++k) acc[k] = r[0][k];
#pragma unroll
    for (int j = 1; j < 9; ++j)
#pragma unroll
        for (int k = 0; k < W; ++k) acc[k] += r[j][k];
}

// g[n] = sum over the nine images, j = 0..8 in order; a null incoming array reads as zero
template <typename T, int C, bool VEC>
__global__ __launch_bounds__(256) void periodic_fold_kernel(int64_t N, const T* __restrict__ g_img_means,
                                                            const T* __restrict__ g_img_conics,
                                                            const T* __restrict__ g_img_values, T* __restrict__ g_means,
                                                            T* __restrict__ g_conics, T* __restrict__ g_values) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    T gm[2] = {T(0), T(0)}, gq[3] = {T(0), T(0), T(0)}, gv[C];
#pragma unroll
    for (int k = 0; k < C; ++k) gv[k] = T(0);
    if (g_img_means) fold_rows<T, 2, VEC>(g_img_means, N, n, gm);
    if (g_img_conics) fold_rows<T, 3, VEC>(g_img_conics, N, n, gq);
    if (g_img_values) fold_rows<T, C, VEC>(g_img_values, N, n, gv);
    store_row<T, 2, VEC>(g_means + 2 * n, gm);
    g_conics[3 * n] = gq[0];
    g_conics[3 * n + 1] = gq[1];
    g_conics[3 * n + 2] = gq[2];
    store_row<T, C, VEC>(g_values + (int64_t)C * n, gv);
}

// the vector path needs every means row pointer on a 2-element boundary and, for c = 2 / 4, every values row
// pointer on a c-element one (a view of a flat gradient buffer may start anywhere)
template <typename T>
static bool rows_aligned(int c, const void* const* means_like, int nm, const void* const* values_like, int nv) {
    for (int i = 0; i < nm; ++i)
        if (means_like[i] && (uintptr_t)means_like[i] % (2 * sizeof(T)) != 0) return false;
    if (c == 2 || c == 4)
        for (int i = 0; i < nv; ++i)
            if (values_like[i] && (uintptr_t)values_like[i] % (c * sizeof(T)) != 0) return false;
    return true;
}

template <typename T, int C, bool VEC>
static void launch_periodic_c(bool fold, unsigned blocks, int64_t N, double lo, double period, double q_cut,
                              const void* a0, const void* a1, const void* a2, void* o0, void* o1, void* o2,
                              uint32_t* flag, hipStream_t stream) {
    if (!fold)
        hipLaunchKernelGGL((periodic_images_kernel<T, C, VEC>), dim3(blocks), dim3(256), 0, stream, N, (T)lo, (T)period,
                           (T)q_cut, (const T*)a0, (const T*)a1, (const T*)a2, (T*)o0, (T*)o1, (T*)o2, flag);
    else
        hipLaunchKernelGGL((periodic_fold_kernel<T, C, VEC>), dim3(blocks), dim3(256), 0, stream, N, (const T*)a0,
                           (const T*)a1, (const T*)a2, (T*)o0, (T*)o1, (T*)o2);
}

template <typename T, bool VEC>
static void launch_periodic_v(bool fold, int c, unsigned blocks, int64_t N, double lo, double period, double q_cut,
                              const void* a0, const void* a1, const void* a2, void* o0, void* o1, void* o2,
                              uint32_t* flag, hipStream_t stream) {
    switch (c) {
        case 1: launch_periodic_c<T, 1, VEC>(fold, blocks, N, lo, period, q_cut, a0, a1, a2, o0, o1, o2, flag, stream); break;
        case 2: launch_periodic_c<T, 2, VEC>(fold, blocks, N, lo, period, q_cut, a0, a1, a2, o0, o1, o2, flag, stream); break;
        case 3: launch_periodic_c<T, 3, VEC>(fold, blocks, N, lo, period, q_cut, a0, a1, a2, o0, o1, o2, flag, stream); break;
        default: launch_periodic_c<T, 4, VEC>(fold, blocks, N, lo, period, q_cut, a0, a1, a2, o0, o1, o2, flag, stream); break;
    }
}

// images (fold = false): a = (means, conics, values), o = image arrays; fold: a = image gradients, o = gradients
template <typename T>
static int launch_periodic(bool fold, int c, int64_t N, double lo, double period, double q_cut, const void* a0,
                           const void* a1, const void* a2, void* o0, void* o1, void* o2, uint32_t* flag,
                           hipStream_t stream) {
    if (N == 0) return PIGS_OK;
    const int64_t blocks = (N + 255) / 256;
    if (blocks > 0x7fffffffLL || N > INT64_MAX / 36) return PIGS_ERR_INVALID;
    const void* ms[2] = {a0, o0};
    const void* vs[2] = {a2, o2};
    const bool vec = rows_aligned<T>(c, ms, 2, vs, 2);
    clear_hip_error();
    if (vec) launch_periodic_v<T, true>(fold, c, (unsigned)blocks, N, lo, period, q_cut, a0, a1, a2, o0, o1, o2, flag, stream);
    else launch_periodic_v<T, false>(fold, c, (unsigned)blocks, N, lo, period, q_cut, a0, a1, a2, o0, o1, o2, flag, stream);
    return launch_status();
}

int periodic_dispatch(bool fold, int dtype, int c, int64_t N, double lo, double period, double q_cut, const void* a0,
                      const void* a1, const void* a2, void* o0, void* o1, void* o2, uint32_t* flag, hipStream_t stream) {
    if (dtype == PIGS_F32) return launch_periodic<float>(fold, c, N, lo, period, q_cut, a0, a1, a2, o0, o1, o2, flag, stream);
    if (dtype == PIGS_F64) return launch_periodic<double>(fold, c, N, lo, period, q_cut, a0, a1, a2, o0, o1, o2, flag, stream);
    return PIGS_ERR_UNSUPPORTED;
}

}  // namespace pigs
