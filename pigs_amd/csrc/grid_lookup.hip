// pigs_grid_lookup (include/pigs_amd.h): the pixel of an image under every sample point, in one launch.
//
// The reference builds the data of its vorticity fits with three torch lines (main_pn.py:206-207, 210;
// test_initialize.py:132-133, 135):
//     coords = ((samples + 1.0) / 2.0 * res).to(torch.long).clamp(0, res - 1)
//     coords = coords[:, 1] * res + coords[:, 0]
//     torch.take(desired, coords)
// -- nine small launches.  Here: one thread per point, every operation rounded once in the samples' type and in the
// reference's order (a subtraction, a true division, a multiplication: nothing that could contract into an FMA), so that
// box = (-1, 1) on a square image reads the same pixels bit for bit.
#include "launch.h"
#include "dense_choice.h"      // GRID_X_MAX

namespace pigs {

// the pixel index of one coordinate on an axis of n pixels: clamp(trunc((x - lo) / span * n), 0, n - 1), compared as
// floating-point numbers so that no out-of-range conversion happens; a non-finite coordinate reads pixel 0
template <typename T>
__device__ __forceinline__ int64_t pixel_of(T x, T lo, T span, int64_t n) {
    if (!(x - x == T(0))) return 0;      // NaN, +-inf
    const T t = (x - lo) / span * (T)n;
    if (!(t >= T(1))) return 0;
    if (t >= (T)(n - 1)) return n - 1;
    return (int64_t)t;                   // truncation; 1 <= t < n - 1
}

template <typename TI, typename TS>
__global__ __launch_bounds__(256) void grid_lookup_kernel(int64_t H, int64_t W, int64_t M, TS lo, TS span,
                                                          const TI* __restrict__ image, const TS* __restrict__ samples,
                                                          TI* __restrict__ out) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const int64_t ix = pixel_of<TS>(samples[2 * m], lo, span, W);
    const int64_t iy = pixel_of<TS>(samples[2 * m + 1], lo, span, H);
    out[m] = image[iy * W + ix];
}

template <typename TI, typename TS>
static int launch_grid_lookup(int64_t H, int64_t W, int64_t M, double lo, double hi, const void* image, const void* samples,
                              void* out, hipStream_t stream) {
    clear_hip_error();
    const TS lo_t = (TS)lo, span = (TS)hi - lo_t;      // one rounding each, in the samples' type
    hipLaunchKernelGGL((grid_lookup_kernel<TI, TS>), dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream, H, W, M, lo_t, span,
                       (const TI*)image, (const TS*)samples, (TI*)out);
    return launch_status();
}

}  // namespace pigs

extern "C" int pigs_grid_lookup(int dtype_image, int dtype_samples, int64_t H, int64_t W, int64_t M, double lo, double hi,
                                const void* image, const void* samples, void* out, void* stream) {
    using namespace pigs;
    if ((dtype_image != PIGS_F32 && dtype_image != PIGS_F64) || (dtype_samples != PIGS_F32 && dtype_samples != PIGS_F64))
        return PIGS_ERR_UNSUPPORTED;
    if (H < 1 || W < 1 || M < 0 || !(hi > lo) || !(hi - lo <= 1.7976931348623157e308)) return PIGS_ERR_INVALID;
    if (H > (1LL << 24) || W > (1LL << 24)) return PIGS_ERR_UNSUPPORTED;      // a pixel count is exact in float32
    if ((M + 255) / 256 > GRID_X_MAX) return PIGS_ERR_UNSUPPORTED;
    if (M == 0) return PIGS_OK;
    if (!image || !samples || !out) return PIGS_ERR_INVALID;
    if (dtype_samples == PIGS_F32 && !((float)hi > (float)lo)) return PIGS_ERR_INVALID;      // the box is empty in float32
    hipStream_t s = (hipStream_t)stream;
    if (dtype_image == PIGS_F32)
        return dtype_samples == PIGS_F32 ? launch_grid_lookup<float, float>(H, W, M, lo, hi, image, samples, out, s)
                                         : launch_grid_lookup<float, double>(H, W, M, lo, hi, image, samples, out, s);
    return dtype_samples == PIGS_F32 ? launch_grid_lookup<double, float>(H, W, M, lo, hi, image, samples, out, s)
                                     : launch_grid_lookup<double, double>(H, W, M, lo, hi, image, samples, out, s);
}
