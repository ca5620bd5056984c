// Refinement: prune and split (or clone) Gaussians, the caller-side step in front of build_covariances.
//
// Replaces the reference's chain of boolean indexing, torch.linalg.eig, repeat_interleave and cat
//   mode "split"  model_pn.py:703-714 (prune) and :578-605 (Model.split)
//   mode "clone"  test_no_mlp.py:198-240 (densification)
// by one streaming pass over the N rows whose only host wait is the read of the two totals.
//
// Index (three launches, no workgroup waits for another):
//   refine_count_kernel   one workgroup per REFINE_ROWS rows: {kept, split} totals -> workspace[block]
//   refine_scan_kernel    ONE workgroup loops over the block totals, REFINE_SCAN_WIDTH per pass: exclusive scan in
//                         place, grand totals -> counts[2]
//   refine_rank_kernel    classifies again (two bytes per row), ranks inside the workgroup (ballot + mbcnt inside a
//                         wave, LDS across the waves), adds the block's offset: kept_pos[N], child_pos[N]
// Apply and backward: one thread per INPUT row through kept_pos / child_pos; every store of apply and every load of
// the backward is guarded by position < rows.  No atomics anywhere; the order is the input order.
//
// The split's displacement e = lambda_max * v (model_pn.py:587-589: the unit eigenvector times the eigenVALUE, not
// its root) from the covariance [[s0, tau], [tau, s1]], tau = tanh(t) sqrt(s0 s1), in closed form:
//   m = (s0 + s1) / 2, delta = (s0 - s1) / 2, r = sqrt(delta^2 + tau^2), lambda_max = m + r
//   v ~ (r + delta, tau) if delta >= 0 else (tau, r - delta)     -- the sum that does not cancel
//   sign: e_x > 0, or e_x = 0 and e_y > 0;  r = 0: v = (1, 0)
#include <hip/hip_runtime.h>

#include "cov_terms.h"
#include "launch.h"

// e, the children and the two-term gradient sums are what the tests compare bit for bit with compositions of single
// IEEE operations: no fused multiply-add in this file
#pragma clang fp contract(off)

namespace pigs {

static_assert(REFINE_ROWS == 1024 && REFINE_SCAN_WIDTH == 256, "the kernels' block sizes are these constants");
constexpr int REFINE_WAVES = REFINE_ROWS / 64;

__device__ __forceinline__ uint32_t lanes_before(uint64_t mask) {     // set bits of mask below this lane (v_mbcnt)
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

struct RefineClass {
    bool kept, split;
    uint32_t rank_kept, rank_split;      // kept / split rows of this workgroup in front of this one
};

// classify row i (keep / split null = all / none; pruned wins over split) and rank it inside the workgroup;
// `totals` (LDS, [REFINE_WAVES][2]) holds the waves' counts afterwards
__device__ __forceinline__ RefineClass refine_classify(int64_t N, const uint8_t* __restrict__ keep,
                                                       const uint8_t* __restrict__ split, uint32_t (*totals)[2]) {
    const int64_t i = (int64_t)blockIdx.x * REFINE_ROWS + threadIdx.x;
    const int wave = threadIdx.x >> 6;
    RefineClass c;
    c.kept = i < N && (!keep || keep[i] != 0);
    c.split = c.kept && split && split[i] != 0;
    const uint64_t mk = __ballot(c.kept), ms = __ballot(c.split);
    c.rank_kept = lanes_before(mk);
    c.rank_split = lanes_before(ms);
    if ((threadIdx.x & 63) == 0) {
        totals[wave][0] = (uint32_t)__builtin_popcountll(mk);
        totals[wave][1] = (uint32_t)__builtin_popcountll(ms);
    }
    __syncthreads();
    for (int w = 0; w < wave; ++w) {     // same address for the whole wave: a broadcast read
        c.rank_kept += totals[w][0];
        c.rank_split += totals[w][1];
    }
    return c;
}

__global__ __launch_bounds__(REFINE_ROWS) void refine_count_kernel(int64_t N, const uint8_t* __restrict__ keep,
                                                                   const uint8_t* __restrict__ split,
                                                                   int64_t* __restrict__ block_totals) {
    __shared__ uint32_t totals[REFINE_WAVES][2];
    const RefineClass c = refine_classify(N, keep, split, totals);
    if (threadIdx.x == REFINE_ROWS - 1) {          // the last thread's rank + itself = the workgroup's total
        block_totals[2 * (int64_t)blockIdx.x] = c.rank_kept + (c.kept ? 1u : 0u);
        block_totals[2 * (int64_t)blockIdx.x + 1] = c.rank_split + (c.split ? 1u : 0u);
    }
}

// one workgroup: block_totals[blocks][2] -> their exclusive prefix sums, in place; counts = the grand totals
__global__ __launch_bounds__(REFINE_SCAN_WIDTH) void refine_scan_kernel(int64_t blocks, int64_t* __restrict__ block_totals,
                                                                        int64_t* __restrict__ counts) {
    __shared__ uint32_t wave_sum[REFINE_SCAN_WIDTH / 64][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t carry[2] = {0, 0};
    for (int64_t base = 0; base < blocks; base += REFINE_SCAN_WIDTH) {
        const int64_t b = base + threadIdx.x;
        uint32_t v[2] = {0u, 0u}, inc[2];          // a pass sums at most REFINE_SCAN_WIDTH * REFINE_ROWS: 32 bits
        if (b < blocks) { v[0] = (uint32_t)block_totals[2 * b]; v[1] = (uint32_t)block_totals[2 * b + 1]; }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            inc[k] = v[k];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)inc[k], o);
                if (lane >= o) inc[k] += t;
            }
            if (lane == 63) wave_sum[wave][k] = inc[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            uint32_t before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < REFINE_SCAN_WIDTH / 64; ++w) {
                if (w < wave) before += wave_sum[w][k];
                all += wave_sum[w][k];
            }
            if (b < blocks) block_totals[2 * b + k] = carry[k] + before + (inc[k] - v[k]);
            carry[k] += all;
        }
        __syncthreads();                           // wave_sum is written again in the next pass
    }
    if (threadIdx.x == 0) { counts[0] = carry[0]; counts[1] = carry[1]; }
}

__global__ __launch_bounds__(REFINE_ROWS) void refine_rank_kernel(bool clone, int64_t N, const uint8_t* __restrict__ keep,
                                                                  const uint8_t* __restrict__ split,
                                                                  const int64_t* __restrict__ block_offsets,
                                                                  const int64_t* __restrict__ counts,
                                                                  int64_t* __restrict__ kept_pos,
                                                                  int64_t* __restrict__ child_pos) {
    __shared__ uint32_t totals[REFINE_WAVES][2];
    const RefineClass c = refine_classify(N, keep, split, totals);
    const int64_t i = (int64_t)blockIdx.x * REFINE_ROWS + threadIdx.x;
    if (i >= N) return;
    const int64_t k = block_offsets[2 * (int64_t)blockIdx.x] + c.rank_kept;
    const int64_t s = block_offsets[2 * (int64_t)blockIdx.x + 1] + c.rank_split;
    const int64_t n_kept = counts[0], n_split = counts[1];
    if (clone) {         // all kept rows, then one copy per parent
        kept_pos[i] = c.kept ? k : -1;
        child_pos[i] = c.split ? n_kept + s : -1;
    } else {             // the rows kept and not split (split is a subset of kept), then the pairs of children
        kept_pos[i] = c.kept && !c.split ? k - s : -1;
        child_pos[i] = c.split ? (n_kept - n_split) + 2 * s : -1;
    }
}

template <typename T>
struct alignas(2 * sizeof(T)) Pair {     // a means / scaling row: one 8-byte (float) or 16-byte (double) access
    T x, y;
};

// e = lambda_max * unit eigenvector of [[s0, tau], [tau, s1]] (the header of this file)
template <typename T>
__device__ __forceinline__ Pair<T> split_displacement(const T* __restrict__ scaling, const T* __restrict__ transform,
                                                      int64_t i) {
    const CovTerms<T> c(scaling, transform, i);
    const T tau = c.h * c.r;
    const T m = T(0.5) * (c.s0 + c.s1), delta = T(0.5) * (c.s0 - c.s1);
    const T r = sqrt(delta * delta + tau * tau);
    const T lambda = m + r;
    T vx = T(1), vy = T(0);
    if (r > T(0)) {
        if (delta >= T(0)) { vx = r + delta; vy = tau; }
        else { vx = tau; vy = r - delta; }
        const T n = sqrt(vx * vx + vy * vy);
        vx /= n;
        vy /= n;
        if (vx < T(0)) { vx = -vx; vy = -vy; }      // vx = 0 only with delta < 0, where vy = r - delta > 0
    }
    return {lambda * vx, lambda * vy};
}

template <typename T>
struct RefineArrays {
    const int64_t *kept_pos, *child_pos;
    const T *means, *scaling, *transforms, *values;              // apply: inputs;     backward: incoming gradients
    T *o_means, *o_scaling, *o_transforms, *o_values;            // apply: outputs;    backward: gradients
    int64_t* source;
    int32_t* child;
};

template <typename T>
__device__ __forceinline__ void refine_store_row(const RefineArrays<T>& a, int c, int64_t rows, int64_t pos, int64_t i,
                                                 int which, Pair<T> mean, Pair<T> scal, T tr, T scale) {
    if (pos >= rows) return;
    if (a.o_means) reinterpret_cast<Pair<T>*>(a.o_means)[pos] = mean;
    if (a.o_scaling) reinterpret_cast<Pair<T>*>(a.o_scaling)[pos] = scal;
    if (a.o_transforms) a.o_transforms[pos] = tr;
    if (a.o_values)
        for (int k = 0; k < c; ++k) a.o_values[pos * c + k] = scale * a.values[i * c + k];
    if (a.source) a.source[pos] = i;
    if (a.child) a.child[pos] = which;
}

template <typename T>
__global__ __launch_bounds__(256) void refine_apply_kernel(bool clone, int c, int64_t N, int64_t rows, T value_scale,
                                                           RefineArrays<T> a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int64_t kp = a.kept_pos[i], cp = a.child_pos[i];
    if (kp < 0 && cp < 0) return;
    Pair<T> mean = {T(0), T(0)}, scal = {T(0), T(0)};
    T tr = T(0);
    if (a.o_means) mean = reinterpret_cast<const Pair<T>*>(a.means)[i];
    if (a.o_scaling) scal = reinterpret_cast<const Pair<T>*>(a.scaling)[i];
    if (a.o_transforms) tr = a.transforms[i];
    if (kp >= 0) refine_store_row(a, c, rows, kp, i, -1, mean, scal, tr, T(1));
    if (cp < 0) return;
    if (clone) {
        refine_store_row(a, c, rows, cp, i, 0, mean, scal, tr, T(1));
        return;
    }
    Pair<T> e = {T(0), T(0)};
    if (a.o_means) e = split_displacement<T>(a.scaling, a.transforms, i);
    refine_store_row(a, c, rows, cp, i, 0, Pair<T>{mean.x - e.x, mean.y - e.y}, scal, tr, value_scale);
    refine_store_row(a, c, rows, cp + 1, i, 1, Pair<T>{mean.x + e.x, mean.y + e.y}, scal, tr, value_scale);
}

// gradient of input row i from its output rows: kept + (first child or copy) + (second child); e is a constant
// (model_pn.py:584-585 computes it under no_grad).  `width` values per row, `scale` on the children's share.
template <typename T>
__device__ __forceinline__ void refine_gather_row(const T* __restrict__ g_out, T* __restrict__ g_in, int width, int64_t rows,
                                                  int64_t i, int64_t kp, int64_t cp, bool second, T scale) {
    if (!g_in) return;
    for (int k = 0; k < width; ++k) {
        T g = T(0);
        if (g_out) {
            if (kp >= 0 && kp < rows) g = g_out[kp * width + k];
            if (cp >= 0 && cp < rows) g += scale * g_out[cp * width + k];
            if (second && cp >= 0 && cp + 1 < rows) g += scale * g_out[(cp + 1) * width + k];
        }
        g_in[i * width + k] = g;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void refine_backward_kernel(bool clone, int c, int64_t N, int64_t rows, T value_scale,
                                                              RefineArrays<T> a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int64_t kp = a.kept_pos[i], cp = a.child_pos[i];
    const bool second = !clone;
    refine_gather_row(a.means, a.o_means, 2, rows, i, kp, cp, second, T(1));
    refine_gather_row(a.scaling, a.o_scaling, 2, rows, i, kp, cp, second, T(1));
    refine_gather_row(a.transforms, a.o_transforms, 1, rows, i, kp, cp, second, T(1));
    refine_gather_row(a.values, a.o_values, c, rows, i, kp, cp, second, clone ? T(1) : value_scale);
}

size_t refine_workspace_bytes(int64_t N) {
    if (N <= 0 || N > REFINE_MAX_N) return 0;
    return (size_t)((N + REFINE_ROWS - 1) / REFINE_ROWS) * 2 * sizeof(int64_t);
}

int refine_index(int mode, int64_t N, const uint8_t* keep, const uint8_t* split, void* workspace, int64_t* kept_pos,
                 int64_t* child_pos, int64_t* counts, hipStream_t stream) {
    const int64_t blocks = (N + REFINE_ROWS - 1) / REFINE_ROWS;      // <= 2^21: N <= REFINE_MAX_N
    int64_t* totals = (int64_t*)workspace;
    clear_hip_error();
    hipLaunchKernelGGL(refine_count_kernel, dim3((unsigned)blocks), dim3(REFINE_ROWS), 0, stream, N, keep, split, totals);
    hipLaunchKernelGGL(refine_scan_kernel, dim3(1), dim3(REFINE_SCAN_WIDTH), 0, stream, blocks, totals, counts);
    hipLaunchKernelGGL(refine_rank_kernel, dim3((unsigned)blocks), dim3(REFINE_ROWS), 0, stream, mode == PIGS_REFINE_CLONE, N,
                       keep, split, totals, counts, kept_pos, child_pos);
    return launch_status();
}

template <typename T>
static int launch_rows(bool backward, const RefineRows& r, hipStream_t stream) {
    RefineArrays<T> a;
    a.kept_pos = r.kept_pos; a.child_pos = r.child_pos;
    a.means = (const T*)r.in[0]; a.scaling = (const T*)r.in[1]; a.transforms = (const T*)r.in[2]; a.values = (const T*)r.in[3];
    a.o_means = (T*)r.out[0]; a.o_scaling = (T*)r.out[1]; a.o_transforms = (T*)r.out[2]; a.o_values = (T*)r.out[3];
    a.source = r.source; a.child = r.child;
    const int64_t blocks = (r.N + 255) / 256;                         // <= 2^23
    const bool clone = r.mode == PIGS_REFINE_CLONE;
    clear_hip_error();
    if (!backward)
        hipLaunchKernelGGL(refine_apply_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, stream, clone, r.c, r.N, r.rows,
                           (T)r.value_scale, a);
    else
        hipLaunchKernelGGL(refine_backward_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, stream, clone, r.c, r.N, r.rows,
                           (T)r.value_scale, a);
    return launch_status();
}

int refine_rows(bool backward, const RefineRows& r, hipStream_t stream) {
    if (r.dtype == PIGS_F32) return launch_rows<float>(backward, r, stream);
    if (r.dtype == PIGS_F64) return launch_rows<double>(backward, r, stream);
    return PIGS_ERR_UNSUPPORTED;
}

}  // namespace pigs
