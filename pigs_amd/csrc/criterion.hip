// The split criteria: which Gaussians to refine, as a byte mask on the device, without a host wait.
//
// Replaces the reference's chains of element-wise kernels, reductions and a full sort
//   quantile rule   model_pn.py:733-754   w = 1 - (D - min D) / max D,  m = (u - u_prev)^2 * w,
//                                         mask = any_k(m > quantile(m, q)) & boundary_mask
//   mean/std rule   test_no_mlp.py:203-205  mask = score > mean + k * std (unbiased)  & keep
//
// The quantile is torch.quantile's linear rule: with L = n * c, pos = q (L - 1), lo = floor(pos), hi = min(lo + 1, L - 1),
// quantile = x[lo] + (x[hi] - x[lo]) (pos - lo) in double, rounded once.  x[lo] and x[hi] are SELECTED elements, found
// by a most-significant-digit-first radix select (8-bit digits: 4 levels for float32, 8 for float64) over the
// order-preserving unsigned image of the float bits.  Both ranks are followed in the same levels: as long as rank hi
// falls into the bin of rank lo they share a prefix; where it does not, hi is the smallest element of the next
// non-empty bin and is followed from there with a second histogram (rank 0 of its own prefix).  That is the rule
// "x[hi] = x[lo] when more than lo + 1 values are <= x[lo], else the smallest value above it" without a pass of its own.
// NaN has a flag of its own: any NaN metric makes quantile, x_lo and x_hi NaN and the mask all false.
//
// One-workgroup variant (L <= CRITERION_LDS_VALUES): ONE launch of ONE workgroup, the keys live in LDS.
// Many-workgroup variant (L <= 2^24), launches:  float32 6,  float64 10
//   1   criterion_minmax_kernel     min / max partials of D per workgroup; workgroup 0 zeroes the histograms and the flag
//   1   criterion_metric_kernel     every workgroup reduces the partials, writes its keys (and the metric), level 0's
//                                   histogram (LDS, then integer atomics on the 256 global bins)
//   3/7 criterion_level_kernel      one per remaining level: every workgroup re-derives the prefixes from the earlier
//                                   levels' histograms and counts the next digit of the keys that match
//   1   criterion_finish_kernel     every workgroup re-derives x[lo], x[hi] and the quantile; workgroup 0 writes the
//                                   stats; all write the mask
// Mean/std: one launch of one workgroup for n <= CRITERION_LDS_VALUES, else three (partial sums; partial squared
// deviations; a one-workgroup finish that writes the mask), sums in double in a fixed order.
//
// No host wait, no allocation, no workgroup waits for another, no float atomics: the only cross-workgroup
// accumulation is per-workgroup partials and integer adds on histogram bins, so every result is a pure function of
// the inputs, and the two variants agree bit for bit.
#include <hip/hip_runtime.h>

#include "launch.h"

// the metric is what the tests compare with a composition of single IEEE operations: no fused multiply-add here
#pragma clang fp contract(off)

namespace pigs {

constexpr int CRIT_BLOCK = 1024;                  // threads of every kernel in this file
constexpr int CRIT_WAVES = CRIT_BLOCK / 64;
constexpr int CRIT_MAX_GRID = 256;                // workgroups of the many-workgroup kernels (grid-stride loops)
constexpr int CRIT_BINS = 256;                    // 8-bit digits

template <typename T> struct KeyOf;
template <> struct KeyOf<float> { using type = uint32_t; };
template <> struct KeyOf<double> { using type = uint64_t; };

// order-preserving image of the float bits: negative values flip entirely, the others get the sign bit set
template <typename T>
__device__ __forceinline__ typename KeyOf<T>::type to_key(T v) {
    using K = typename KeyOf<T>::type;
    constexpr K sign = K(1) << (8 * sizeof(K) - 1);
    K u;
    __builtin_memcpy(&u, &v, sizeof(K));
    return (u & sign) ? ~u : (u | sign);
}
template <typename T>
__device__ __forceinline__ T from_key(typename KeyOf<T>::type k) {
    using K = typename KeyOf<T>::type;
    constexpr K sign = K(1) << (8 * sizeof(K) - 1);
    const K u = (k & sign) ? (k ^ sign) : ~k;
    T v;
    __builtin_memcpy(&v, &u, sizeof(K));
    return v;
}

// ---- reductions inside a workgroup, in a fixed order ------------------------------------------------------------
__device__ __forceinline__ double block_sum(double v, double* scratch /* [CRIT_WAVES + 1] LDS */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();                                   // scratch may still be read from the call before
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < CRIT_WAVES; ++w) s += scratch[w];
        scratch[CRIT_WAVES] = s;
    }
    __syncthreads();
    return scratch[CRIT_WAVES];
}

// min and max over the workgroup; a NaN anywhere makes both NaN (torch's min / max propagate it)
template <typename T>
__device__ __forceinline__ void block_minmax(T& mn, T& mx, bool nan, T* scratch /* [2 * CRIT_WAVES] LDS */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T a = __shfl_down(mn, o), b = __shfl_down(mx, o);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    const int any_nan = __syncthreads_or(nan ? 1 : 0);
    if ((threadIdx.x & 63) == 0) { scratch[threadIdx.x >> 6] = mn; scratch[CRIT_WAVES + (threadIdx.x >> 6)] = mx; }
    __syncthreads();
    mn = scratch[0]; mx = scratch[CRIT_WAVES];
    for (int w = 1; w < CRIT_WAVES; ++w) {
        const T a = scratch[w], b = scratch[CRIT_WAVES + w];
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if (any_nan) mn = mx = __builtin_nan("");
    __syncthreads();
}

// ---- the select -------------------------------------------------------------------------------------------------
template <typename K>
struct Select {
    K pref_lo, pref_hi;        // the digits decided so far, as an integer
    uint32_t rank_lo;          // rank of x[lo] among the keys that share pref_lo
    int diverged;              // pref_hi is a prefix of its own (then x[hi] is the smallest key under it)
};

// smallest non-empty bin >= from (256: none); h = this lane's four bins 4 * lane .. 4 * lane + 3; whole wave
__device__ __forceinline__ int next_bin(const uint32_t (&h)[4], int from) {
    int best = CRIT_BINS;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint64_t m = __ballot(h[j] != 0u);
        const int lane_min = from > j ? (from - j + 3) >> 2 : 0;
        m = lane_min >= 64 ? 0ull : m & (~0ull << lane_min);
        const int cand = m ? 4 * (int)__builtin_ctzll(m) + j : CRIT_BINS;
        best = cand < best ? cand : best;
    }
    return best;
}

// One level: from the histogram of the next digit under pref_lo (h_lo) and under pref_hi (h_hi, read where the two
// have diverged) to the state one digit longer.  Wave 0 decides, the workgroup reads the outcome from `out` (LDS [4]).
template <typename K>
__device__ __forceinline__ void select_level(const uint32_t* h_lo, const uint32_t* h_hi, bool want_hi, Select<K>& s,
                                             uint32_t* out) {
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        uint32_t h[4], inc = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { h[j] = h_lo[4 * lane + j]; inc += h[j]; }
        const uint32_t own = inc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)inc, o);
            if (lane >= o) inc += t;
        }
        uint32_t before = inc - own;                         // keys in the bins in front of this lane's four
        const bool mine = before <= s.rank_lo && s.rank_lo < inc;
        int digit = 0;
        uint32_t rank = 0, upto = 0;
        if (mine) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (before <= s.rank_lo && s.rank_lo < before + h[j]) { digit = 4 * lane + j; rank = s.rank_lo - before; upto = before + h[j]; }
                before += h[j];
            }
        }
        const uint64_t who = __ballot(mine);
        const int src = who ? (int)__builtin_ctzll(who) : 0;
        digit = __shfl(digit, src);
        rank = (uint32_t)__shfl((int)rank, src);
        upto = (uint32_t)__shfl((int)upto, src);
        int digit_hi = digit, diverged = s.diverged;
        if (want_hi) {
            if (diverged) {
                uint32_t g[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) g[j] = h_hi[4 * lane + j];
                digit_hi = next_bin(g, 0);
            } else if (s.rank_lo + 1 >= upto) {              // rank hi lies behind this bin: the next non-empty one
                digit_hi = next_bin(h, digit + 1);
                diverged = 1;
            }
            if (digit_hi >= CRIT_BINS) { digit_hi = digit; diverged = s.diverged; }      // unreachable: hi < L
        }
        if (lane == 0) { out[0] = (uint32_t)digit; out[1] = rank; out[2] = (uint32_t)digit_hi; out[3] = (uint32_t)diverged; }
    }
    __syncthreads();
    const K base_hi = s.diverged ? s.pref_hi : s.pref_lo;
    s.pref_hi = (base_hi << 8) | (K)out[2];
    s.pref_lo = (s.pref_lo << 8) | (K)out[0];
    s.rank_lo = out[1];
    s.diverged = (int)out[3];
    __syncthreads();                                         // `out` is written again at the next level
}

// count the digit of `level` of one key into the workgroup's two LDS histograms
template <typename K>
__device__ __forceinline__ void count_key(K key, int level, const Select<K>& s, bool want_hi, uint32_t* hist /* [2][256] LDS */) {
    constexpr int bits = 8 * sizeof(K);
    const int shift = bits - 8 * (level + 1);
    const K upper = level ? key >> (shift + 8) : K(0);
    const uint32_t digit = (uint32_t)(key >> shift) & 255u;
    if (upper == s.pref_lo) atomicAdd(&hist[digit], 1u);
    else if (want_hi && s.diverged && upper == s.pref_hi) atomicAdd(&hist[CRIT_BINS + digit], 1u);
}

template <typename T>
struct QuantileArgs {
    int c, want_hi;
    int64_t n, L;
    uint32_t lo;
    double t;
    const T *sample_u, *prev_sample_u, *density;
    const uint8_t* boundary;
    T *metric, *stats;
    uint8_t* mask;
};

template <typename T>
__device__ __forceinline__ T metric_of(const QuantileArgs<T>& a, int64_t idx, T mn, T mx) {
    const T w = T(1) - (a.density[idx / a.c] - mn) / mx;
    const T d = a.sample_u[idx] - a.prev_sample_u[idx];
    return (d * d) * w;
}

// the quantile from the two selected keys; stats = {quantile, x_lo, x_hi, nan flag}
template <typename T>
__device__ __forceinline__ T finish_quantile(const QuantileArgs<T>& a, const Select<typename KeyOf<T>::type>& s, bool nan,
                                             bool write) {
    T x_lo = from_key<T>(s.pref_lo);
    T x_hi = a.want_hi ? from_key<T>(s.diverged ? s.pref_hi : s.pref_lo) : x_lo;
    const double xl = (double)x_lo, xh = (double)x_hi;
    T quantile = (T)(xl + (xh - xl) * a.t);
    if (nan) quantile = x_lo = x_hi = (T)__builtin_nan("");
    if (write && a.stats) { a.stats[0] = quantile; a.stats[1] = x_lo; a.stats[2] = x_hi; a.stats[3] = nan ? T(1) : T(0); }
    return quantile;
}

template <typename T>
__device__ __forceinline__ void write_mask_row(const QuantileArgs<T>& a, int64_t i, const typename KeyOf<T>::type* keys,
                                               T quantile) {
    bool any = false;
    for (int k = 0; k < a.c; ++k) any = any || from_key<T>(keys[i * a.c + k]) > quantile;      // false against NaN
    a.mask[i] = (any && (!a.boundary || a.boundary[i] != 0)) ? 1 : 0;
}

// ---- quantile rule, one workgroup ---------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(CRIT_BLOCK) void criterion_quantile_one_kernel(QuantileArgs<T> a) {
    using K = typename KeyOf<T>::type;
    __shared__ K keys[CRITERION_LDS_VALUES];
    __shared__ uint32_t hist[2 * CRIT_BINS];
    __shared__ T red[2 * CRIT_WAVES];
    __shared__ uint32_t out[4];
    const int L = (int)a.L, n = (int)a.n;

    T mn = a.density[0], mx = mn;
    bool nan = false;
    for (int i = threadIdx.x; i < n; i += CRIT_BLOCK) {
        const T d = a.density[i];
        nan = nan || d != d;
        mn = d < mn ? d : mn;
        mx = d > mx ? d : mx;
    }
    block_minmax(mn, mx, nan, red);

    nan = false;
    for (int idx = threadIdx.x; idx < L; idx += CRIT_BLOCK) {
        const T m = metric_of(a, idx, mn, mx);
        nan = nan || m != m;
        keys[idx] = to_key<T>(m);
        if (a.metric) a.metric[idx] = m;
    }
    const bool any_nan = __syncthreads_or(nan ? 1 : 0) != 0;          // also the barrier behind the keys

    Select<K> s{K(0), K(0), a.lo, 0};
    for (int level = 0; level < (int)sizeof(K); ++level) {
        for (int b = threadIdx.x; b < 2 * CRIT_BINS; b += CRIT_BLOCK) hist[b] = 0u;
        __syncthreads();
        for (int idx = threadIdx.x; idx < L; idx += CRIT_BLOCK) count_key<K>(keys[idx], level, s, a.want_hi != 0, hist);
        __syncthreads();
        select_level<K>(hist, hist + CRIT_BINS, a.want_hi != 0, s, out);
    }
    const T quantile = finish_quantile<T>(a, s, any_nan, threadIdx.x == 0);
    for (int i = threadIdx.x; i < n; i += CRIT_BLOCK) write_mask_row<T>(a, i, keys, quantile);
}

// ---- quantile rule, many workgroups -------------------------------------------------------------------------------
// workspace: keys [L] | histograms [levels][2][256] uint32 | nan flag, padding (uint32 x 2) | partials [CRIT_MAX_GRID][2] T,
// nan partials [CRIT_MAX_GRID] uint32
template <typename T>
struct Workspace {
    using K = typename KeyOf<T>::type;
    K* keys;
    uint32_t* hist;
    uint32_t* nan_flag;
    T* partials;
    uint32_t* nan_partials;
    __host__ __device__ Workspace(void* base, int64_t L) {
        char* p = (char*)base;
        keys = (K*)p;
        p += (size_t)((L * (int64_t)sizeof(K) + 7) / 8 * 8);
        hist = (uint32_t*)p;
        p += sizeof(K) * 2 * CRIT_BINS * sizeof(uint32_t);
        nan_flag = (uint32_t*)p;
        p += 8;
        partials = (T*)p;
        p += CRIT_MAX_GRID * 2 * sizeof(T);
        nan_partials = (uint32_t*)p;
    }
    static size_t bytes(int64_t L) {
        return (size_t)((L * (int64_t)sizeof(K) + 7) / 8 * 8) + sizeof(K) * 2 * CRIT_BINS * sizeof(uint32_t) + 8 +
               CRIT_MAX_GRID * 2 * sizeof(T) + CRIT_MAX_GRID * sizeof(uint32_t);
    }
};

template <typename T>
__global__ __launch_bounds__(CRIT_BLOCK) void criterion_minmax_kernel(QuantileArgs<T> a, void* base) {
    __shared__ T red[2 * CRIT_WAVES];
    const Workspace<T> ws(base, a.L);
    if (blockIdx.x == 0) {
        for (int b = threadIdx.x; b < (int)sizeof(typename KeyOf<T>::type) * 2 * CRIT_BINS; b += CRIT_BLOCK) ws.hist[b] = 0u;
        if (threadIdx.x == 0) ws.nan_flag[0] = 0u;
    }
    T mn = a.density[0], mx = mn;
    bool nan = false;
    for (int64_t i = (int64_t)blockIdx.x * CRIT_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * CRIT_BLOCK) {
        const T d = a.density[i];
        nan = nan || d != d;
        mn = d < mn ? d : mn;
        mx = d > mx ? d : mx;
    }
    block_minmax(mn, mx, nan, red);
    if (threadIdx.x == 0) {
        ws.partials[2 * blockIdx.x] = mn;
        ws.partials[2 * blockIdx.x + 1] = mx;
        ws.nan_partials[blockIdx.x] = mn != mn ? 1u : 0u;
    }
}

// flush a workgroup's LDS histograms into the level's global bins: integer adds, order-free
__device__ __forceinline__ void flush_hist(const uint32_t* hist, uint32_t* global_level) {
    for (int b = threadIdx.x; b < 2 * CRIT_BINS; b += CRIT_BLOCK)
        if (hist[b]) atomicAdd(&global_level[b], hist[b]);
}

template <typename T>
__global__ __launch_bounds__(CRIT_BLOCK) void criterion_metric_kernel(QuantileArgs<T> a, void* base, int minmax_blocks) {
    using K = typename KeyOf<T>::type;
    __shared__ uint32_t hist[2 * CRIT_BINS];
    __shared__ T red[2 * CRIT_WAVES];
    const Workspace<T> ws(base, a.L);
    const int p = threadIdx.x < minmax_blocks ? threadIdx.x : 0;        // minmax_blocks <= CRIT_MAX_GRID <= CRIT_BLOCK
    T mn = ws.partials[2 * p], mx = ws.partials[2 * p + 1];
    block_minmax(mn, mx, ws.nan_partials[p] != 0u, red);
    for (int b = threadIdx.x; b < 2 * CRIT_BINS; b += CRIT_BLOCK) hist[b] = 0u;
    __syncthreads();
    const Select<K> s{K(0), K(0), a.lo, 0};
    bool nan = false;
    for (int64_t idx = (int64_t)blockIdx.x * CRIT_BLOCK + threadIdx.x; idx < a.L; idx += (int64_t)gridDim.x * CRIT_BLOCK) {
        const T m = metric_of(a, idx, mn, mx);
        nan = nan || m != m;
        const K key = to_key<T>(m);
        ws.keys[idx] = key;
        if (a.metric) a.metric[idx] = m;
        count_key<K>(key, 0, s, false, hist);
    }
    const int any_nan = __syncthreads_or(nan ? 1 : 0);
    if (any_nan && threadIdx.x == 0) atomicOr(ws.nan_flag, 1u);
    flush_hist(hist, ws.hist);
}

// the state after `levels` levels, from the global histograms; every workgroup computes the same
template <typename T>
__device__ __forceinline__ Select<typename KeyOf<T>::type> derive(const QuantileArgs<T>& a, const Workspace<T>& ws, int levels,
                                                                  uint32_t* out) {
    using K = typename KeyOf<T>::type;
    Select<K> s{K(0), K(0), a.lo, 0};
    for (int l = 0; l < levels; ++l)
        select_level<K>(ws.hist + (size_t)l * 2 * CRIT_BINS, ws.hist + (size_t)l * 2 * CRIT_BINS + CRIT_BINS, a.want_hi != 0, s, out);
    return s;
}

template <typename T>
__global__ __launch_bounds__(CRIT_BLOCK) void criterion_level_kernel(QuantileArgs<T> a, void* base, int level) {
    using K = typename KeyOf<T>::type;
    __shared__ uint32_t hist[2 * CRIT_BINS];
    __shared__ uint32_t out[4];
    const Workspace<T> ws(base, a.L);
    for (int b = threadIdx.x; b < 2 * CRIT_BINS; b += CRIT_BLOCK) hist[b] = 0u;
    const Select<K> s = derive<T>(a, ws, level, out);            // its barriers also stand behind the zeroes
    for (int64_t idx = (int64_t)blockIdx.x * CRIT_BLOCK + threadIdx.x; idx < a.L; idx += (int64_t)gridDim.x * CRIT_BLOCK)
        count_key<K>(ws.keys[idx], level, s, a.want_hi != 0, hist);
    __syncthreads();
    flush_hist(hist, ws.hist + (size_t)level * 2 * CRIT_BINS);
}

template <typename T>
__global__ __launch_bounds__(CRIT_BLOCK) void criterion_finish_kernel(QuantileArgs<T> a, void* base) {
    using K = typename KeyOf<T>::type;
    __shared__ uint32_t out[4];
    const Workspace<T> ws(base, a.L);
    const Select<K> s = derive<T>(a, ws, (int)sizeof(K), out);
    const T quantile = finish_quantile<T>(a, s, ws.nan_flag[0] != 0u, blockIdx.x == 0 && threadIdx.x == 0);
    for (int64_t i = (int64_t)blockIdx.x * CRIT_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * CRIT_BLOCK)
        write_mask_row<T>(a, i, ws.keys, quantile);
}

// ---- mean/std rule ------------------------------------------------------------------------------------------------
template <typename T>
struct MeanStdArgs {
    int64_t n;
    double k;
    const T* score;
    const uint8_t* keep;
    T* stats;
    uint8_t* mask;
};

// threshold = mean + k * std from the two sums; stats = {threshold, mean, std}; n = 1: 0 / 0 = NaN
template <typename T>
__device__ __forceinline__ T finish_threshold(const MeanStdArgs<T>& a, double mean, double squares, bool write) {
    const double sd = sqrt(squares / (double)(a.n - 1));
    const T threshold = (T)(mean + a.k * sd);
    if (write && a.stats) { a.stats[0] = threshold; a.stats[1] = (T)mean; a.stats[2] = (T)sd; }
    return threshold;
}

template <typename T>
__device__ __forceinline__ void write_threshold_mask(const MeanStdArgs<T>& a, T threshold) {
    for (int64_t i = threadIdx.x; i < a.n; i += CRIT_BLOCK)
        a.mask[i] = (a.score[i] > threshold && (!a.keep || a.keep[i] != 0)) ? 1 : 0;
}

template <typename T>
__global__ __launch_bounds__(CRIT_BLOCK) void criterion_meanstd_one_kernel(MeanStdArgs<T> a) {
    __shared__ double red[CRIT_WAVES + 1];
    double sum = 0.0;
    for (int64_t i = threadIdx.x; i < a.n; i += CRIT_BLOCK) sum += (double)a.score[i];
    const double mean = block_sum(sum, red) / (double)a.n;
    double sq = 0.0;
    for (int64_t i = threadIdx.x; i < a.n; i += CRIT_BLOCK) {
        const double d = (double)a.score[i] - mean;
        sq += d * d;
    }
    const double squares = block_sum(sq, red);
    write_threshold_mask<T>(a, finish_threshold<T>(a, mean, squares, threadIdx.x == 0));
}

// the sum of the first `blocks` partials, in index order inside the tree of block_sum
__device__ __forceinline__ double sum_partials(const double* partials, int blocks, double* red) {
    return block_sum((int)threadIdx.x < blocks ? partials[threadIdx.x] : 0.0, red);
}

// pass 0: partial sums of the scores; pass 1: partial sums of the squared deviations from the mean of pass 0
template <typename T>
__global__ __launch_bounds__(CRIT_BLOCK) void criterion_meanstd_partial_kernel(MeanStdArgs<T> a, double* partials, int pass) {
    __shared__ double red[CRIT_WAVES + 1];
    double mean = 0.0;
    if (pass == 1) mean = sum_partials(partials, (int)gridDim.x, red) / (double)a.n;
    double sum = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * CRIT_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * CRIT_BLOCK) {
        const double d = (double)a.score[i] - mean;
        sum += pass == 1 ? d * d : d;
    }
    sum = block_sum(sum, red);
    if (threadIdx.x == 0) partials[pass * CRIT_MAX_GRID + blockIdx.x] = sum;
}

template <typename T>
__global__ __launch_bounds__(CRIT_BLOCK) void criterion_meanstd_finish_kernel(MeanStdArgs<T> a, const double* partials, int blocks) {
    __shared__ double red[CRIT_WAVES + 1];
    const double mean = sum_partials(partials, blocks, red) / (double)a.n;
    const double squares = sum_partials(partials + CRIT_MAX_GRID, blocks, red);
    write_threshold_mask<T>(a, finish_threshold<T>(a, mean, squares, threadIdx.x == 0));
}

// ---- host ---------------------------------------------------------------------------------------------------------
static_assert(CRITERION_LDS_VALUES * sizeof(uint64_t) + 2 * CRIT_BINS * 4 + 2 * CRIT_WAVES * 8 + 16 <= 160 * 1024,
              "the float64 keys of the one-workgroup variant fit the LDS of a CU");
static_assert(CRIT_MAX_GRID <= CRIT_BLOCK, "one thread per partial");

size_t criterion_workspace_bytes(int dtype, int64_t n, int c) {
    if ((dtype != PIGS_F32 && dtype != PIGS_F64) || n <= 0 || c < 1 || n > CRITERION_MAX_VALUES / c) return 0;
    const size_t meanstd = 2 * CRIT_MAX_GRID * sizeof(double);
    const size_t quantile = dtype == PIGS_F32 ? Workspace<float>::bytes(n * c) : Workspace<double>::bytes(n * c);
    return quantile > meanstd ? quantile : meanstd;
}

static unsigned grid_for(int64_t items) {
    const int64_t g = (items + CRIT_BLOCK - 1) / CRIT_BLOCK;
    return (unsigned)(g < CRIT_MAX_GRID ? g : CRIT_MAX_GRID);
}

template <typename T>
static int launch_quantile(const CriterionQuantile& q, hipStream_t stream) {
    QuantileArgs<T> a;
    a.c = q.c; a.n = q.n; a.L = q.n * q.c;
    const double pos = q.q * (double)(a.L - 1);                  // torch.quantile's linear rule
    const double lo = floor(pos);
    a.lo = (uint32_t)lo;
    a.want_hi = (int64_t)a.lo + 1 <= a.L - 1;
    a.t = pos - lo;
    a.sample_u = (const T*)q.sample_u; a.prev_sample_u = (const T*)q.prev_sample_u; a.density = (const T*)q.density;
    a.boundary = q.boundary; a.metric = (T*)q.metric; a.stats = (T*)q.stats; a.mask = q.mask;
    clear_hip_error();
    if (q.one_workgroup) {
        hipLaunchKernelGGL(criterion_quantile_one_kernel<T>, dim3(1), dim3(CRIT_BLOCK), 0, stream, a);
        return launch_status();
    }
    const unsigned rows = grid_for(a.n), values = grid_for(a.L);
    hipLaunchKernelGGL(criterion_minmax_kernel<T>, dim3(rows), dim3(CRIT_BLOCK), 0, stream, a, q.workspace);
    hipLaunchKernelGGL(criterion_metric_kernel<T>, dim3(values), dim3(CRIT_BLOCK), 0, stream, a, q.workspace, (int)rows);
    for (int level = 1; level < (int)sizeof(typename KeyOf<T>::type); ++level)
        hipLaunchKernelGGL(criterion_level_kernel<T>, dim3(values), dim3(CRIT_BLOCK), 0, stream, a, q.workspace, level);
    hipLaunchKernelGGL(criterion_finish_kernel<T>, dim3(rows), dim3(CRIT_BLOCK), 0, stream, a, q.workspace);
    return launch_status();
}

int criterion_quantile(const CriterionQuantile& q, hipStream_t stream) {
    if (q.dtype == PIGS_F32) return launch_quantile<float>(q, stream);
    if (q.dtype == PIGS_F64) return launch_quantile<double>(q, stream);
    return PIGS_ERR_UNSUPPORTED;
}

template <typename T>
static int launch_meanstd(const CriterionMeanStd& m, hipStream_t stream) {
    MeanStdArgs<T> a;
    a.n = m.n; a.k = m.k; a.score = (const T*)m.score; a.keep = m.keep; a.stats = (T*)m.stats; a.mask = m.mask;
    clear_hip_error();
    if (m.one_workgroup) {
        hipLaunchKernelGGL(criterion_meanstd_one_kernel<T>, dim3(1), dim3(CRIT_BLOCK), 0, stream, a);
        return launch_status();
    }
    const unsigned blocks = grid_for(a.n);
    double* partials = (double*)m.workspace;
    hipLaunchKernelGGL(criterion_meanstd_partial_kernel<T>, dim3(blocks), dim3(CRIT_BLOCK), 0, stream, a, partials, 0);
    hipLaunchKernelGGL(criterion_meanstd_partial_kernel<T>, dim3(blocks), dim3(CRIT_BLOCK), 0, stream, a, partials, 1);
    hipLaunchKernelGGL(criterion_meanstd_finish_kernel<T>, dim3(1), dim3(CRIT_BLOCK), 0, stream, a, (const double*)partials, (int)blocks);
    return launch_status();
}

int criterion_meanstd(const CriterionMeanStd& m, hipStream_t stream) {
    if (m.dtype == PIGS_F32) return launch_meanstd<float>(m, stream);
    if (m.dtype == PIGS_F64) return launch_meanstd<double>(m, stream);
    return PIGS_ERR_UNSUPPORTED;
}

}  // namespace pigs
