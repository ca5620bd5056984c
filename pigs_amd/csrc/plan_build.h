// Binned sampler, preprocess: the samples build and the Gaussians' half of a plan build.  Included by plan.hip alone.
//
// Samples build = 4 launches (bbox partials -> cell key + rank -> scan -> scatter); plan build =
// the same chain for the Gaussians (sharing the launches of a samples build that runs with it) +
// the list launch (plan_lists.h).  No memset, no host synchronisation, static memory.
// Here too: grid_barrier (the samples' fall-back sort inside the count launch) and the mapping of workgroups
// to XCDs that the list launch and the sampling kernels share (build-time knob PIGS_XCD_CHUNK).
#pragma once
#include "pair_math.h"
#include "plan.h"
#include "grid_walk.h"
#include <type_traits>

namespace pigs {

// ------------------------------------------------------------------------------------------
// preprocess kernels
// ------------------------------------------------------------------------------------------
struct BuildArgs {
    // samples side
    SampleParams* sparams;
    float4* sboxes;       // [PLAN_BBOX_BLOCKS] per-workgroup partial boxes {min x, min y, max x, max y}
    float4* slat;         // [PLAN_BBOX_BLOCKS] per-workgroup largest neighbour steps {along x, along y, across x, across y} (index-tiled order)
    int no_lattice;       // PIGS_LATTICE=0: never index-tiled (tests, A/B)
    uint32_t rf_hint;     // the row length the last completed build of a point set of this size found (0: none): the first
                          // launch loads its tiles for that length while it is still verifying it
    uint32_t* scounts;    // [s_scan_blocks * PLAN_SCAN_BLOCK] fine-cell counters, followed by the scan aggregates
    unsigned long long* sagg;
    uint32_t* sstarts;
    uint2* skey;          // per point {cell id, rank inside the cell}
    SPoint* spts;
    const float* samples;
    uint32_t M, scells_cap, s_scan_blocks, s_zero_words;
    uint32_t s_blocks;    // blocks of 1 024 points of the one-pass count (its sample workgroups: one per block, or fewer, striding)
    uint32_t* szero;      // what the bbox launch zeroes for the samples side (s_zero_words): counters + scan aggregates
    // coarse-bin path of the samples build (plan.h): scounts / sagg / sstarts then are the (bin, workgroup) count
    // matrix, its scan aggregates and its scan
    int coarse;
    uint32_t cells_per_bin, h_chunk, h_wgs;
    STmp* tmp;
    // plan side
    PlanParams* params;
    uint32_t* counts;     // [scan_blocks * PLAN_SCAN_BLOCK] Gaussian cell counters, followed by the scan aggregates
    unsigned long long* agg;   // [scan_blocks] {1 << 32 | workgroup total}, zero before the scan
    uint32_t* starts;     // [gcells + 1] exclusive scan of counts
    uint2* gkey;          // per Gaussian {cell key, rank inside the cell}
    float4* rec;
    float4* gbox;
    float* gacc;
    uint32_t* g2o;
    const float* means;
    const float* conics;
    const float* values;
    uint32_t N;
    int c, G0, L;
    uint32_t scan_blocks, zero_words;
    uint32_t level_off[PLAN_MAX_LEVELS + 1];
    float q_max;          // the WIDE cut-off max(q_f, q_b): levels and candidate boxes are sized for it
    float q_f, q_b;
    // which halves this build covers
    int do_samples, do_plan;
    int no_lookback;      // test hook: the scan's workgroups never publish; every look-back recomputes
    int zero_gacc;        // the backward's scratch is not known to be zero (a workspace that is not PIGS_BUILD_PLAN_WS_CLEAN)
    uint32_t bbox_blocks; // workgroups of the first launch = partials in sboxes / slat: 256, or 512 from 2^19 points on
    // round 4, "the Gaussians one launch ahead" (run_build): with a lattice expected and the box of the last build of this
    // size known, the Gaussian chain does not wait for the first launch -- launch 1 = box of the samples || count of the
    // Gaussians on the REMEMBERED box (grid domains steer the quality of the binning, never the result), launch 2 = scan
    // of the Gaussian cells || the samples' lattice decision (and their count, should they be no lattice), launch 3 =
    // scatter of the Gaussians (|| scan + scatter of the samples by scan_pick, should they be no lattice): one launch
    // fewer in front of the tile lists.
    int ahead;
    float hint_box[4];
    int s_scan_in_scatter;  // launch 3 of the chain above: no scan launch ran for the samples
    int sort_in_count;      // ... or no launch 3 at all (ahead && strips: it would hold nothing but the samples' fall-back):
                            // points that are no lattice are counted, scanned AND scattered by the samples' workgroups
                            // of launch 2, behind two device-wide barriers among them (samples_sort_in_count)
    // STRIPS (plan.h, PlanParams::strips): the Gaussians keep the caller's order -- gauss_pack_part instead of count,
    // scan and scatter; `parea` is written by builds of either kind (the statistic the library decides from) whose
    // statistics are wanted home, null in every other build (plan.hip, run_build)
    int strips;
    int fwd_only;         // PIGS_BUILD_FORWARD_ONLY (PlanParams::fwd_only): q_max = q_f = q_b
    // TRUSTED build (plan.hip, run_build): point sets of this size have long been the same compact lattice, so nobody looks
    // at the points in front of the list launch -- the count launch holds the Gaussians' pack workgroups alone, on
    // `hint_box`, and its first workgroup writes the samples header the decision would have written (row length rf_hint,
    // fast axis hint_axis).  The list launch checks every tile against that box (plan_lists.h, the guard).
    int trusted;
    uint32_t hint_axis;
    float4* pbox;
    float4* sbox;
    float* parea;
};

__device__ __forceinline__ void zero_words(uint32_t* p, uint32_t words, uint32_t bid, uint32_t nb) {
    uint4* p4 = (uint4*)p;
    for (uint32_t i = bid * blockDim.x + threadIdx.x; i < words / 4; i += nb * blockDim.x) p4[i] = make_uint4(0, 0, 0, 0);
}
__device__ __forceinline__ void zero_words(uint32_t* p, uint32_t words) { zero_words(p, words, blockIdx.x, gridDim.x); }

// Bounding boxes with the DPP modifier fused into the min / max (hipcc emits v_mov_dpp + a
// canonicalising v_max + v_min per step from the builtin form: 4x the instructions).  The four
// reductions are independent chains and are interleaved step by step, so the two wait states a
// DPP read needs after the VALU write of its source are filled by the other three chains: one
// s_nop at the head instead of one per step (an s_nop costs an issue slot like a VALU
// instruction).  row_box_dpp leaves in every lane the box of the lane's own 16-lane row;
// wave_box_dpp continues from there to the box of the wave, broadcast from lane 63.
#define PIGS_BOX_STEP(MOD)                                \
    "v_min_f32_dpp %0, %0, %0 " MOD " bank_mask:0xf\n\t" \
    "v_max_f32_dpp %1, %1, %1 " MOD " bank_mask:0xf\n\t" \
    "v_min_f32_dpp %2, %2, %2 " MOD " bank_mask:0xf\n\t" \
    "v_max_f32_dpp %3, %3, %3 " MOD " bank_mask:0xf\n\t"
__device__ __forceinline__ void row_box_dpp(float& x0, float& x1, float& y0, float& y1) {
    asm volatile("s_nop 1\n\t"
                 PIGS_BOX_STEP("quad_perm:[1,0,3,2] row_mask:0xf")
                 PIGS_BOX_STEP("quad_perm:[2,3,0,1] row_mask:0xf")
                 PIGS_BOX_STEP("row_half_mirror row_mask:0xf")
                 PIGS_BOX_STEP("row_mirror row_mask:0xf")
                 "s_nop 1"
                 : "+v"(x0), "+v"(x1), "+v"(y0), "+v"(y1));
}
__device__ __forceinline__ void wave_box_from_rows_dpp(float& x0, float& x1, float& y0, float& y1) {
    asm volatile("s_nop 1\n\t"
                 PIGS_BOX_STEP("row_bcast:15 row_mask:0xa")
                 PIGS_BOX_STEP("row_bcast:31 row_mask:0xc")
                 "s_nop 1"
                 : "+v"(x0), "+v"(x1), "+v"(y0), "+v"(y1));
    x0 = readlane_f(x0, 63); x1 = readlane_f(x1, 63); y0 = readlane_f(y0, 63); y1 = readlane_f(y1, 63);
}

// Launch 1 of a samples build (PLAN_BBOX_BLOCKS workgroups): zero the cell counters (of the
// plan too, when one is built alongside); per-workgroup bounding box of the sample points, written as a plain
// partial.  And what the INDEX-TILED order (plan.h, SampleParams::lat) is decided from, in the same streaming pass:
// every workgroup finds the first index at which the fast coordinate steps backwards -- the row length rf of a
// lattice in row order (a search of the first 2 049 points, of 16 385 when those hold none; all workgroups read the
// same few KB) -- and, for a row length whose rf and M / rf are multiples of 8, the largest steps between
// neighbours: along a row (point i against i - 1, row ends left out) and across rows (point i against i - rf),
// per coordinate.  An 8 x 8 index tile is at most 7 (along + across) wide and high: the next launch holds that
// against the bounding box and decides whether index tiles are compact -- then nothing is sorted and NOTHING IS
// COPIED: the sampling kernels read the caller's array through the index arithmetic -- or the points go through
// the sort.  The pass runs on the row length of the last build of this size (the library's memory, `rf_hint`)
// while the search is still in flight, and is repeated only when the search finds another one.
constexpr uint32_t LAT_SEARCH0 = 2048, LAT_SEARCH1 = 16384;
__device__ __forceinline__ bool lattice_shape_ok(uint32_t rf, uint32_t n) {
    const uint32_t rs = rf ? n / rf : 0u;
    return rf >= 8u && (rf & 7u) == 0u && rs * rf == n && (rs & 7u) == 0u && n >= 64u;
}
struct GaussLoad;
__device__ __forceinline__ void gauss_count_ahead(const BuildArgs& a, uint32_t bid);
__global__ __launch_bounds__(256) void samples_bbox_kernel(BuildArgs a) {
    __shared__ float sh[4][8];
    __shared__ uint32_t shk[4];
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    if (a.ahead && blockIdx.x >= a.bbox_blocks) {       // (block-uniform) the Gaussians one launch ahead, on the remembered box
        gauss_count_ahead(a, blockIdx.x - a.bbox_blocks);
        return;
    }
    const uint32_t nblocks = a.bbox_blocks;             // (the launch may hold the Gaussians' workgroups behind these)
    zero_words(a.szero, a.s_zero_words, blockIdx.x, nblocks);
    if (blockIdx.x == 0 && tid < 2) a.sparams->order_stat[tid] = 0u;
    if (blockIdx.x == 0 && tid < 2 * 17) a.sparams->bar[tid] = 0u;
    if (a.do_plan && !a.ahead) {        // (ahead: a clean workspace, and its counters are being counted in this very launch)
        zero_words(a.counts, a.zero_words, blockIdx.x, nblocks);
        if (a.zero_gacc) zero_words((uint32_t*)a.gacc, 8u * a.N, blockIdx.x, nblocks);
    }
    if (a.do_plan && blockIdx.x == 0 && tid < PLAN_BAR_WORDS) a.params->bar[tid] = 0u;
    const float INF = __builtin_huge_valf();
    float x0 = INF, y0 = INF, x1 = -INF, y1 = -INF;
    auto take = [&](float x, float y) {
        if (fabsf(x) < INF) { x0 = fminf(x0, x); x1 = fmaxf(x1, x); }
        if (fabsf(y) < INF) { y0 = fminf(y0, y); y1 = fmaxf(y1, y); }
    };
    const float2* pts = (const float2*)a.samples;
    const float4* pts2 = (const float4*)a.samples;
    const uint32_t n = a.M;
    const uint32_t npair = n / 2;                 // float4 = two points
    const uint32_t stride = nblocks * BBOX_THREADS;
    // the largest neighbour steps (NaN / inf coordinates: +inf, never compact)
    float ax = 0.f, ay = 0.f, bx = 0.f, by = 0.f;
    auto step = [&](float& s, float u, float v) {
        const float d = fabsf(u - v);
        s = d == d ? fmaxf(s, d) : INF;
    };
    // one streaming pass, 8 pairs (float4 = two points) per thread in flight: the box (first time only) and, with a
    // row length rf, the neighbour steps.  With a row length a thread takes the SAME column pair of 8 consecutive rows:
    // the point above is then its own previous load (one extra load for the first of its rows), the point to the right
    // its neighbour lane's (one lane of the wave loads it) -- 9 + 1 loads where point, right and upper neighbour of
    // every pair were 24 (first launch 8.6 -> 6.x us at 1024^2).
    auto pass = [&](auto pbc, uint32_t rf, bool box) {
        constexpr int PB = decltype(pbc)::value;
        ax = ay = bx = by = 0.f;
        if (rf == 0u) {
            for (uint32_t i = blockIdx.x * BBOX_THREADS + tid; i < npair; i += PB * stride) {
                float4 v[PB];
#pragma unroll
                for (int k = 0; k < PB; ++k) {
                    const uint32_t j = i + k * stride;
                    v[k] = pts2[j < npair ? j : i];
                }
#pragma unroll
                for (int k = 0; k < PB; ++k) {
                    if (i + k * stride >= npair) break;
                    if (box) { take(v[k].x, v[k].y); take(v[k].z, v[k].w); }
                }
            }
        } else {
            const uint32_t half = rf >> 1;            // pairs per row (rf is even: a float4 never straddles a row end)
            const uint32_t items = (n / rf / PB) * half;      // (column pair, block of 8 rows): rs is a multiple of 8
            for (uint32_t g = blockIdx.x * BBOX_THREADS + tid; g - (uint32_t)lane < items; g += stride) {      // whole waves stay in (the shuffles)
                const bool in = g < items;
                const uint32_t gg = in ? g : items - 1u;
                const uint32_t rb = gg / half, c = gg - rb * half;
                const uint32_t j0 = rb * PB * half + c;
                float4 v[PB];
#pragma unroll
                for (int k = 0; k < PB; ++k) v[k] = pts2[j0 + (uint32_t)k * half];
                const float4 up0 = pts2[rb ? j0 - half : j0];
                const bool last = c == half - 1u;                      // the pair at the end of a row: its right neighbour starts the next row
                const bool edge = lane == 63 && !last;                 // right neighbour in another wave: loaded
                float2 nxl[PB];
#pragma unroll
                for (int k = 0; k < PB; ++k) nxl[k] = edge ? pts[2u * (j0 + (uint32_t)k * half) + 2u] : make_float2(0.f, 0.f);
#pragma unroll
                for (int k = 0; k < PB; ++k) {
                    const float rx = __shfl_down(v[k].x, 1), ry = __shfl_down(v[k].y, 1);
                    if (!in) continue;
                    if (box) { take(v[k].x, v[k].y); take(v[k].z, v[k].w); }
                    step(ax, v[k].z, v[k].x); step(ay, v[k].w, v[k].y);
                    if (!last) { step(ax, edge ? nxl[k].x : rx, v[k].z); step(ay, edge ? nxl[k].y : ry, v[k].w); }
                    const float4 u = k ? v[k > 0 ? k - 1 : 0] : up0;
                    if (k || rb) {
                        step(bx, v[k].x, u.x); step(by, v[k].y, u.y);
                        step(bx, v[k].z, u.z); step(by, v[k].w, u.w);
                    }
                }
            }
        }
        if (box && (n & 1u) && blockIdx.x == 0 && tid == 0) take(pts[n - 1].x, pts[n - 1].y);
    };
    // ---- the candidate row length.  The fast axis is the one along which the first two points differ most, its
    // direction the sign of that step; a row ends where the fast coordinate steps the other way (a jittered lattice
    // keeps its rows as long as the jitter stays below half a step).  key = that first index (NONE: none found).
    // Thread t looks at the eight steps from point 8 t on; the loads are issued HERE and looked at behind the pass:
    // one memory round trip for the launch.
    constexpr uint32_t NONE = 0xffffffffu;
    // With a row length remembered (rf_hint) there is nothing to search for: the pass below runs on it, and a point set
    // whose rows are not that long fails it (the row ends it did not expect are neighbour steps as wide as the domain) --
    // it is sorted this once, the memory forgets the row length, the next build searches again.  (The search walks up to
    // 16 385 points in every workgroup: rows of 2 880 points -- a rank's shard of bench.py's grid for 8 GPUs -- made the
    // first launch 21 us instead of 8.)
    const bool hinted = !a.no_lattice && n >= 64u && lattice_shape_ok(a.rf_hint, n);
    const bool search = !a.no_lattice && n >= 64u && !hinted;
    float2 e0 = make_float2(0.f, 0.f), e1 = e0, q[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) q[k] = e0;
    if (search) {
        e0 = pts[0]; e1 = pts[1];
#pragma unroll
        for (int k = 0; k < 9; ++k)
            if (8u * tid + (uint32_t)k < n) q[k] = pts[8u * tid + (uint32_t)k];
    }
    // the pass on the remembered row length (or, without one, for the box alone)
    const uint32_t hf = hinted ? a.rf_hint : 0u;
    if (hinted) { e0 = pts[0]; e1 = pts[1]; }        // (the fast axis: from the first two points, as the search takes it)
    // (from 2^19 points on, and with no row length expected, the launch has twice the workgroups and a thread half the
    // rows: BuildArgs::bbox_blocks)
    const bool wide = nblocks > 256u;
    if (wide) pass(std::integral_constant<int, 4>{}, hf, true); else pass(std::integral_constant<int, 8>{}, hf, true);
    const uint32_t axis = fabsf(e1.y - e0.y) > fabsf(e1.x - e0.x) ? 1u : 0u;
    const float dir = (axis ? e1.y - e0.y : e1.x - e0.x) < 0.f ? -1.f : 1.f;
    auto backward = [&](float2 p, float2 r) { return (axis ? r.y - p.y : r.x - p.x) * dir < 0.f; };
    auto block_min = [&](uint32_t k) -> uint32_t {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) k = min(k, (uint32_t)__shfl_xor((int)k, o));
        __syncthreads();
        if (lane == 0) shk[wave] = k;
        __syncthreads();
        return min(min(shk[0], shk[1]), min(shk[2], shk[3]));
    };
    uint32_t key = NONE;
    if (search) {
#pragma unroll
        for (int k = 7; k >= 0; --k)
            if (8u * tid + (uint32_t)k + 1u < n && backward(q[k], q[k + 1])) key = 8u * tid + (uint32_t)k;
        key = block_min(key);
        if (key == NONE && n > LAT_SEARCH0 + 1u) {
            uint32_t k2 = NONE;
            for (uint32_t i = LAT_SEARCH0 + tid; i < LAT_SEARCH1 && i + 1u < n; i += BBOX_THREADS)
                if (backward(pts[i], pts[i + 1u])) k2 = min(k2, i);
            key = block_min(k2);
        }
    }
    const uint32_t rf = hinted ? hf : key == NONE ? 0u : key + 1u;
    const bool cand = lattice_shape_ok(rf, n);      // block-uniform
    if (cand && rf != hf) {                         // first build of a size, or the points changed shape
        if (wide) pass(std::integral_constant<int, 4>{}, rf, false); else pass(std::integral_constant<int, 8>{}, rf, false);
    }
    if (blockIdx.x == 0 && tid == 0) {
        a.sparams->lat_cand[0] = cand ? rf : 0u;
        a.sparams->lat_cand[1] = axis;
    }
    x0 = wave_min_bcast(x0); y0 = wave_min_bcast(y0);
    x1 = wave_max_bcast(x1); y1 = wave_max_bcast(y1);
    ax = wave_max_bcast(ax); ay = wave_max_bcast(ay); bx = wave_max_bcast(bx); by = wave_max_bcast(by);
    __syncthreads();
    if (lane == 0) { sh[wave][0] = x0; sh[wave][1] = y0; sh[wave][2] = x1; sh[wave][3] = y1; sh[wave][4] = ax; sh[wave][5] = ay; sh[wave][6] = bx; sh[wave][7] = by; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) {
            x0 = fminf(x0, sh[w][0]); y0 = fminf(y0, sh[w][1]);
            x1 = fmaxf(x1, sh[w][2]); y1 = fmaxf(y1, sh[w][3]);
            ax = fmaxf(ax, sh[w][4]); ay = fmaxf(ay, sh[w][5]); bx = fmaxf(bx, sh[w][6]); by = fmaxf(by, sh[w][7]);
        }
        a.sboxes[blockIdx.x] = make_float4(x0, y0, x1, y1);
        a.slat[blockIdx.x] = make_float4(ax, ay, bx, by);
    }
}

// a plan built on an existing samples workspace has no bbox launch in front of it: its counters
// are zeroed by this one
__global__ __launch_bounds__(256) void plan_zero_kernel(BuildArgs a) {
    zero_words(a.counts, a.zero_words);
    if (a.zero_gacc) zero_words((uint32_t*)a.gacc, 8u * a.N);
    if (blockIdx.x == 0 && threadIdx.x < PLAN_BAR_WORDS) a.params->bar[threadIdx.x] = 0u;
}

// every workgroup of the count kernel reduces the PLAN_BBOX_BLOCKS partials (4 KB, L2 resident)
// sbox[0..3] = the box; sbox[4..7] = the largest neighbour steps {along x, along y, across x, across y} (meaningful
// when the first launch had a lattice candidate; a NaN partial cannot occur: the first launch turns it into +inf)
__device__ __forceinline__ void reduce_boxes(const float4* boxes, const float4* lat, uint32_t nparts, float* sbox, float (*sh)[8]) {
    static_assert(PLAN_BBOX_BLOCKS == 512, "one or two partials per thread");
    const float4 p = boxes[threadIdx.x];
    const float4 l = lat[threadIdx.x];
    float v[8] = {p.x, p.y, p.z, p.w, l.x, l.y, l.z, l.w};
    if (nparts > 256u) {      // launch-uniform
        const float4 p2 = boxes[256 + threadIdx.x];
        const float4 l2 = lat[256 + threadIdx.x];
        v[0] = fminf(v[0], p2.x); v[1] = fminf(v[1], p2.y); v[2] = fmaxf(v[2], p2.z); v[3] = fmaxf(v[3], p2.w);
        v[4] = fmaxf(v[4], l2.x); v[5] = fmaxf(v[5], l2.y); v[6] = fmaxf(v[6], l2.z); v[7] = fmaxf(v[7], l2.w);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (k & 2) || k >= 4 ? wave_max_bcast(v[k]) : wave_min_bcast(v[k]);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) sh[wave][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float r = sh[0][k];
        for (int w = 1; w < 4; ++w) r = (k & 2) || k >= 4 ? fmaxf(r, sh[w][k]) : fminf(r, sh[w][k]);
        sbox[k] = r;
    }
}
// the decision behind a lattice candidate (plan.h, SampleParams::lat): an 8 x 8 index tile is at most 7 (along +
// across) steps wide and high; it must be at most twice as wide and as high as its share of the bounding box (an
// exact lattice: 7/8 of it).  Uniform over the launch: every workgroup reduces the same partials.
__device__ __forceinline__ bool lattice_compact(const float* sbox, uint32_t rf, uint32_t rs, uint32_t axis) {
    if (rf == 0u) return false;
    const float ex = sbox[2] - sbox[0], ey = sbox[3] - sbox[1];
    const float nx = (float)(axis ? rs : rf), ny = (float)(axis ? rf : rs);      // points along x / along y
    return 7.f * (sbox[4] + sbox[6]) * nx <= 16.f * ex && 7.f * (sbox[5] + sbox[7]) * ny <= 16.f * ey;      // NaN / inf: false
}

// Launch 2: cell key of every Gaussian / point and its rank inside the cell, with ONE returning
// atomic per run of equal keys in a wave (points of a regular grid arrive in runs that share a
// cell): the run leader adds the run length to the cell counter, the others take consecutive
// ranks behind it.  run_* split the step so that several independent atomics are in flight.
struct Run { int start; uint32_t len; bool leader; };
__device__ __forceinline__ Run run_of(uint32_t k, int lane) {
    const uint32_t prev = __shfl_up(k, 1);
    Run r;
    r.leader = lane == 0 || k != prev;
    const uint64_t lm = __ballot(r.leader);
    const uint64_t upto = (2ull << lane) - 1ull;          // bits 0..lane (lane 63: all ones)
    r.start = 63 - __builtin_clzll(lm & upto);
    const uint64_t above = lm & ~upto;
    r.len = (uint32_t)((above ? __builtin_ctzll(above) : 64) - lane);   // meaningful for leaders
    return r;
}

// The coarse-bin path's first pass (plan.h): workgroup w ranks its chunk of the point array inside every coarse
// bin with LDS atomics (one per point; random points spread over the 256 counters) and publishes its 256 counts
// as column w of the (bin, workgroup) matrix; a point keeps {fine cell, rank in (bin, workgroup)}.
__device__ __forceinline__ void samples_hist_part(const BuildArgs& a, uint32_t w, const SampleGrid& sg, uint32_t* lh, int lane);

// The Gaussians' half of the count: cell key (level by size, cell by centre) and rank of every Gaussian.  `box`: the
// samples' bounding box the grid's domain is laid over -- of this build, or (BuildArgs::ahead) of the last one.
struct GaussLoad { float m[2], c[3], v[2]; };      // (v: loaded by builds that keep the caller's order alone)
// One Gaussian into its place in cell order: records, the box the walk through the cells tests first, the way back.
__device__ __forceinline__ void gauss_scatter_one(const BuildArgs& a, uint32_t i, uint32_t pos) {
    float v[2] = {0.f, 0.f};
    for (int k = 0; k < a.c; ++k) v[k] = a.values[(size_t)i * a.c + k];
    // {mux, muy, a, b}, {c, v0, v1, 0}
    a.rec[2 * pos] = make_float4(a.means[2 * i], a.means[2 * i + 1], a.conics[3 * i], a.conics[3 * i + 1]);
    a.rec[2 * pos + 1] = make_float4(a.conics[3 * i + 2], v[0], v[1], 0.f);
    if (i == 0) {         // record N: all zero (v = 0 contributes nothing), what list positions behind a list's end read
        a.rec[2 * (size_t)a.N] = make_float4(0.f, 0.f, 0.f, 0.f);
        a.rec[2 * (size_t)a.N + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    {   // bounding box of the q <= q_max ellipse: half extents sqrt(q_max Sigma_xx), sqrt(q_max Sigma_yy)
        const float ca = a.conics[3 * i], cb = a.conics[3 * i + 1], cc = a.conics[3 * i + 2];
        const float k = a.q_max / (ca * cc - cb * cb);
        float hx = sqrtf(k * cc), hy = sqrtf(k * ca);
        if (!(hx < 3.0e38f)) hx = 3.0e38f;      // NaN / inf (degenerate conic): always a candidate
        if (!(hy < 3.0e38f)) hy = 3.0e38f;
        a.gbox[pos] = make_float4(a.means[2 * i], a.means[2 * i + 1], hx * 1.0001f, hy * 1.0001f);
    }
    a.g2o[pos] = i;
    // (the backward's scratch `gacc` is zero from the workspace's first build on -- zeroed once by the first
    // launch of a build into a workspace that is not PIGS_BUILD_PLAN_WS_CLEAN, re-zeroed by plan_unpermute_kernel
    // behind every backward: no memset launch, and no 8 scattered stores per Gaussian here either)
}

// The boxes of the strips (16 consecutive Gaussians of the caller's array = a row of this wave's lanes) and of the
// super-strip (the workgroup's 256): the union of the boxes of their q <= q_max ellipses.  A strip box's area over the
// domain's goes to `parea` (summed by the list launch into PlanParams::strip_cover); the boxes themselves to `pbox` /
// `sbox` when the build keeps the caller's order (`store`; block-uniform -- a barrier inside).  Non-finite extents (a
// degenerate conic) and NaN centres make a strip reach everywhere.
__device__ __forceinline__ void strip_box(const BuildArgs& a, uint32_t i, bool valid, float mx, float my, float hx, float hy,
                                          const float* box, bool store) {
    __shared__ float4 rowbox[16];
    const float INF = __builtin_huge_valf();
    if (!(hx < 3.0e38f)) hx = INF;      // NaN too
    if (!(hy < 3.0e38f)) hy = INF;
    float x0 = valid ? mx - hx : INF, x1 = valid ? mx + hx : -INF;
    float y0 = valid ? my - hy : INF, y1 = valid ? my + hy : -INF;
    if (valid && !(mx == mx)) { x0 = -INF; x1 = INF; }      // a NaN centre: fminf / fmaxf would drop it
    if (valid && !(my == my)) { y0 = -INF; y1 = INF; }
    row_box_dpp(x0, x1, y0, y1);
    const bool first = (threadIdx.x & 15u) == 0u;
    if (first && i < a.N) {
        const uint32_t strip = i / STRIP;
        if (store) a.pbox[strip] = make_float4(x0, y0, x1, y1);
    }
    if (first && i < a.N && a.parea) {      // (launch-uniform: the build's statistics are wanted home)
        const uint32_t strip = i / STRIP;
        // inside the domain only: what lies outside meets no tile
        const float dx = box[2] - box[0], dy = box[3] - box[1];
        const float w = fminf(x1, box[2]) - fmaxf(x0, box[0]), h = fminf(y1, box[3]) - fmaxf(y0, box[1]);
        float cover = (w > 0.f && h > 0.f && dx > 0.f && dy > 0.f) ? (w * h) / (dx * dy) : 0.f;
        if (!(cover == cover)) cover = 1.f;
        a.parea[strip] = cover;
    }
    if (!store) return;
    if (first) rowbox[threadIdx.x >> 4] = make_float4(x0, y0, x1, y1);
    __syncthreads();
    if (threadIdx.x == 0 && i < a.N) {
        float4 b = rowbox[0];
        for (int r = 1; r < 16; ++r) {
            const float4 q = rowbox[r];
            b.x = fminf(b.x, q.x); b.y = fminf(b.y, q.y); b.z = fmaxf(b.z, q.z); b.w = fmaxf(b.w, q.w);
        }
        a.sbox[i / SUPER] = b;
    }
}
// A build that keeps the caller's order (PlanParams::strips): records, boxes and the way back at position i itself, the
// strip's box beside them -- the whole Gaussian half of a build in one pass, no atomics.  Everything comes from the
// registers gauss_count_load filled (one round trip to memory, nothing is loaded again), and only what a plan of strips
// reads is written: `gbox` belongs to the walk through the cells (grid_walk.h, traverse) and is left alone -- 16 B per
// Gaussian that every launch boundary would write back.
__device__ __forceinline__ void gauss_pack_part(const BuildArgs& a, uint32_t i, const float* box, const GaussLoad& ld) {
    const bool valid = i < a.N;
    float hx = 0.f, hy = 0.f;
    if (valid) {
        // {mux, muy, a, b}, {c, v0, v1, 0}
        a.rec[2 * i] = make_float4(ld.m[0], ld.m[1], ld.c[0], ld.c[1]);
        a.rec[2 * i + 1] = make_float4(ld.c[2], ld.v[0], ld.v[1], 0.f);
        if (i == 0) {         // record N: all zero (gauss_scatter_one)
            a.rec[2 * (size_t)a.N] = make_float4(0.f, 0.f, 0.f, 0.f);
            a.rec[2 * (size_t)a.N + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        a.g2o[i] = i;
        const float k = a.q_max / (ld.c[0] * ld.c[2] - ld.c[1] * ld.c[1]);
        hx = sqrtf(k * ld.c[2]) * 1.0001f; hy = sqrtf(k * ld.c[0]) * 1.0001f;      // (as gbox would hold them)
    }
    strip_box(a, i, valid, ld.m[0], ld.m[1], hx, hy, box, true);
}
__device__ __forceinline__ GaussLoad gauss_count_load(const BuildArgs& a, uint32_t bid) {      // (issued early: flies while the box is reduced)
    GaussLoad ld = {{0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f}};
    const uint32_t i = bid * 256 + threadIdx.x;
    if (i < a.N) {
        ld.m[0] = a.means[2 * i]; ld.m[1] = a.means[2 * i + 1];
        ld.c[0] = a.conics[3 * i]; ld.c[1] = a.conics[3 * i + 1]; ld.c[2] = a.conics[3 * i + 2];
        if (a.strips) {       // (launch-uniform) the pack forms the records from these registers
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (k < a.c) ld.v[k] = a.values[(size_t)i * a.c + k];
        }
    }
    return ld;
}
__device__ __forceinline__ void gauss_count_part(const BuildArgs& a, uint32_t bid, const float* box, const GaussLoad& ld) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = bid * 256 + threadIdx.x;
    const bool valid = i < a.N;
    const float* gm = ld.m;
    const float* gc = ld.c;
    const GaussGrid g = gauss_grid(box, a.G0);
    if (bid == 0 && threadIdx.x == 0) {
        a.params->gg = g;
        a.params->scan_error = 0;
        a.params->q_f = a.q_f;
        a.params->q_b = a.q_b;
        a.params->n_points = 0u;
        a.params->strips = a.strips ? 1u : 0u;
        a.params->points_wanted = 0u;
        a.params->lattice_broken = 0u;
        a.params->fwd_only = a.fwd_only ? 1u : 0u;
        if (a.strips) a.params->level_mask = 0u;
#pragma unroll
        for (int l = 0; l <= PLAN_MAX_LEVELS; ++l) a.params->level_off[l] = a.level_off[l];
    }
    if (a.strips) {                    // launch-uniform: the caller's order is kept (PlanParams::strips)
        gauss_pack_part(a, i, box, ld);
        return;
    }
    uint32_t key = 0xffffffffu;
    int l = 0;
    {   // the statistic the library decides the NEXT build's kind from: this wave's Gaussians as four strips
        float hx = 0.f, hy = 0.f;
        if (valid) {
            const float k = a.q_max / (gc[0] * gc[2] - gc[1] * gc[1]);
            hx = sqrtf(k * gc[2]); hy = sqrtf(k * gc[0]);
        }
        strip_box(a, i, valid, gm[0], gm[1], hx, hy, box, false);
    }
    if (valid) {
        const float mx = gm[0], my = gm[1];
        const float ca = gc[0], cb = gc[1], cc = gc[2];
        // half extents of the q <= q_max ellipse: sqrt(q_max * Sigma_xx), Sigma = C^-1
        const float det = ca * cc - cb * cb;
        const float R = sqrtf(a.q_max * fmaxf(ca, cc) / det);   // NaN / inf (degenerate conic) -> top level
        float s = g.s0;
        while (l < a.L - 1 && !(R <= s)) { ++l; s *= 2.f; }
        const int G = a.G0 >> l;
        const float inv_s = 1.f / s;
        const int cx = (int)clampf((mx - g.ox) * inv_s, 0.f, (float)(G - 1));   // NaN -> 0
        const int cy = (int)clampf((my - g.oy) * inv_s, 0.f, (float)(G - 1));
        key = a.level_off[l] + ((uint32_t)(cy * G + cx) << level_shift((uint32_t)(G * G)));
    }
    const Run r = run_of(key, lane);
    uint32_t base = 0;
    if (r.leader && valid) base = atomicAdd(&a.counts[key], r.len);
    base = __shfl(base, r.start);
    if (valid) a.gkey[i] = make_uint2(key, base + (uint32_t)(lane - r.start));
}

__device__ __forceinline__ void gauss_count_ahead(const BuildArgs& a, uint32_t bid) {
    gauss_count_part(a, bid, a.hint_box, gauss_count_load(a, bid));
}

template <bool COH>
__device__ __forceinline__ void scan_block(const BuildArgs& a, bool seg0, uint32_t b, uint32_t* sh, uint32_t* sh2);

// One barrier = 17 words: arrivals are counted per XCD-sized group of workgroups (id & 7: 32 arrivals per
// address instead of 256 -- same-address atomics retire one every ~10 ns), the last arrival of a group
// counts the group in, the last group raises eight release flags and every workgroup polls its own group's
// (32 pollers per address).
__device__ __forceinline__ void grid_barrier(uint32_t* bar, uint32_t G, uint32_t id) {      // id: this workgroup among the G that meet
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");      // this wave's memory operations have completed
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t grp = id & 7u;
        const uint32_t in_grp = (G - grp + 7u) >> 3, groups = G < 8u ? G : 8u;
        if (__hip_atomic_fetch_add(&bar[grp], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == in_grp - 1u) {
            if (__hip_atomic_fetch_add(&bar[8], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == groups - 1u) {
#pragma unroll
                for (int k = 0; k < 8; ++k) __hip_atomic_store(&bar[9 + k], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        while (__hip_atomic_load(&bar[9 + grp], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) __builtin_amdgcn_s_sleep(2);
    }
    __syncthreads();
}

// BuildArgs::sort_in_count: the rest of a one-pass sort behind the count, in the count's own launch -- for points that
// were expected to be a lattice (so that the host launched nothing behind this for them) and are none.  `ns` sample
// workgroups (all resident: the host launches at most 256), this one the `sid`-th: everybody's counters are final behind
// the first barrier; the scan's blocks are dealt out in turn (every workgroup takes its blocks in rising order and a
// block looks back at lower ones only: nobody waits on somebody who waits on him), past the caches; behind the second
// barrier every thread moves the points it keyed itself.  Slow next to three launches (two device-wide barriers), and
// rare: the memory turns around.
__device__ __forceinline__ void samples_sort_in_count(const BuildArgs& a, uint32_t sid, uint32_t ns, uint32_t* sh, uint32_t* sh2, int lane) {
    grid_barrier(&a.sparams->bar[0], ns, sid);
    for (uint32_t b = sid; b < a.s_scan_blocks; b += ns) {
        scan_block<true>(a, false, b, sh, sh2);
        __syncthreads();                      // sh / sh2 are the next block's
    }
    grid_barrier(&a.sparams->bar[17], ns, sid);
    for (uint32_t sb = sid; sb < a.s_blocks; sb += ns) {
        const uint32_t i0 = (sb * 4 + (threadIdx.x >> 6)) * 256 + (uint32_t)lane;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t i = i0 + 64 * k;
            if (i < a.M) {
                const uint2 kr = a.skey[i];          // (this thread's own store)
                const float2 p = ((const float2*)a.samples)[i];
                SPoint sp;
                sp.x = p.x; sp.y = p.y; sp.m = i;
                a.spts[__hip_atomic_load(&a.sstarts[kr.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + kr.y] = sp;
            }
        }
    }
}

__global__ __launch_bounds__(256) void plan_count_kernel(BuildArgs a) {
    __shared__ float shb[4][8];
    __shared__ uint32_t lh[SAMPLES_COARSE_BINS];
    __shared__ uint32_t scan_sh[4], scan_sh2[4];
    const int lane = threadIdx.x & 63;
    // BuildArgs::ahead: the Gaussians were counted in the first launch -- the first workgroups of THIS one scan their
    // cells (look-back among the launch's first workgroups, as in plan_scan_kernel), the samples' workgroups follow
    const uint32_t shift = a.ahead && !a.strips ? a.scan_blocks : 0u;
    if (blockIdx.x < shift) {                            // block-uniform
        scan_block<false>(a, true, blockIdx.x, scan_sh, scan_sh2);
        return;
    }
    const uint32_t bid = blockIdx.x - shift, nb = gridDim.x - shift;
    // Every dependent memory round trip costs 2-4 us in this kernel (in-kernel stamps): issue the
    // workgroup's own loads first, so they fly while the bounding-box partials are reduced.
    const uint32_t gblocks = a.do_plan && !a.ahead ? (a.N + 255) / 256 : 0;
    const bool gpart = bid < gblocks;
    float2 pt[4];
    uint32_t i0 = ((bid - gblocks) * 4 + (threadIdx.x >> 6)) * 256 + lane;
    // the first launch's lattice candidate (plan.h): with one, the sample workgroups most likely have nothing to do
    // (a trusted build has no first launch and no sample workgroups: every workgroup packs Gaussians)
    const bool looked = a.do_samples && !a.trusted;
    const uint32_t lat_rf = looked ? a.sparams->lat_cand[0] : 0u;
    const uint32_t lat_axis = looked ? a.sparams->lat_cand[1] : 0u;
    auto load_points = [&]() {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t i = i0 + 64 * k;
            pt[k] = i < a.M ? ((const float2*)a.samples)[i] : make_float2(0.f, 0.f);
        }
    };
    GaussLoad gld = {{0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f}};
    if (gpart) gld = gauss_count_load(a, bid);
    else if (!a.coarse && lat_rf == 0u) load_points();
    float sbox[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool lattice = false;
    if (a.trusted) {      // (launch-uniform) the remembered box, from the kernel arguments: the header is being written
#pragma unroll
        for (int k = 0; k < 4; ++k) sbox[k] = a.hint_box[k];
        if (bid == 0 && threadIdx.x == 0) {
            // the header the decision launch would have left for a lattice of this row length on this box
            SampleParams* sp = a.sparams;
#pragma unroll
            for (int k = 0; k < 4; ++k) sp->box[k] = sbox[k];
            sp->sg = sample_grid(sbox, a.M, a.scells_cap);
            sp->scan_error = 0;
            sp->order_stat[0] = 0u; sp->order_stat[1] = 0u;
            sp->lat_cand[0] = a.rf_hint; sp->lat_cand[1] = a.hint_axis;
            sp->lat[0] = a.rf_hint; sp->lat[1] = a.M / a.rf_hint;
            sp->src = (uint64_t)(uintptr_t)a.samples;
        }
        gauss_count_part(a, bid, sbox, gld);      // (gpart: the launch is the Gaussians' workgroups)
        return;
    }
    if (a.do_samples) {
        reduce_boxes(a.sboxes, a.slat, a.bbox_blocks, sbox, shb);
        lattice = lattice_compact(sbox, lat_rf, lat_rf ? a.M / lat_rf : 0u, lat_axis);
    } else {      // the samples workspace is complete: its box is in its header
#pragma unroll
        for (int k = 0; k < 4; ++k) sbox[k] = a.sparams->box[k];
    }
    const SampleGrid sg = sample_grid(sbox, a.M, a.scells_cap);
    if (bid == gblocks && threadIdx.x == 0 && a.do_samples) {      // (the first of the samples' workgroups)
#pragma unroll
        for (int k = 0; k < 4; ++k) a.sparams->box[k] = sbox[k];
        a.sparams->sg = sg;
        a.sparams->scan_error = 0;
        a.sparams->lat[0] = lattice ? lat_rf : 0u;
        a.sparams->lat[1] = lattice ? a.M / lat_rf : 0u;
        a.sparams->src = lattice ? (uint64_t)(uintptr_t)a.samples : 0ull;
    }
    // Gaussian workgroups first, sample workgroups after them: the two halves are independent
    // latency chains (load -> returning atomic -> store) and run concurrently on different CUs
    if (gpart) {                        // block-uniform: whole waves enter
        gauss_count_part(a, bid, sbox, gld);
    } else if (lattice) {
        // index-tiled: nothing to key, count or move (block-uniform)
    } else if (a.coarse) {
        samples_hist_part(a, bid - gblocks, sg, lh, lane);
    } else {
    // the one-pass count: a sample workgroup takes 1 024 points at a time -- one block where the launch has a workgroup
    // per block; where the host expected a lattice (rf_hint) and launched an eighth of them, the workgroups stride
    // over the blocks: the points that were no lattice after all are still all counted, by fewer hands
    for (uint32_t sb = bid - gblocks; sb < a.s_blocks; sb += nb - gblocks) {
        const bool first = sb == bid - gblocks;
        i0 = (sb * 4 + (threadIdx.x >> 6)) * 256 + lane;
        if (!first || lat_rf != 0u) load_points();      // (the first block's loads were issued early unless a lattice candidate stood)
        // each wave: 4 steps of 64 consecutive points, their atomics issued back to back
        uint32_t id[4], base[4];
        Run r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t i = i0 + 64 * k;
            id[k] = 0xffffffffu;
            if (i < a.M) {
                const float2 p = pt[k];
                const int cx = (int)clampf((p.x - sg.ox) * sg.inv_w, 0.f, (float)(sg.nx - 1));
                const int cy = (int)clampf((p.y - sg.oy) * sg.inv_w, 0.f, (float)(sg.ny - 1));
                id[k] = sample_cell_id(cx, cy, sg.nx);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            r[k] = run_of(id[k], lane);
            base[k] = 0;
            if (r[k].leader && id[k] != 0xffffffffu)
                base[k] = atomicAdd(&a.scounts[id[k]], r[k].len);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t i = i0 + 64 * k;
            const uint32_t b = __shfl(base[k], r[k].start);
            if (i < a.M) a.skey[i] = make_uint2(id[k], b + (uint32_t)(lane - r[k].start));
        }
        if ((sb & 31u) == 0u && threadIdx.x < 64u) {      // a sample of the waves (one in 128): runs per point (SampleParams::order_stat)
            uint32_t runs = 0, pts = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                runs += (uint32_t)__builtin_popcountll(__ballot(r[k].leader && id[k] != 0xffffffffu));
                pts += (uint32_t)__builtin_popcountll(__ballot(id[k] != 0xffffffffu));
            }
            if (lane == 0) { atomicAdd(&a.sparams->order_stat[0], runs); atomicAdd(&a.sparams->order_stat[1], pts); }
        }
    }
    if (a.sort_in_count) samples_sort_in_count(a, bid - gblocks, nb - gblocks, scan_sh, scan_sh2, lane);      // (launch-uniform)
    }
}

__device__ __forceinline__ void samples_hist_part(const BuildArgs& a, uint32_t w, const SampleGrid& sg, uint32_t* lh, int lane) {
    static_assert(SAMPLES_COARSE_BINS == 256, "one bin per thread of the workgroup");
    lh[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t p0 = (uint64_t)w * a.h_chunk;
    const uint64_t p1 = p0 + a.h_chunk < (uint64_t)a.M ? p0 + a.h_chunk : (uint64_t)a.M;
    // the same statistic as the one-pass build keeps, from the chunk's first 256 points (all lanes present)
    const bool sampled = (w & 31u) == 0u && p0 + 256u <= p1;
    bool first = true;
    for (uint64_t i0 = p0 + threadIdx.x; i0 < p1; i0 += 1024u) {      // four loads in flight per thread
        float2 p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t i = i0 + 256u * k;
            p[k] = i < p1 ? ((const float2*)a.samples)[i] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t i = i0 + 256u * k;
            if (i < p1) {
                const int cx = (int)clampf((p[k].x - sg.ox) * sg.inv_w, 0.f, (float)(sg.nx - 1));
                const int cy = (int)clampf((p[k].y - sg.oy) * sg.inv_w, 0.f, (float)(sg.ny - 1));
                const uint32_t id = sample_cell_id(cx, cy, sg.nx);
                const uint32_t rank = atomicAdd(&lh[id / a.cells_per_bin], 1u);
                a.skey[i] = make_uint2(id, rank);
                if (sampled && first && k == 0) {
                    const Run r = run_of(id, lane);
                    const uint32_t runs = (uint32_t)__builtin_popcountll(__ballot(r.leader));
                    if (lane == 0) { atomicAdd(&a.sparams->order_stat[0], runs); atomicAdd(&a.sparams->order_stat[1], 64u); }
                }
            }
        }
        first = false;
    }
    __syncthreads();
    a.scounts[(size_t)threadIdx.x * a.h_wgs + w] = lh[threadIdx.x];
}

// Launch 3: exclusive scan counts -> starts in ONE launch, for the Gaussian cells and (when the
// samples are built alongside) the sample cells: two independent segments.  A workgroup scans
// PLAN_SCAN_BLOCK counters (one coalesced uint4 per thread), publishes its total as one 8-byte
// {flag, total} granule (single agent-scope store: data and flag travel together, no fence
// needed) and sums the granules of the workgroups before it; nobody waits on a later workgroup.
// The wait on a predecessor is bounded, and a predecessor that has not published within the bound is
// not an error: the counters are final before this launch starts (the count kernel has completed),
// so the waiting thread sums that workgroup's PLAN_SCAN_BLOCK counters ITSELF -- slower, never
// wrong, whatever order the hardware dispatches workgroups in.  `scan_error` in the workspace header
// only records that this happened (a diagnostic; never seen with in-order dispatch).
// `no_lookback` (PIGS_BUILD_DEBUG_NO_LOOKBACK) makes every thread take that path: the test hook.
constexpr uint32_t SCAN_SPIN_LIMIT = 1u << 14;
// COH: counters read and starts written with agent-scope accesses that bypass the (per-XCD, mutually
// incoherent) L2s -- for the one-launch chain, where producer and consumer phases of one launch run on
// different XCDs with no kernel boundary in between.
template <bool COH>
__device__ __forceinline__ uint4 scan_load4(const uint32_t* p) {
    if constexpr (COH) {
        uint4 v;
        v.x = __hip_atomic_load(p + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v.y = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v.z = __hip_atomic_load(p + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v.w = __hip_atomic_load(p + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return v;
    } else {
        return *(const uint4*)p;
    }
}
template <bool COH>
__device__ __forceinline__ void scan_block(const BuildArgs& a, bool seg0, uint32_t b, uint32_t* sh, uint32_t* sh2) {
    const uint32_t* counts = seg0 ? a.counts : a.scounts;
    unsigned long long* agg = seg0 ? a.agg : a.sagg;
    uint32_t* starts = seg0 ? a.starts : a.sstarts;
    uint32_t* err = seg0 ? &a.params->scan_error : &a.sparams->scan_error;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t q = b * 256 + threadIdx.x;          // uint4 index
    const uint4 v = scan_load4<COH>(counts + 4 * (size_t)q);
    const uint32_t s = v.x + v.y + v.z + v.w;
    uint32_t inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0 && !a.no_lookback)
        __hip_atomic_store(&agg[b], (1ull << 32) | (sh[0] + sh[1] + sh[2] + sh[3]), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    uint32_t pre = 0;
    for (uint32_t t = threadIdx.x; t < b; t += 256) {
        unsigned long long x = 0;
        if (!a.no_lookback) {
            for (uint32_t spins = 0; spins < SCAN_SPIN_LIMIT; ++spins) {
                x = __hip_atomic_load(&agg[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (x >> 32) break;
                __builtin_amdgcn_s_sleep(1);
            }
        }
        if (!(x >> 32)) {       // not published (in time): workgroup t's total from its counters
            const uint32_t* c4 = counts + (size_t)t * 1024;
            uint32_t tot = 0;
            for (int i = 0; i < 256; ++i) {
                const uint4 w = scan_load4<COH>(c4 + 4 * i);
                tot += w.x + w.y + w.z + w.w;
            }
            x = tot;
            atomicOr(err, 1u);
        }
        pre += (uint32_t)x;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pre += __shfl_xor(pre, o);
    if (lane == 0) sh2[wave] = pre;
    __syncthreads();
    uint32_t run = inc - s + sh2[0] + sh2[1] + sh2[2] + sh2[3];
    for (int w = 0; w < wave; ++w) run += sh[w];
    uint4 o4;
    o4.x = run; o4.y = run + v.x; o4.z = o4.y + v.y; o4.w = o4.z + v.z;
    // counters beyond the last cell are zero: starts[ncells] = total
    if constexpr (COH) {
        uint32_t* d = starts + 4 * (size_t)q;
        __hip_atomic_store(d + 0, o4.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(d + 1, o4.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(d + 2, o4.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(d + 3, o4.w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        ((uint4*)starts)[q] = o4;
    }
}
__global__ __launch_bounds__(256) void plan_scan_kernel(BuildArgs a) {
    __shared__ uint32_t sh[4];
    __shared__ uint32_t sh2[4];
    const uint32_t nb0 = a.do_plan && !a.strips ? a.scan_blocks : 0;
    const bool seg0 = blockIdx.x < nb0;
    if (!seg0 && a.sparams->lat[0] != 0u) return;      // index-tiled points: nothing was counted (block-uniform)
    scan_block<false>(a, seg0, seg0 ? blockIdx.x : blockIdx.x - nb0, sh, sh2);
}

// Launch 4: scatter into sorted order (no atomics: position = cell start + rank) and publish the
// level mask.
// The coarse-bin path's scatter (plan.h): workgroup w moves ITS chunk of the point array (the chunk it ranked in
// samples_hist_part) to the bins' segments of the temporary array.  The chunk is first laid out bin by bin in LDS
// (slot = the workgroup's own exclusive scan over its 256 bin counts + the point's rank), then written out slot
// by slot: consecutive threads write consecutive 16-byte records of a bin's run, where a direct scatter sends
// every lane of a store to another line (16.7 -> 12.2 us at 1 M random points).  count(bin, w) is the difference
// of neighbouring entries of the scanned matrix.
__device__ __forceinline__ void samples_scatter_part(const BuildArgs& a, uint32_t w, uint4* stage, uint32_t* lscan, uint32_t* gbase) {
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const uint64_t p0 = (uint64_t)w * a.h_chunk;
    const uint64_t p1 = p0 + a.h_chunk < (uint64_t)a.M ? p0 + a.h_chunk : (uint64_t)a.M;
    if (p0 >= p1) return;                     // block-uniform: a padding workgroup of the matrix
    {   // thread = bin: this workgroup's count in the bin, scanned over the bins
        const size_t e = (size_t)tid * a.h_wgs + w;
        const uint32_t hs = a.sstarts[e];
        const uint32_t nx = e + 1 < (size_t)SAMPLES_COARSE_BINS * a.h_wgs ? a.sstarts[e + 1] : a.M;
        const uint32_t c = nx - hs;
        uint32_t inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(inc, o);
            if (lane >= o) inc += v;
        }
        __shared__ uint32_t ws[4];
        if (lane == 63) ws[wave] = inc;
        __syncthreads();
        uint32_t run = inc - c;
        for (int k = 0; k < wave; ++k) run += ws[k];
        lscan[tid] = run;
        gbase[tid] = hs;
    }
    __syncthreads();
    for (uint64_t i0 = p0 + tid; i0 < p1; i0 += 1024u) {
        uint2 kr[4];
        float2 p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t i = i0 + 256u * k;
            kr[k] = i < p1 ? a.skey[i] : make_uint2(0u, 0u);
            p[k] = i < p1 ? ((const float2*)a.samples)[i] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t i = i0 + 256u * k;
            if (i < p1)
                stage[lscan[kr[k].x / a.cells_per_bin] + kr[k].y] =
                    make_uint4(__float_as_uint(p[k].x), __float_as_uint(p[k].y), (uint32_t)i, kr[k].x);
        }
    }
    __syncthreads();
    const uint32_t n = (uint32_t)(p1 - p0);
    uint4* tmp4 = (uint4*)a.tmp;
    for (uint32_t slot = tid; slot < n; slot += 256u) {
        const uint4 r = stage[slot];
        const uint32_t bin = r.w / a.cells_per_bin;
        tmp4[gbase[bin] + (slot - lscan[bin])] = r;
    }
}

// A workgroup scans ALL `nblocks` blocks of 1 024 counters itself, a block at a time through LDS (the counters are
// final: the count launch has completed), and every thread picks the start of ITS key out of the block that holds
// it.  ~0.7 us per block and workgroup: the slow way round, taken by the samples' workgroups of launch 3 of
// BuildArgs::ahead when the points they expected to be a lattice are none (the memory then turns around).  (As a
// replacement of the Gaussians' scan launch it was measured: 43 blocks, scatter 5.4 -> 28.9 us)
__device__ __forceinline__ uint32_t scan_pick(const uint32_t* counts, uint32_t nblocks, uint32_t key, uint32_t* lds, uint32_t* ws) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0, mine = 0;
    for (uint32_t c0 = 0; c0 < nblocks; c0 += 8u) {
        uint4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            v[k] = c0 + (uint32_t)k < nblocks ? ((const uint4*)counts)[(size_t)(c0 + (uint32_t)k) * 256 + threadIdx.x] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t c = c0 + (uint32_t)k;
            if (c >= nblocks) break;                       // block-uniform
            const uint32_t sum = v[k].x + v[k].y + v[k].z + v[k].w;
            uint32_t inc = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = __shfl_up(inc, o);
                if (lane >= o) inc += t;
            }
            if (lane == 63) ws[wave] = inc;
            __syncthreads();
            uint32_t base = carry + inc - sum;
            for (int w = 0; w < wave; ++w) base += ws[w];
            const uint32_t tot = ws[0] + ws[1] + ws[2] + ws[3];
            ((uint4*)lds)[threadIdx.x] = make_uint4(base, base + v[k].x, base + v[k].x + v[k].y, base + v[k].x + v[k].y + v[k].z);
            __syncthreads();
            if ((key >> 10) == c) mine = lds[key & 1023u];
            carry += tot;
            __syncthreads();                               // lds / ws are the next block's
        }
    }
    return mine;
}

__global__ __launch_bounds__(256) void plan_scatter_kernel(BuildArgs a) {
    extern __shared__ uint4 scatter_stage[];      // coarse-bin path with a chunk that fits: [h_chunk] records + 2 x 256 words
    __shared__ uint32_t scan_lds[PLAN_SCAN_BLOCK];
    __shared__ uint32_t scan_ws[4];
    const uint32_t gblocks = a.do_plan && !a.strips ? (a.N + 255) / 256 : 0;      // (strips: the Gaussians are in place already)
    const bool gpart = blockIdx.x < gblocks;
    const uint32_t i = (gpart ? blockIdx.x : blockIdx.x - gblocks) * 256 + threadIdx.x;
    if (a.do_plan && !a.strips && blockIdx.x == 0 && threadIdx.x < 64) {
        // level l holds a Gaussian iff its cells' scanned range is not empty (no atomics, no scratch)
        const int l = (int)threadIdx.x;
        const int lc = l < a.L ? l : 0;
        const bool occ = l < a.L && a.starts[a.level_off[lc + 1]] != a.starts[a.level_off[lc]];
        const uint64_t m = __ballot(occ);
        if (threadIdx.x == 0) a.params->level_mask = (uint32_t)m;
    }
    if (a.do_plan && !a.strips) {
        // the scan has consumed the counters and its own flags: leave them zeroed, so that a later
        // build into this workspace (PIGS_BUILD_PLAN_WS_CLEAN) needs no zeroing launch
        for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < a.zero_words; k += gridDim.x * 256) a.counts[k] = 0u;
    }
    if (!gpart && a.sparams->lat[0] != 0u) return;     // index-tiled points: nothing to move (block-uniform)
    if (!gpart && a.coarse && a.h_chunk <= SCATTER_STAGE_MAX) {
        // (the sample workgroups of this launch are then the chunks' workgroups: h_wgs of them)
        uint32_t* words = (uint32_t*)(scatter_stage + a.h_chunk);
        samples_scatter_part(a, blockIdx.x - gblocks, scatter_stage, words, words + SAMPLES_COARSE_BINS);
        return;
    }
    if (gpart && i < a.N) {
        const uint2 kr = a.gkey[i];
        gauss_scatter_one(a, i, a.starts[kr.x] + kr.y);
    }
    uint32_t sstart = 0;
    if (!gpart && a.s_scan_in_scatter) {      // block-uniform: an expected lattice that was none, and no scan launch ran
        const uint2 kr = i < a.M ? a.skey[i] : make_uint2(0xffffffffu, 0u);
        sstart = scan_pick(a.scounts, a.s_scan_blocks, kr.x, scan_lds, scan_ws);
    }
    if (!gpart && i < a.M) {
        const uint2 kr = a.skey[i];
        const float2 p = ((const float2*)a.samples)[i];
        if (a.s_scan_in_scatter) {
            SPoint sp;
            sp.x = p.x; sp.y = p.y; sp.m = i;
            a.spts[sstart + kr.y] = sp;
        } else if (a.coarse) {
            // coarse-bin path: to the point's bin segment of the temporary array, behind the points that earlier
            // workgroups (chunks) sent to this bin; the fine cell travels along
            const uint32_t w = i / a.h_chunk, bin = kr.x / a.cells_per_bin;
            STmp t;
            t.x = p.x; t.y = p.y; t.m = i; t.id = kr.x;
            a.tmp[a.sstarts[(size_t)bin * a.h_wgs + w] + kr.y] = t;
        } else {
            SPoint sp;
            sp.x = p.x; sp.y = p.y; sp.m = i;
            a.spts[a.sstarts[kr.x] + kr.y] = sp;
        }
    }
}

// Last launch of the coarse-bin path: one workgroup per coarse bin counting-sorts the bin's segment of the
// temporary array by fine cell into the final array.  LDS: one counter per fine cell of the bin (count, then
// -- scanned in place -- cursor).  Segments up to 8 192 points are read once (registers); the writes stay inside
// the segment.  SUB = 16 (where the LDS holds 16 counters per cell: up to ~2 M points) also orders the points of a
// cell along the cell path continued into the cell (key_of below): a group is 16 consecutive sorted points, cells
// of unordered points hold 16 +- 4, so most groups straddle two cells, and with a cell's points in no order such
// a group's box spans both cells whole.  (A 4 x 4 Z-order of sub-cells was tried first: 41.9 -> 41.0 Gaussians
// per point at 1 M random points -- the halves of a Z-order are full-width strips.)  Order inside a key: as the
// atomics fall.
template <int SUB>
__global__ __launch_bounds__(1024) void samples_binsort_kernel(BuildArgs a) {
    extern __shared__ uint32_t cnt[];       // [cells_per_bin * SUB]
    __shared__ uint32_t wsum[16];
    constexpr int B = 8;                    // points a thread keeps in registers
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    if (a.sparams->lat[0] != 0u) return;               // index-tiled points: nothing to sort (block-uniform)
    const uint32_t seg0 = a.sstarts[(size_t)b * a.h_wgs];
    const uint32_t seg1 = b + 1 < SAMPLES_COARSE_BINS ? a.sstarts[(size_t)(b + 1) * a.h_wgs] : a.M;
    const uint32_t id0 = b * a.cells_per_bin, nkey = a.cells_per_bin * (uint32_t)SUB;
    const bool one_batch = seg1 - seg0 <= (uint32_t)B * 1024u;      // block-uniform
    const uint4* tmp4 = (const uint4*)a.tmp;
    const SampleGrid sg = a.sparams->sg;
    auto key_of = [&](const uint4 t) -> uint32_t {
        uint32_t k = (t.w - id0) * (uint32_t)SUB;
        if constexpr (SUB == 16) {
            // The point's place on the cell path continued INTO the cell: the path through a 4 x 4 block of cells is the
            // order-2 Hilbert curve (sample_cell_id), whose order-4 refinement runs through the 4 x 4 sub-cells of every
            // cell from the side the path enters the cell to the side it leaves (its top nibble IS the cell's index
            // inside the block) -- so consecutive points stay neighbours across a cell border.  Coordinates: 4 bits per
            // axis inside the block, from the same clamped cell coordinates the cell id came from; x mirrored in the
            // right-to-left block rows, as there.
            const float u = clampf((__uint_as_float(t.x) - sg.ox) * sg.inv_w, 0.f, (float)(sg.nx - 1));
            const float v = clampf((__uint_as_float(t.y) - sg.oy) * sg.inv_w, 0.f, (float)(sg.ny - 1));
            const int cx = (int)u, cy = (int)v;
            uint32_t x = (uint32_t)(cx & 3) * 4u + min(3u, (uint32_t)((u - (float)cx) * 4.f));
            uint32_t y = (uint32_t)(cy & 3) * 4u + min(3u, (uint32_t)((v - (float)cy) * 4.f));
            if ((cy >> 2) & 1) x = 15u - x;
            uint32_t d = 0;
#pragma unroll
            for (uint32_t sbit = 8u; sbit > 0u; sbit >>= 1) {
                const uint32_t rx = (x & sbit) ? 1u : 0u, ry = (y & sbit) ? 1u : 0u;
                d += sbit * sbit * ((3u * rx) ^ ry);
                if (ry == 0u) {
                    if (rx == 1u) { x = 15u - x; y = 15u - y; }
                    const uint32_t tt = x; x = y; y = tt;
                }
            }
            k += d & 15u;      // NaN coordinates: cell (0, 0), sub-cell 0
        }
        return k;
    };
    uint4 r[B];
    uint32_t rk[B];
    if (one_batch) {                         // the loads fly while the counters are cleared
#pragma unroll
        for (int k = 0; k < B; ++k) {
            const uint32_t p = seg0 + (uint32_t)k * 1024u + tid;
            r[k] = p < seg1 ? tmp4[p] : make_uint4(0u, 0u, 0u, 0xffffffffu);
        }
    }
    for (uint32_t t = tid; t < nkey; t += 1024u) cnt[t] = 0u;
    __syncthreads();
    if (one_batch) {
#pragma unroll
        for (int k = 0; k < B; ++k) {
            rk[k] = r[k].w != 0xffffffffu ? key_of(r[k]) : 0xffffffffu;
            if (rk[k] != 0xffffffffu) atomicAdd(&cnt[rk[k]], 1u);
        }
    } else {
        // A segment longer than one batch: a dense patch of a clustered cloud, 100 k points and more in one bin -- 73 us for
        // this launch at sigma = 0.15, a third of that cloud's cold step.  What bounds it is ONE compute unit's memory
        // stream (the segment is read twice, 16 B per point: 3.7 MB at ~55 GB/s): batches of 4 loads with the next batch
        // in flight were measured slower (118 us), rounds of 8 loads the same (70), eight workgroups per bin each taking
        // a slice of the cells but reading the whole segment the same again (74, and 2 048 workgroups to launch cost the
        // uniform case 60 us).  Sixteen loads per thread and round:
        for (uint32_t p0 = seg0; p0 < seg1; p0 += 16u * 1024u) {
            uint4 t[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint32_t p = p0 + (uint32_t)k * 1024u + tid;
                t[k] = p < seg1 ? tmp4[p] : make_uint4(0u, 0u, 0u, 0xffffffffu);
            }
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (t[k].w != 0xffffffffu) atomicAdd(&cnt[key_of(t[k])], 1u);
        }
    }
    __syncthreads();
    // exclusive scan in place: thread t owns the `per` consecutive counters from t * per
    const uint32_t per = (nkey + 1023u) / 1024u;
    const uint32_t lo = tid * per, hi = lo + per < nkey ? lo + per : nkey;
    uint32_t sum = 0;
    for (uint32_t t = lo; t < hi; ++t) sum += cnt[t];
    uint32_t inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t run = inc - sum;
    for (int w2 = 0; w2 < wave; ++w2) run += wsum[w2];
    for (uint32_t t = lo; t < hi; ++t) {
        const uint32_t c = cnt[t];
        cnt[t] = run;
        run += c;
    }
    __syncthreads();
    auto place = [&](const uint4 t, uint32_t key) {
        const uint32_t k = atomicAdd(&cnt[key], 1u);
        SPoint sp;
        sp.x = __uint_as_float(t.x); sp.y = __uint_as_float(t.y); sp.m = t.z;
        a.spts[seg0 + k] = sp;
    };
    if (one_batch) {
#pragma unroll
        for (int k = 0; k < B; ++k)
            if (rk[k] != 0xffffffffu) place(r[k], rk[k]);
    } else {
        for (uint32_t p0 = seg0; p0 < seg1; p0 += 16u * 1024u) {
            uint4 t[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint32_t p = p0 + (uint32_t)k * 1024u + tid;
                t[k] = p < seg1 ? tmp4[p] : make_uint4(0u, 0u, 0u, 0xffffffffu);
            }
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (t[k].w != 0xffffffffu) place(t[k], key_of(t[k]));
        }
    }
}

// Workgroups are dispatched round-robin over the 8 XCDs (workgroup i runs on XCD i % 8) and every
// XCD has its own L2.  Tiles follow the domain block row by block row, so inside every group of
// 8 * PIGS_XCD_CHUNK consecutive workgroups XCD x takes the x-th contiguous run of PIGS_XCD_CHUNK:
// each L2 then holds the Gaussian records and lists of a strip of the domain instead of all of
// them, while the launch still sweeps the domain once from top to bottom.  Bijective for any grid
// size (blocks behind the last whole group keep their index).  0 = no remapping.
#ifndef PIGS_XCD_CHUNK
#define PIGS_XCD_CHUNK 256
#endif
template <uint32_t CHUNK>
__device__ __forceinline__ uint32_t xcd_block_chunk(uint32_t nblocks, uint32_t b) {      // nblocks: the blocks that take part; b: this one's index among them
    if constexpr (CHUNK > 0) {                                                            //   (helper workgroups in front of them: a multiple of 8, keep out)
        constexpr uint32_t GROUP = 8u * CHUNK;
        const uint32_t g = b / GROUP, r = b % GROUP;
        if ((g + 1) * GROUP > nblocks) return b;
        return g * GROUP + (r & 7u) * CHUNK + (r >> 3);
    } else {
        return b;
    }
}
template <uint32_t CHUNK>
__device__ __forceinline__ uint32_t xcd_block_chunk(uint32_t nblocks) { return xcd_block_chunk<CHUNK>(nblocks, blockIdx.x); }
__device__ __forceinline__ uint32_t xcd_block(uint32_t nblocks, uint32_t b) { return xcd_block_chunk<PIGS_XCD_CHUNK>(nblocks, b); }

}  // namespace pigs
