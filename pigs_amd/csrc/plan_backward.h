// Binned sampler, sampling kernels: the backward.  Included by plan.hip alone.
//
// One wave = one tile, as in the forward (plan_forward.h).  Backward: the tile list 64 entries at
// a time, split by the group masks into four per-row lists (ballot + mbcnt), rows reduced by a
// transposing DPP fold into an LDS table, one atomic per entry and value.  No workgroup barriers.
// Build-time knobs: PIGS_BWD_WAVES, PIGS_BWD_STEP.
#pragma once
#include "plan_forward.h"

#ifndef PIGS_BWD_WAVES
#define PIGS_BWD_WAVES 6      // waves per SIMD the backward kernel's register budget is held to (its LDS allows 6 workgroups per CU)
#endif

namespace pigs {

// ------------------------------------------------------------------------------------------
// Backward helpers: a step's records go to the wave's LDS once (slot = lane); the group masks are
// split into four per-row index lists holding LDS byte offsets, padded with the offset of an
// all-zero record to the longest of the four.
// ------------------------------------------------------------------------------------------
#ifndef PIGS_BWD_STEP
#define PIGS_BWD_STEP 64      // entries per step of the backward: its LDS (records, lists, sums table) scales with it
                              // (32 doubles the resident waves and splits C3's 49-entry lists in two steps: 83 vs 81 us)
#endif
constexpr int BWD_STEP = PIGS_BWD_STEP;
static_assert(BWD_STEP == 32 || BWD_STEP == 64, "entries per step");
constexpr int LIST_PAD = 8;
struct TileLds {
    float4 rec[BWD_STEP + 1][2];            // slot BWD_STEP: the all-zero record (v = 0: contributes nothing)
    uint16_t list[4][BWD_STEP + LIST_PAD];  // byte offsets into rec (< 2 112)
};
constexpr uint32_t ZERO_REC_OFF = BWD_STEP * 32u;

// splits the step's masks; returns the padded row count (a multiple of UNROLL); rank[g] = position of
// this lane's entry in group g's list (meaningful where its mask bit is set)
template <int UNROLL>
__device__ __forceinline__ int split_step(TileLds& lds, uint32_t gm, int lane, int* rank) {
    int cnt[4], rows = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const bool bit = gm >> g & 1u;
        const uint64_t m = __ballot(bit);
        rank[g] = lanes_below(m);
        if (bit) lds.list[g][rank[g]] = (uint16_t)(lane * 32);
        cnt[g] = __builtin_popcountll(m);
        rows = cnt[g] > rows ? cnt[g] : rows;
    }
    rows = (rows + UNROLL - 1) / UNROLL * UNROLL;
#pragma unroll
    for (int g = 0; g < 4; ++g)
        if (cnt[g] + lane < rows + UNROLL) lds.list[g][cnt[g] + lane] = (uint16_t)ZERO_REC_OFF;   // + UNROLL: the prefetch
    return rows;
}

// ------------------------------------------------------------------------------------------
// Backward: the same tile / list structure.  Every (row, Gaussian) pair of a step yields
// NV = 5 + c per-lane contributions that must be summed over the row's 16 points.  The row sums
// are written -- plain stores, no read-modify-write: a (group, list position) pair is met once --
// into an LDS table indexed by group and list position; at the end of the step every lane, which
// knows the positions of its own entry in the (up to four) group lists from the split, adds its
// rows of the table and flushes ONE atomic per entry and value into gacc[k][j] (entries follow the
// sorted order, so consecutive lanes hit near-consecutive addresses); plan_unpermute_kernel writes
// the caller's layout.  (LDS float atomics into a per-entry table took 44 LDS cycles per
// instruction here: the kernel ran at the LDS's pace.)
// ------------------------------------------------------------------------------------------
// Round 4: the table holds HALF a step's list positions (BWD_HALF); the rows of a step are taken in two halves and an
// entry's lane collects its rows of the table after each (registers), so that the step's LDS is 6.1 KB per wave instead
// of 9.8 and SIX workgroups fit a CU where four did (the row arithmetic is what bounds the kernel).
constexpr int BWD_HALF = BWD_STEP / 2;
template <int NV>
struct TileLdsBwd {
    static constexpr int S = NV <= 6 ? 6 : 8;        // floats per table row (8-byte aligned)
    TileLds t;
    float sums[4][BWD_HALF + 4][S];                  // [group][list position - first of the half]: reduced contributions
};

// Row sums of FOUR wave-rows at once by a transposing fold.  Input: v[u][k], u = 0..3 (four consecutive
// list rows), k < NV, each to be summed over the 16 lanes of every DPP row.  Two folding levels merge
// the four u of one k into ONE register while they halve the lanes twice: bank_mask lets a DPP add
// write only some of a row's four banks (4 lanes each), so two adds build one merged register --
//   level A (row_ror:8, lanes i <-> i^8):       banks {0,1} <- v[u0] ,  banks {2,3} <- v[u1]
//   level B (row_half_mirror, i <-> 7-i of 8):   banks {0,2} <- first ,  banks {1,3} <- second
// -- then two quad steps finish the sum inside each bank.  6 + 2 instructions per k and four rows
// = 2 NV per row instead of 4 NV.  Afterwards every lane of bank b of a DPP row holds, in z[k], the
// sum over that row's 16 lanes of v[SIGMA(b)][k], SIGMA = {0, 2, 1, 3}.
#define PIGS_FOLD_A(OUT, X, Y)                                                            \
    "v_add_f32_dpp " OUT ", " X ", " X " row_ror:8 row_mask:0xf bank_mask:0x3\n\t"        \
    "v_add_f32_dpp " OUT ", " Y ", " Y " row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
#define PIGS_FOLD_B(OUT, X, Y)                                                            \
    "v_add_f32_dpp " OUT ", " X ", " X " row_half_mirror row_mask:0xf bank_mask:0x5\n\t"  \
    "v_add_f32_dpp " OUT ", " Y ", " Y " row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
// two values k at a time: their chains are interleaved, so that one s_nop at the head covers the two
// wait states a DPP read needs behind the VALU write of its source
__device__ __forceinline__ void fold4_pair(float& z0, float& z1, float a0, float a1, float a2, float a3, float b0,
                                           float b1, float b2, float b3) {
    float t0, t1, t2, t3;
    asm volatile("s_nop 1\n\t"
                 PIGS_FOLD_A("%2", "%6", "%7") PIGS_FOLD_A("%3", "%8", "%9")
                 PIGS_FOLD_A("%4", "%10", "%11") PIGS_FOLD_A("%5", "%12", "%13")
                 PIGS_FOLD_B("%0", "%2", "%3") PIGS_FOLD_B("%1", "%4", "%5")
                 : "=&v"(z0), "=&v"(z1), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
                 : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(b0), "v"(b1), "v"(b2), "v"(b3));
}
__device__ __forceinline__ void fold4_single(float& z0, float a0, float a1, float a2, float a3) {
    float t0, t1;
    asm volatile("s_nop 1\n\t"
                 PIGS_FOLD_A("%1", "%3", "%4") PIGS_FOLD_A("%2", "%5", "%6")
                 "s_nop 1\n\t"
                 PIGS_FOLD_B("%0", "%1", "%2")
                 : "=&v"(z0), "=&v"(t0), "=&v"(t1)
                 : "v"(a0), "v"(a1), "v"(a2), "v"(a3));
}
#define PIGS_QUAD1(MOD, R) "v_add_f32_dpp " R ", " R ", " R " " MOD " row_mask:0xf bank_mask:0xf\n\t"
#define PIGS_QUAD6(MOD) PIGS_QUAD1(MOD, "%0") PIGS_QUAD1(MOD, "%1") PIGS_QUAD1(MOD, "%2") PIGS_QUAD1(MOD, "%3") \
    PIGS_QUAD1(MOD, "%4") PIGS_QUAD1(MOD, "%5")
template <int NV>
__device__ __forceinline__ void quad_sums(float* z) {
    static_assert(NV == 6 || NV == 7, "5 + c values");
    if constexpr (NV == 6)
        asm volatile("s_nop 1\n\t" PIGS_QUAD6("quad_perm:[1,0,3,2]") PIGS_QUAD6("quad_perm:[2,3,0,1]") "s_nop 1"
                     : "+v"(z[0]), "+v"(z[1]), "+v"(z[2]), "+v"(z[3]), "+v"(z[4]), "+v"(z[5]));
    else
        asm volatile("s_nop 1\n\t" PIGS_QUAD6("quad_perm:[1,0,3,2]") PIGS_QUAD1("quad_perm:[1,0,3,2]", "%6")
                     PIGS_QUAD6("quad_perm:[2,3,0,1]") PIGS_QUAD1("quad_perm:[2,3,0,1]", "%6") "s_nop 1"
                     : "+v"(z[0]), "+v"(z[1]), "+v"(z[2]), "+v"(z[3]), "+v"(z[4]), "+v"(z[5]), "+v"(z[6]));
}

// rows: a multiple of 4 (split_step<4> pads the lists with the all-zero record; the sums of such rows
// land behind the lists' ends in the table and are never read)
template <int C, int MASK>      // MASK: the mask of the arithmetic (a residual's: ORDR_AS); list rows r0 .. r0 + rows - 1
__device__ __forceinline__ void backward_rows(const float* s, const Gsym<float, 2, C, MASK>& G,
                                              TileLdsBwd<BwdLayout<2, C>::N>& lds, int r0, int rows, int lane) {
    using BL = BwdLayout<2, C>;
    constexpr int NV = BL::N;
    constexpr int S = TileLdsBwd<NV>::S;
    const char* base = (const char*)&lds.t.rec[0][0];
    const int g = lane >> 4;
    const uint16_t* lst = lds.t.list[g];
    const int bank = (lane >> 2) & 3;
    const int sigma = ((bank & 1) << 1) | (bank >> 1);      // {0, 2, 1, 3}: the list row whose sums this lane's bank ends up with
    const bool leader = (lane & 3) == 0;
    for (int k0 = 0; k0 < rows; k0 += 4) {
        float part[4][NV];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t off = lst[r0 + k0 + u];
            const Rec r = make_rec(*(const float4*)(base + off), *(const float4*)(base + off + 16));
#pragma unroll
            for (int q = 0; q < NV; ++q) part[u][q] = 0.f;
            bwd_accumulate<float, 2, C, MASK, (MASK & ORD3) != 0, C == 1>(part[u], s, r.mu, r.con, r.v, G);
        }
        float z[8];
#pragma unroll
        for (int q = 0; q + 1 < NV; q += 2)
            fold4_pair(z[q], z[q + 1], part[0][q], part[1][q], part[2][q], part[3][q], part[0][q + 1], part[1][q + 1],
                       part[2][q + 1], part[3][q + 1]);
        if constexpr (NV & 1) {
            fold4_single(z[NV - 1], part[0][NV - 1], part[1][NV - 1], part[2][NV - 1], part[3][NV - 1]);
            z[NV] = 0.f;
        }
        quad_sums<NV>(z);
        if (leader) {
            float2* dst = (float2*)lds.sums[g][k0 + sigma];
#pragma unroll
            for (int q = 0; q < S; q += 2) dst[q / 2] = make_float2(z[q], z[q + 1]);
        }
    }
}

// Tiles that run at the same time should not be neighbours in the domain: neighbouring tiles share
// most of their Gaussians, their waves start together and move in step, and their atomics then meet
// on the same cache lines at the same moment (same-line atomics retire one every ~10 ns; measured
// 82 -> 67 us at C3).  The tiles are shuffled inside the XCD chunks of 1024 tiles (65.5 us; over the
// whole domain 66.9: here the lines stay in one L2): a multiplication by an odd number is a bijection
// on [0, 1024); the tiles behind the last whole chunk keep their places.
__device__ __forceinline__ uint32_t spread_tile(uint32_t t, uint32_t ntiles) {
    if (t >= ntiles) return t;           // the launch's padding: stays outside
    const uint32_t base = t & ~1023u;
    if (base + 1024u > ntiles) return t;
    return base + ((t & 1023u) * 37u & 1023u);
}

template <int C, int MASK>
constexpr int bwd_waves() {
    // c = 2: the sums table has 8 floats per row (NV = 7), 47.7 KB of LDS per workgroup -> 3 workgroups per
    // CU whatever the registers allow, so every c = 2 variant asks for 3 waves (168 VGPRs: no spills in
    // the widest gradient sets either); c = 1 with order 3 the same for its registers
    // (the general residual, c = 1: one wave less than its siblings 7 / 19 / ORDR, which fit 6 waves' 80 VGPRs only with
    // two registers in scratch memory; at 5 waves it has none)
    if (MASK == ORDG && C == 1) return PIGS_BWD_WAVES - 1;
    return (C == 2 || MASK == 15) ? 3 : (MASK == 7 || MASK == 19 || MASK == ORDR || MASK == 1 || MASK == 2) ? PIGS_BWD_WAVES : 4;
}
// this lane's point of a tile and the gradients that arrive at it (lanes behind the last point: zero)
template <int C, int MASK>
__device__ __forceinline__ void load_tile_point(const SamplesView& sv, uint32_t tile, int lane, const float* __restrict__ G0p,
                                                const float* __restrict__ G1p, const float* __restrict__ G2p,
                                                const float* __restrict__ G3p, const RzOf<float, MASK>& rz, SPoint& sp, bool& valid,
                                                Gsym<float, 2, C, bwd_mask_of(MASK)>& G,
                                                const float4* __restrict__ stage = nullptr) {
    const uint32_t m = tile * TILE_POINTS + (uint32_t)lane;
    valid = m < sv.M;
    sp = tile_point(sv, point_order(sv), tile, (uint32_t)lane);
    if constexpr (C == 1 && (MASK == 7 || MASK == 19)) {
        if (stage) {        // the incoming gradients of this point as one record (gradients_to_stage_kernel)
            const float4 a = stage[2 * (size_t)sp.m];
            G.g0[0] = a.x; G.g1[0][0] = a.y; G.g1[1][0] = a.z;
            if constexpr (MASK == 7) {
                const float4 b = stage[2 * (size_t)sp.m + 1];
                G.g2[0][0] = a.w; G.g2[1][0] = b.x; G.g2[2][0] = b.y;
            } else {
                G.g2[0][0] = a.w; G.g2[1][0] = 0.f; G.g2[2][0] = a.w;
            }
        } else {
            G.load((int64_t)sp.m, G0p, G1p, G2p, G3p);
        }
    } else if constexpr (MASK == ORDR) G.load_residual((int64_t)sp.m, G0p, rz);
    else if constexpr (MASK == ORDG) G.load_terms((int64_t)sp.m, G0p, rz);
    else if constexpr (MASK == ORDV) G.load_vorticity((int64_t)sp.m, G0p);
    else if constexpr (MASK == ORDC) G.load_coupled((int64_t)sp.m, G0p, rz);
    else if constexpr (MASK == ORDN) G.load_vorticity_residual((int64_t)sp.m, G0p, rz);
    else if constexpr (MASK == ORDF) G.load_vorticity_fit((int64_t)sp.m, G0p, rz);
    else G.load((int64_t)sp.m, G0p, G1p, G2p, G3p);
    if (!valid) {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            G.g0[ch] = 0.f;
            G.g1[0][ch] = G.g1[1][ch] = 0.f;
            G.g2[0][ch] = G.g2[1][ch] = G.g2[2][ch] = 0.f;
            G.g3[0][ch] = G.g3[1][ch] = G.g3[2][ch] = G.g3[3][ch] = 0.f;
        }
    }
}

// After a half of a step's rows: this lane's entry adds its rows of the sums table (those whose list position lies in
// the half that starts at r0).
template <int NV>
__device__ __forceinline__ void collect_rows(const TileLdsBwd<NV>& lds, uint32_t gm, const int* rank, int r0, float* esum) {
    constexpr int S = TileLdsBwd<NV>::S;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int rr = rank[g] - r0;
        if ((gm >> g & 1u) && rr >= 0 && rr < BWD_HALF) {
            const float2* src = (const float2*)lds.sums[g][rr];
#pragma unroll
            for (int q = 0; q < S; q += 2) {
                const float2 v = src[q / 2];
                esum[q] += v.x; esum[q + 1] += v.y;
            }
        }
    }
}
// The end of a step: every entry's sums leave as atomics into gacc[j][8] (one 32-byte row per sorted Gaussian).  Float
// atomics execute at the memory side, one request per 64-byte segment an instruction touches (MI355X_MICROARCH.md,
// Global float atomics: full rate for 256 contiguous bytes, lanes in different rows up to 17x slower), and the entries
// of a step come in runs of consecutive sorted indices (the list build walks contiguous record ranges).  So an
// instruction takes EIGHT consecutive entries, lane = (entry, value): eight 32-byte rows, mostly adjacent -- ~2.4x
// fewer segment requests than one instruction per value over all the entries of the step (which touched every run
// once per value: round 3, gacc[8][N]).  A lane fetches its (entry, value) from the entry's lane by shuffles.
template <int NV>
__device__ __forceinline__ void flush_entries(const PlanView& pv, uint32_t gm, uint32_t idx, const float* esum, int lane) {
    const uint64_t live = __ballot((gm & 15u) != 0u);
    const int q = lane & 7, sub = lane >> 3;
#pragma unroll 2
    for (int j = 0; j < BWD_STEP / 8; ++j) {
        if (((live >> (8 * j)) & 0xffull) == 0ull) continue;           // wave-uniform: none of these eight entries reaches the tile
        const int e = 8 * j + sub;
        const uint32_t ie = (uint32_t)__shfl((int)idx, e);
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const float t = __shfl(esum[k], e);
            v = q == k ? t : v;
        }
        if ((live >> e & 1ull) && q < NV) atomicAdd(&pv.gacc[(size_t)ie * 8 + q], v);
    }
}

// one tile through its own lists (tile list / group lists / record ranges)
template <int C, int MASK>
__device__ __forceinline__ void backward_tile(const PlanView& pv, const SamplesView& sv, uint32_t tile,
                                              TileLdsBwd<BwdLayout<2, C>::N>& lds, int lane, const float* __restrict__ G0p,
                                              const float* __restrict__ G1p, const float* __restrict__ G2p,
                                              const float* __restrict__ G3p, const RzOf<float, MASK>& rz) {
    constexpr int EM = bwd_mask_of(MASK);      // a residual's backward = orders 0, 1, trace
    using BL = BwdLayout<2, C>;
    constexpr int NV = BL::N;
    constexpr int S = TileLdsBwd<NV>::S;
    SPoint sp;
    bool valid;
    Gsym<float, 2, C, EM> G;
    load_tile_point<C, MASK>(sv, tile, lane, G0p, G1p, G2p, G3p, rz, sp, valid, G, pv.stage);
    const float s[2] = {sp.x, sp.y};
    if (lane < 2) lds.t.rec[BWD_STEP][lane] = make_float4(0.f, 0.f, 0.f, 0.f);
    // A tile that fell back to record ranges has no masks: they are found entry by entry against the
    // boxes of its four groups (a range holds every Gaussian NEAR the tile; few reach a given group when
    // the tile's points are scattered, which is when lists overflow).  Built only when the walk meets
    // such a tile, and outside `step`.
    // gradients that arrive at second / third derivatives (or the trace) use the plan's wide cut-off (plan.h)
    constexpr bool WIDE = (EM & (ORD2 | ORD3 | ORD2T)) != 0;
    auto ranges_mask = [&]() {
        const float INF = __builtin_huge_valf();
        const float q_cut = WIDE ? pv.params->q_b : pv.params->q_f;
        float x0 = valid ? sp.x : INF, x1 = valid ? sp.x : -INF, y0 = valid ? sp.y : INF, y1 = valid ? sp.y : -INF;
        row_box_dpp(x0, x1, y0, y1);
        float4 b0 = make_float4(readlane_f(x0, 0), readlane_f(y0, 0), readlane_f(x1, 0), readlane_f(y1, 0));
        float4 b1 = make_float4(readlane_f(x0, 16), readlane_f(y0, 16), readlane_f(x1, 16), readlane_f(y1, 16));
        float4 b2 = make_float4(readlane_f(x0, 32), readlane_f(y0, 32), readlane_f(x1, 32), readlane_f(y1, 32));
        float4 b3 = make_float4(readlane_f(x0, 48), readlane_f(y0, 48), readlane_f(x1, 48), readlane_f(y1, 48));
        return [=, &pv](uint32_t idx, bool have) -> uint32_t {
            const float4 A = pv.rec[2 * idx], B = pv.rec[2 * idx + 1];
            const Ellipse e = ellipse_of(A, B.x);
            const float4 bx[4] = {b0, b1, b2, b3};
            uint32_t gm = 0u;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (have && bx[g].x <= bx[g].z && ellipse_reaches_rect(e, bx[g].x, bx[g].y, bx[g].z, bx[g].w, q_cut)) gm |= 1u << g;
            return gm;
        };
    };
    if ((pv.hdr[(size_t)tile * TILE_HDR_WORDS] >> TILE_MODE_SHIFT) == TILE_MODE_POINTS) return;      // the helper workgroups' (backward_points_helper)
    for_each_step<BWD_STEP, WIDE>(pv, tile, lane, [&](uint32_t idx, uint32_t gm, bool have) {
        const float4 A = pv.rec[2 * idx], B = pv.rec[2 * idx + 1];
        wave_lds_fence();
        if (lane < BWD_STEP) {
            lds.t.rec[lane][0] = A;
            lds.t.rec[lane][1] = B;
        }
        int rank[4];
        const int rows = split_step<4>(lds.t, gm, lane, rank);
        wave_lds_fence();
        float esum[S];                        // this lane's entry: the sums of its rows of the table
#pragma unroll
        for (int q = 0; q < S; ++q) esum[q] = 0.f;
        for (int r0 = 0; r0 < rows; r0 += BWD_HALF) {        // (wave-uniform: at most two halves)
            backward_rows<C, EM>(s, G, lds, r0, rows - r0 < BWD_HALF ? rows - r0 : BWD_HALF, lane);
            wave_lds_fence();
            collect_rows<NV>(lds, have ? gm : 0u, rank, r0, esum);
            wave_lds_fence();
        }
        flush_entries<NV>(pv, have ? gm : 0u, idx, esum, lane);
    }, ranges_mask);
}

// helper workgroups of the backward (plan.h, TILE_MODE_POINTS): four points at a time, 16 lanes per point, lane =
// candidate.  No two lanes share a (point, Gaussian) pair, so there is nothing to reduce: NV atomics per pair
// (such tiles are few, their points meet few Gaussians).
template <int C, int MASK>
__device__ __forceinline__ void backward_points_helper(const PlanView& pv, const SamplesView& sv, uint32_t hw, uint32_t nhw, int lane,
                                                       const float* __restrict__ G0p, const float* __restrict__ G1p,
                                                       const float* __restrict__ G2p, const float* __restrict__ G3p,
                                                       const RzOf<float, MASK>& rz) {
    constexpr int EM = bwd_mask_of(MASK);
    constexpr int NV = BwdLayout<2, C>::N;
    constexpr bool WIDE = (EM & (ORD2 | ORD3 | ORD2T)) != 0;
    const uint32_t n = pv.params->n_points;
    if (n == 0u) return;
    const float q_cut = WIDE ? pv.params->q_b : pv.params->q_f;
    const int row = lane >> 4, i = lane & 15;
    for (uint32_t qd = hw; qd < n * 16u; qd += nhw) {
        const uint32_t m = pv.ptiles[qd >> 4] * TILE_POINTS + (qd & 15u) * 4u + (uint32_t)row;
        const bool valid = m < sv.M;
        const SPoint sp = tile_point(sv, point_order(sv), pv.ptiles[qd >> 4], (qd & 15u) * 4u + (uint32_t)row);
        const float s[2] = {sp.x, sp.y};
        Gsym<float, 2, C, EM> G;
        if constexpr (MASK == ORDR) G.load_residual((int64_t)sp.m, G0p, rz);
        else if constexpr (MASK == ORDG) G.load_terms((int64_t)sp.m, G0p, rz);
        else if constexpr (MASK == ORDV) G.load_vorticity((int64_t)sp.m, G0p);
        else if constexpr (MASK == ORDC) G.load_coupled((int64_t)sp.m, G0p, rz);
        else if constexpr (MASK == ORDN) G.load_vorticity_residual((int64_t)sp.m, G0p, rz);
        else if constexpr (MASK == ORDF) G.load_vorticity_fit((int64_t)sp.m, G0p, rz);
        else G.load((int64_t)sp.m, G0p, G1p, G2p, G3p);
        // The walk in step over the whole wave (round 4): every lane meets its own (point, Gaussian) pair, and a pair's
        // NV sums leave as ONE atomic request -- lane = (pair, value), eight pairs per instruction, each a pair's 32-byte
        // row of gacc -- where an instruction per value with 64 different Gaussians in its lanes was 64 requests, NV
        // times over (the memory side takes one request per 64-byte segment: a clamped-normal cloud's backward spent
        // ~150 of its 240 us in these tiles).
        walk_point_instep(pv, sp.x, sp.y, i, [&](bool have, uint32_t j, const float4 A, const float4 B) {
            const bool hit = have && valid && !(pair_q(A, B, sp.x, sp.y) > q_cut);
            float part[NV];
#pragma unroll
            for (int q = 0; q < NV; ++q) part[q] = 0.f;
            if (hit) {
                const Rec r = make_rec(A, B);
                bwd_accumulate<float, 2, C, EM, (EM & ORD3) != 0, C == 1>(part, s, r.mu, r.con, r.v, G);
            }
            const uint64_t hm = __ballot(hit);
            const int q = lane & 7, sub = lane >> 3;
            for (int it = 0; it < 8; ++it) {
                if (((hm >> (8 * it)) & 0xffull) == 0ull) continue;          // wave-uniform
                const int src = 8 * it + sub;
                const uint32_t js = (uint32_t)__shfl((int)j, src);
                float v = 0.f;
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const float t = __shfl(part[k], src);
                    v = q == k ? t : v;
                }
                if ((hm >> src & 1ull) && q < NV) atomicAdd(&pv.gacc[(size_t)js * 8 + q], v);
            }
        });
    }
}

template <int C, int MASK>
__global__ __launch_bounds__(256, (bwd_waves<C, MASK>())) void tile_backward_kernel(
    PlanView pv, SamplesView sv, const float* __restrict__ G0p, const float* __restrict__ G1p,
    const float* __restrict__ G2p, const float* __restrict__ G3p, RzOf<float, MASK> rz) {
    __shared__ TileLdsBwd<BwdLayout<2, C>::N> lds_all[4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nmain = (sv.ntiles + 3u) / 4u;
    static_assert(POINT_HELPER_BLOCKS % 8u == 0u, "the main workgroups keep their XCD");
    if (blockIdx.x < POINT_HELPER_BLOCKS) {        // the helpers come first in the launch (tile_forward_kernel)
        backward_points_helper<C, MASK>(pv, sv, blockIdx.x * 4u + (uint32_t)wave, POINT_HELPER_BLOCKS * 4u, lane, G0p, G1p, G2p, G3p, rz);
        return;
    }
    const uint32_t tile = spread_tile(xcd_block(nmain, blockIdx.x - POINT_HELPER_BLOCKS) * 4 + (uint32_t)wave, sv.ntiles);
    if (tile >= sv.ntiles) return;
    backward_tile<C, MASK>(pv, sv, tile, lds_all[wave], lane, G0p, G1p, G2p, G3p, rz);
}

template <int C>
__global__ __launch_bounds__(256) void plan_unpermute_kernel(PlanView pv, float* __restrict__ g_means,
                                                             float* __restrict__ g_conics,
                                                             float* __restrict__ g_values) {
    using BL = BwdLayout<2, C>;
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= pv.N) return;
    const uint32_t n = pv.g2o[j];
    float v[8];
    {
        float4* row = (float4*)(pv.gacc + (size_t)j * 8);
        const float4 lo = row[0], hi = row[1];
        v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
        row[0] = make_float4(0.f, 0.f, 0.f, 0.f);      // leave the scratch zeroed for the next backward
        row[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if constexpr (C == 1) {
        // the backward accumulates the factored sums (pair_math.h, FACTORED): finish them with the
        // Gaussian's own conic and value
        const float4 A = pv.rec[2 * j], B = pv.rec[2 * j + 1];
        const float a = A.z, b = A.w, c = B.x, val = B.y;
        const float sx = v[BL::MU + 0], sy = v[BL::MU + 1];
        v[BL::MU + 0] = val * (a * sx + b * sy);
        v[BL::MU + 1] = val * (b * sx + c * sy);
#pragma unroll
        for (int k = 0; k < 3; ++k) v[BL::CON + k] *= val;
    }
    // PIGS_BUILD_FORWARD_ONLY: the plan has no tile lists for the backward -- NaN, not a gradient with terms missing.  (The
    // host entry cannot refuse such a plan without reading the flag back, i.e. waiting for the device: measured, a
    // stream query and that read in every backward entry cost the sampler-only training step 2.5 us.)
    if (pv.params->fwd_only) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = __builtin_nanf("");
    }
    g_means[2 * n] = v[BL::MU + 0];
    g_means[2 * n + 1] = v[BL::MU + 1];
#pragma unroll
    for (int k = 0; k < 3; ++k) g_conics[3 * n + k] = v[BL::CON + k];
#pragma unroll
    for (int k = 0; k < C; ++k) g_values[(size_t)C * n + k] = v[BL::VAL + k];
}

// staging launch (PlanView::stage; as stage_to_outputs_kernel of plan_forward.h: thread = point in the CALLER's order):
// the incoming gradients as Gsym holds them: {g0, g1x, g1y, g2_xx}, {g2_xy + g2_yx, g2_yy, 0, 0} (null arrays: zero)
template <int MASK>
__global__ __launch_bounds__(256) void gradients_to_stage_kernel(float4* __restrict__ stage, uint32_t M, const float* __restrict__ G0,
                                                                 const float* __restrict__ G1, const float* __restrict__ G2) {
    const uint32_t m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const float g0 = G0 ? G0[m] : 0.f;
    const float2 g1 = G1 ? ((const float2*)G1)[m] : make_float2(0.f, 0.f);
    if constexpr (MASK == 7) {
        const float4 g2 = G2 ? ((const float4*)G2)[m] : make_float4(0.f, 0.f, 0.f, 0.f);
        stage[2 * (size_t)m] = make_float4(g0, g1.x, g1.y, g2.x);
        stage[2 * (size_t)m + 1] = make_float4(0.f + g2.y + g2.z, g2.w, 0.f, 0.f);
    } else {
        stage[2 * (size_t)m] = make_float4(g0, g1.x, g1.y, G2 ? G2[m] : 0.f);
    }
}

}  // namespace pigs
