// Binned sampler, the last launch of a plan build: the tile lists.  Included by plan.hip alone.
//
// One launch in which every wave walks the Gaussian grid once for four consecutive 64-point tiles
// and writes their lists (tile list with group masks for the backward, four group lists for the
// forward).  Build-time knobs: PIGS_LISTS_TPW, PIGS_TRAV_STEPS (grid_walk.h).
#pragma once
#include "plan_build.h"

namespace pigs {

// ------------------------------------------------------------------------------------------
// Launch 5 of a plan build: the tile lists.  One wave = LISTS_TPW consecutive tiles (4 tiles = 256
// consecutive sorted points = one 4 x 4 block of sample cells): ONE traversal of the Gaussian grid
// against the box of all of them -- the traversal is a chain of dependent loads and most of the
// kernel's instructions, so it is shared -- whose survivors (exact ellipse-vs-box test) wait in
// LDS with what the ellipse test needs of them; every 128 survivors, and at the end, each tile's
// four 16-point groups are tested against them and the accepted ones appended to the tile's list
// and group lists; entries with an empty mask are dropped.
// ------------------------------------------------------------------------------------------
constexpr int SURV_CAP = 128;
template <int TPW>
struct ListsLds {
    TravLds trav;
    float4 sa[SURV_CAP];              // survivor: {mux, muy, a, b}
    float4 sb[SURV_CAP];              //           {c, -b/c, -b/a, sorted index (bits)}
    float4 gbox[TPW * 4];       // boxes of the groups: {x0, y0, x1, y1}
    uint32_t sel[SURV_CAP];           // positions of the survivors that reach the tile in hand
};
struct ListArgs {
    PlanView pv;
    SamplesView sv;
    uint32_t* hdr;
    uint32_t* tlist;
    uint32_t* glist;
    uint32_t* ptiles;     // queue of the tiles in TILE_MODE_POINTS
    uint32_t* n_points;   //   and its length (PlanParams::n_points, zeroed by the count kernel)
    uint32_t* points_wanted;   // PlanParams::points_wanted
    float q_f;            // the narrow cut-off (pv.q_max is the wide one)
    const float* parea;   // per strip: box area / domain area (written by the build's Gaussian pass)
    float* strip_cover;   //   their sum (PlanParams::strip_cover)
    // The guard of a TRUSTED build (plan.hip, run_build; null: none -- every other build).  Nobody looked at the points in
    // front of this launch: they are taken in index-tiled order because point sets of this size have long been the same
    // lattice.  The lists are right whatever the points are (they come from the groups' real boxes); what may have failed
    // is the compactness of the order, and this launch has every tile's real box: a tile wider or higher than twice its
    // share of the remembered box -- lattice_compact's own bound (plan_build.h), per tile -- sets PlanParams::
    // lattice_broken, which rides home with the plan's statistics.  guard_n = points along x / y, guard_e = 16 x the
    // remembered box's extents, with 1/1000 to spare: the decision launch bounds a tile's extent by 7 (along + across)
    // rounded neighbour steps, this one takes the difference of two coordinates, and a lattice that one accepts on the
    // same box must never trip the other.
    uint32_t* lattice_broken;
    float guard_n[2], guard_e[2];
};

// the lists of the TPW tiles from tile0 (one wave).  TPW = 4 (a 4 x 4 block of sample cells: the traversal of the grid is
// shared by four tiles) where the launch fills the chip; TPW = 1 for small point sets (LISTS_SMALL_TILES): the launch's
// time is the serial life of ONE wave there (21 us at 65 536 points with four tiles per wave, the chip nearly idle), and
// a wave with a quarter of the work has a shorter life.
// FWD_ONLY (PIGS_BUILD_FORWARD_ONLY; pv.q_max == q_f then): the forward reads the group lists alone, so the tile list
// and its wide masks are not written, one cut-off is tested per group, and a tile whose group lists fit is LIST with a
// count of zero (no tile list a backward could read; there is no TILE_MODE_GROUPS rebuild either).
template <int TPW, bool STRIPS = false, bool FWD_ONLY = false>
__device__ __forceinline__ void build_block_lists(const ListArgs& a, ListsLds<TPW>& lds, uint32_t tile0, int lane) {
    const PlanView& pv = a.pv;
    const uint32_t ntiles = a.sv.ntiles;
    const GaussGrid gg = pv.params->gg;
    const uint32_t level_mask = pv.params->level_mask;
    constexpr bool strips = STRIPS;                       // candidates from strip boxes, not from grid cells (PlanParams::strips)
    const uint32_t loff = pv.params->level_off[lane < PLAN_MAX_LEVELS ? lane : 0];   // lane = level: its first counter
    const float INF = __builtin_huge_valf();
    SPoint sp[TPW];
    bool valid[TPW];
    const PointOrder po = point_order(a.sv);
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const uint32_t m = (tile0 + (uint32_t)t) * TILE_POINTS + (uint32_t)lane;
        valid[t] = m < a.sv.M;           // also false for every point of a tile behind the last one
        sp[t] = SPoint{0.f, 0.f, 0u};
        if (tile0 + (uint32_t)t < ntiles) sp[t] = tile_point(a.sv, po, tile0 + (uint32_t)t, (uint32_t)lane);     // wave-uniform
    }
    float bx0 = INF, bx1 = -INF, by0 = INF, by1 = -INF;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        float x0 = valid[t] ? sp[t].x : INF, x1 = valid[t] ? sp[t].x : -INF;
        float y0 = valid[t] ? sp[t].y : INF, y1 = valid[t] ? sp[t].y : -INF;
        row_box_dpp(x0, x1, y0, y1);
        if ((lane & 15) == 0) lds.gbox[t * 4 + (lane >> 4)] = make_float4(x0, y0, x1, y1);
        bx0 = fminf(bx0, x0); bx1 = fmaxf(bx1, x1); by0 = fminf(by0, y0); by1 = fmaxf(by1, y1);
    }
    wave_box_from_rows_dpp(bx0, bx1, by0, by1);

    const uint32_t cap = pv.list_cap;
    // what a per-point walk would meet: 9 cells of every level at the level's mean occupancy (wave-uniform;
    // all lanes call it together)
    auto walk_candidates = [&]() -> float {
        float e = 0.f;
        if (lane < pv.L) {
            const float cells = (float)(pv.G0 >> lane) * (float)(pv.G0 >> lane);
            e = 9.f * (float)(pv.starts[pv.level_off[lane + 1]] - pv.starts[pv.level_off[lane]]) / cells;
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) e += __shfl_xor(e, o);      // levels live in lanes 0..11
        return __shfl(e, 0);
    };
    // A block of 256 points spread over more than POINTS_MODE_BLOCK_CELLS finest Gaussian cells (a group of 16 then
    // spans dozens of cells: its list would run to hundreds) goes to the per-point walk without being listed at
    // all: the traversal of such a box is the list build's own tail (thousands of candidates in one wave).
    if (strips && (bx1 - bx0) * gg.inv_s0 * ((by1 - by0) * gg.inv_s0) > POINTS_MODE_BLOCK_CELLS) {
        // far-apart points: the cells would have sent this block to the per-point walk -- say so (PlanParams::points_wanted)
        if (lane == 0) atomicAdd(a.points_wanted, 1u);
    }
    if (!strips && (bx1 - bx0) * gg.inv_s0 * ((by1 - by0) * gg.inv_s0) > POINTS_MODE_BLOCK_CELLS && walk_candidates() <= 4.f * (float)cap) {
        for (int t = 0; t < TPW; ++t) {
            if (tile0 + (uint32_t)t >= ntiles) break;
            if (lane < TILE_HDR_WORDS)
                a.hdr[(size_t)(tile0 + (uint32_t)t) * TILE_HDR_WORDS + lane] = lane == 0 ? (TILE_MODE_POINTS << TILE_MODE_SHIFT) : 0u;
            if (lane == 0) a.ptiles[atomicAdd(a.n_points, 1u)] = tile0 + (uint32_t)t;
        }
        return;
    }
    uint32_t n[TPW], ng[TPW][4];
    bool overflow[TPW], goverflow[TPW];       // the tile list / one of the group lists is full
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        n[t] = 0; overflow[t] = false; goverflow[t] = false;
#pragma unroll
        for (int g = 0; g < 4; ++g) ng[t][g] = 0;
    }
    int sn = 0;
    // the tiles' tests on the survivors in LDS: per tile, (A) the survivors that reach the tile's
    // box, compacted (their positions, one byte each would do: 128 survivors), then (B) the four
    // group tests on those: usually one step of 64 instead of two
    auto flush = [&]() __attribute__((always_inline)) {
        wave_lds_fence();
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            if (tile0 + (uint32_t)t >= ntiles) continue;
            float4 gb[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) gb[g] = lds.gbox[t * 4 + g];
            const float tx0 = fminf(fminf(gb[0].x, gb[1].x), fminf(gb[2].x, gb[3].x));
            const float ty0 = fminf(fminf(gb[0].y, gb[1].y), fminf(gb[2].y, gb[3].y));
            const float tx1 = fmaxf(fmaxf(gb[0].z, gb[1].z), fmaxf(gb[2].z, gb[3].z));
            const float ty1 = fmaxf(fmaxf(gb[0].w, gb[1].w), fmaxf(gb[2].w, gb[3].w));
            int sel = 0;
            for (int s0 = 0; s0 < sn; s0 += 64) {
                const int k = s0 + lane < sn ? s0 + lane : 0;
                const float4 A = lds.sa[k], B = lds.sb[k];
                Ellipse e;
                e.x = A.x; e.y = A.y; e.a = A.z; e.b = A.w; e.c = B.x; e.nb_c = B.y; e.nb_a = B.z;
                const bool hit = s0 + lane < sn && ellipse_reaches_rect(e, tx0, ty0, tx1, ty1, pv.q_max);
                const uint64_t hm = __ballot(hit);
                if (hit) lds.sel[sel + lanes_below(hm)] = (uint32_t)k;
                sel += __builtin_popcountll(hm);
            }
            wave_lds_fence();
            uint32_t* tl = a.tlist + (size_t)(tile0 + (uint32_t)t) * cap;
            uint32_t* gl = a.glist + (size_t)(tile0 + (uint32_t)t) * 4 * cap;
            for (int s0 = 0; s0 < sel; s0 += 64) {
                const int k = (int)lds.sel[s0 + lane < sel ? s0 + lane : 0];
                const float4 A = lds.sa[k], B = lds.sb[k];
                Ellipse e;
                e.x = A.x; e.y = A.y; e.a = A.z; e.b = A.w; e.c = B.x; e.nb_c = B.y; e.nb_a = B.z;
                const uint32_t j = __builtin_bit_cast(uint32_t, B.w);
                uint32_t gm = 0, gf = 0;       // wide (tile list, backward) and narrow (group lists, forward) masks
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    // a group without a point (the ragged last tile) has an inverted box: never needed
                    const float qmin = ellipse_min_q_rect(e, gb[g].x, gb[g].y, gb[g].z, gb[g].w);
                    if (gb[g].x <= gb[g].z) {
                        if (!FWD_ONLY && !(qmin > pv.q_max)) gm |= 1u << g;
                        if (!(qmin > a.q_f)) gf |= 1u << g;
                    }
                }
                if (s0 + lane >= sel) gm = gf = 0u;
                if constexpr (!FWD_ONLY) {
                    const uint64_t km = __ballot(gm != 0u);
                    const uint32_t cnt = (uint32_t)__builtin_popcountll(km);
                    if (n[t] + cnt <= cap) {
                        if (gm != 0u) tl[n[t] + (uint32_t)lanes_below(km)] = j | (gm << LIST_WIDE_SHIFT) | (gf << LIST_NARROW_SHIFT);
                    } else {
                        overflow[t] = true;
                    }
                    n[t] += cnt;
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const uint64_t mg = __ballot(gf >> g & 1u);
                    const uint32_t cg = (uint32_t)__builtin_popcountll(mg);
                    if (ng[t][g] + cg <= cap) {
                        if (gf >> g & 1u) gl[g * cap + ng[t][g] + (uint32_t)lanes_below(mg)] = j;
                    } else {
                        goverflow[t] = true;
                    }
                    ng[t][g] += cg;
                }
            }
            wave_lds_fence();
        }
        sn = 0;
    };
    auto walk_rect = [&](float x0, float y0, float x1, float y1, bool walk, auto&& rows, auto&& batch) __attribute__((always_inline)) {
        if constexpr (STRIPS) traverse_strips(pv, x0, y0, x1, y1, lane, lds.trav, walk, rows, batch);
        else traverse(pv, gg, level_mask, loff, x0, y0, x1, y1, lane, lds.trav, walk, rows, batch);
    };
    walk_rect(bx0, by0, bx1, by1, true,
             [](int, uint32_t, uint32_t) {},
             [&](const float4 A, const float4 B, uint64_t mask, uint32_t j) __attribute__((always_inline)) {
        // The survivors wait until the buffer cannot take the batch in hand (round 4: it used to be flushed as soon as
        // a FULL batch might not fit any more, i.e. from 65 on -- a block's ~100 survivors then went through the per-tile
        // filter and the group tests in two portions, twice the steps of one; a walk that finds them in batches of ~25,
        // four strips of 16 candidates, more often still).
        const int add = __builtin_popcountll(mask);
        if (sn + add > SURV_CAP) flush();
        if (mask >> lane & 1ull) {
            const Ellipse e = ellipse_of(A, B.x);
            const int k = sn + lanes_below(mask);
            lds.sa[k] = A;
            lds.sb[k] = make_float4(B.x, e.nb_c, e.nb_a, __builtin_bit_cast(float, j));
        }
        sn += add;
    });
    if (sn > 0) flush();

    // A tile list that does not fit while the four group lists do (64 scattered points of a sparse
    // region share few Gaussians: up to 4 x cap distinct ones) is no reason to give the lists up: the
    // forward reads the group lists only, and the backward walks them as four single-group lists
    // (TILE_MODE_GROUPS) -- which must then hold the WIDE set: they are rebuilt below.
    const bool two_cuts = !FWD_ONLY && pv.q_max > a.q_f;
    bool any_rare = false;
    bool rebuild[TPW];
    const bool guard = a.lattice_broken != nullptr;       // launch-uniform
    if (guard) wave_lds_fence();                          // (the group boxes: no flush may have run)
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        rebuild[t] = false;
        if (tile0 + (uint32_t)t >= ntiles) { overflow[t] = false; continue; }
        if (guard) {      // the trusted build's guard (ListArgs::lattice_broken); a comparison that NaN or inf fails: broken
            float4 gb[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) gb[g] = lds.gbox[t * 4 + g];
            const float wx = fmaxf(fmaxf(gb[0].z, gb[1].z), fmaxf(gb[2].z, gb[3].z)) - fminf(fminf(gb[0].x, gb[1].x), fminf(gb[2].x, gb[3].x));
            const float wy = fmaxf(fmaxf(gb[0].w, gb[1].w), fmaxf(gb[2].w, gb[3].w)) - fminf(fminf(gb[0].y, gb[1].y), fminf(gb[2].y, gb[3].y));
            if (!(wx * a.guard_n[0] <= a.guard_e[0] && wy * a.guard_n[1] <= a.guard_e[1]) && lane == 0) *a.lattice_broken = 1u;
        }
        const bool tl_over = FWD_ONLY ? goverflow[t] : overflow[t];      // (no tile list: its group lists decide)
        overflow[t] = tl_over && goverflow[t];            // from here on: the tile needs the ranges fallback
        rebuild[t] = tl_over && !goverflow[t] && two_cuts;
        // spread-out points with long lists: the per-point walk is cheaper than the lists (plan.h)
        uint32_t longest = ng[t][0] > ng[t][1] ? ng[t][0] : ng[t][1];
        longest = ng[t][2] > longest ? ng[t][2] : longest;
        longest = ng[t][3] > longest ? ng[t][3] : longest;
        if (longest > POINTS_MODE_MIN_LIST) {      // (strips: the per-point walk needs the grid -- only noted)
            float4 gb[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) gb[g] = lds.gbox[t * 4 + g];
            const float wx = fmaxf(fmaxf(gb[0].z, gb[1].z), fmaxf(gb[2].z, gb[3].z)) - fminf(fminf(gb[0].x, gb[1].x), fminf(gb[2].x, gb[3].x));
            const float wy = fmaxf(fmaxf(gb[0].w, gb[1].w), fmaxf(gb[2].w, gb[3].w)) - fminf(fminf(gb[0].y, gb[1].y), fminf(gb[2].y, gb[3].y));
            if (strips && wx * gg.inv_s0 * (wy * gg.inv_s0) > POINTS_MODE_MIN_CELLS) {
                if (lane == 0) atomicAdd(a.points_wanted, 1u);
            }
            if (!strips && wx * gg.inv_s0 * (wy * gg.inv_s0) > POINTS_MODE_MIN_CELLS && walk_candidates() <= 4.f * (float)(longest < cap ? longest : cap)) {
                overflow[t] = false; rebuild[t] = false;
                if (lane < 5)
                    a.hdr[(size_t)(tile0 + (uint32_t)t) * TILE_HDR_WORDS + lane] = lane == 0 ? (TILE_MODE_POINTS << TILE_MODE_SHIFT) : 0u;
                if (lane == 0) a.ptiles[atomicAdd(a.n_points, 1u)] = tile0 + (uint32_t)t;
                continue;
            }
        }
        any_rare |= overflow[t] || rebuild[t];
        if (!overflow[t] && !rebuild[t] && lane < TILE_HDR_WORDS) {
            const bool fits = n[t] <= cap;
            uint32_t w = 0;
            if (lane == 0) w = fits ? ((n[t] & TILE_COUNT_MASK) | (TILE_MODE_LIST << TILE_MODE_SHIFT)) : (TILE_MODE_GROUPS << TILE_MODE_SHIFT);
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (lane == 1 + g) w = ng[t][g];
            if (lane < 5) a.hdr[(size_t)(tile0 + (uint32_t)t) * TILE_HDR_WORDS + lane] = w;      // words 5..7: the block's
        }
    }
    if (!any_rare) return;
    // Rare paths, one tile at a time, not unrolled.  (1) group-lists-only tile under two cut-offs: its
    // group lists are rebuilt from a walk of the grid around ITS box with the wide cut-off (the forward
    // then evaluates a few pairs more than q_f asks for in such a tile: harmless).  (2) a group list does
    // not fit: the tile keeps the grid's record ranges around its box instead (pairs {first, length}; the
    // sampling kernels test the ranges' records against the group boxes themselves); when even those do
    // not fit, the single range of all Gaussians.
    for (int t = 0; t < TPW; ++t) {
        const bool mine_rebuild = __builtin_amdgcn_readfirstlane((int)(t == 0   ? rebuild[0]
                                                                       : t == 1 ? rebuild[TPW > 1 ? 1 : 0]
                                                                       : t == 2 ? rebuild[TPW > 2 ? 2 : 0]
                                                                                : rebuild[TPW > 3 ? 3 : 0])) != 0;
        bool mine = __builtin_amdgcn_readfirstlane((int)(t == 0   ? overflow[0]
                                                         : t == 1 ? overflow[TPW > 1 ? 1 : 0]
                                                         : t == 2 ? overflow[TPW > 2 ? 2 : 0]
                                                                  : overflow[TPW > 3 ? 3 : 0])) != 0;
        if (!mine && !mine_rebuild) continue;
        float4 gb[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) gb[g] = lds.gbox[t * 4 + g];
        const float tx0 = fminf(fminf(gb[0].x, gb[1].x), fminf(gb[2].x, gb[3].x));
        const float ty0 = fminf(fminf(gb[0].y, gb[1].y), fminf(gb[2].y, gb[3].y));
        const float tx1 = fmaxf(fmaxf(gb[0].z, gb[1].z), fmaxf(gb[2].z, gb[3].z));
        const float ty1 = fmaxf(fmaxf(gb[0].w, gb[1].w), fmaxf(gb[2].w, gb[3].w));
        uint32_t* tl = a.tlist + (size_t)(tile0 + (uint32_t)t) * cap;
        if (mine_rebuild) {
            uint32_t* gl = a.glist + (size_t)(tile0 + (uint32_t)t) * 4 * cap;
            uint32_t ngw[4] = {0u, 0u, 0u, 0u};
            bool gover = false;
            walk_rect(tx0, ty0, tx1, ty1, true,
                     [](int, uint32_t, uint32_t) {},
                     [&](const float4 A, const float4 B, uint64_t mask, uint32_t j) __attribute__((always_inline)) {
                const bool have = mask >> lane & 1ull;
                const Ellipse e = ellipse_of(A, B.x);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const bool hit = have && gb[g].x <= gb[g].z &&
                                     !(ellipse_min_q_rect(e, gb[g].x, gb[g].y, gb[g].z, gb[g].w) > pv.q_max);
                    const uint64_t mg = __ballot(hit);
                    const uint32_t cg = (uint32_t)__builtin_popcountll(mg);
                    if (ngw[g] + cg <= cap) {
                        if (hit) gl[g * cap + ngw[g] + (uint32_t)lanes_below(mg)] = j;
                    } else {
                        gover = true;
                    }
                    ngw[g] += cg;
                }
            });
            if (!gover) {
                if (lane < 5) {
                    uint32_t w = 0;
                    if (lane == 0) w = TILE_MODE_GROUPS << TILE_MODE_SHIFT;
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (lane == 1 + g) w = ngw[g];
                    a.hdr[(size_t)(tile0 + (uint32_t)t) * TILE_HDR_WORDS + lane] = w;
                }
                continue;
            }
            mine = true;          // the wide group lists do not fit either: ranges
        }
        // scattered points (a box of many Gaussian cells for 64 points): no lists, every lane walks the grid
        // around its own point at sampling time (plan.h, TILE_MODE_POINTS)
        if (!strips && (tx1 - tx0) * gg.inv_s0 * ((ty1 - ty0) * gg.inv_s0) > POINTS_MODE_MIN_CELLS && walk_candidates() <= 4.f * (float)cap) {
            if (lane < 5)
                a.hdr[(size_t)(tile0 + (uint32_t)t) * TILE_HDR_WORDS + lane] = lane == 0 ? (TILE_MODE_POINTS << TILE_MODE_SHIFT) : 0u;
            if (lane == 0) a.ptiles[atomicAdd(a.n_points, 1u)] = tile0 + (uint32_t)t;
            continue;
        }
        uint32_t nr = 0;
        bool fits = true;
        walk_rect(tx0, ty0, tx1, ty1, false,
                 [&](int nrow, uint32_t jb, uint32_t len) {
            const bool keep = lane < nrow && len > 0;
            const uint64_t km = __ballot(keep);
            const uint32_t cnt = (uint32_t)__builtin_popcountll(km);
            if (2 * (nr + cnt) <= cap) {
                if (keep) {
                    const uint32_t p = 2 * (nr + (uint32_t)lanes_below(km));
                    tl[p] = jb; tl[p + 1] = len;
                }
            } else {
                fits = false;
            }
            nr += cnt;
        },
                 [](const float4, const float4, uint64_t, uint32_t) {});
        if (!fits && lane == 0) { tl[0] = 0; tl[1] = pv.N; }
        const uint32_t cnt = fits ? nr : 1u;
        if (lane < 5)
            a.hdr[(size_t)(tile0 + (uint32_t)t) * TILE_HDR_WORDS + lane] = lane == 0 ? (cnt | (TILE_MODE_RANGES << TILE_MODE_SHIFT)) : 0u;
    }
}

// the same strips of the domain on the same XCD as in the sampling kernels, which then find a tile's
// lists in the L2 that wrote them (a workgroup here is 4 * TPW tiles; forward 27.05 -> 26.4 us)
template <int TPW>
__device__ __forceinline__ uint32_t lists_tile0(int wave) {
    return (xcd_block_chunk<PIGS_XCD_CHUNK / TPW>(gridDim.x) * 4 + (uint32_t)wave) * TPW;
}
// the first workgroup of a list launch: the strips' cover of the domain (PlanParams::strip_cover), summed from what the
// build's Gaussian pass left per strip
__device__ __forceinline__ void lists_strip_cover(const ListArgs& a) {
    __shared__ float cover_sh[4];
    if (blockIdx.x != 0) return;
    const uint32_t ns = (a.pv.N + STRIP - 1u) / STRIP;
    float sum = 0.f;
    for (uint32_t k = threadIdx.x; k < ns; k += 256u) sum += a.parea[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((threadIdx.x & 63u) == 0u) cover_sh[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) a.strip_cover[0] = cover_sh[0] + cover_sh[1] + cover_sh[2] + cover_sh[3];
}

template <int TPW, bool STRIPS, bool FWD_ONLY = false>
__global__ __launch_bounds__(256) void plan_lists_kernel(ListArgs a) {
    __shared__ ListsLds<TPW> lds_all[4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    lists_strip_cover(a);
    const uint32_t tile0 = lists_tile0<TPW>(wave);
    if (tile0 >= a.sv.ntiles) return;
    build_block_lists<TPW, STRIPS, FWD_ONLY>(a, lds_all[wave], tile0, lane);
}

}  // namespace pigs
