// Binned sampler, the last launch of a plan build: the tile lists.  Included by plan.hip alone.
//
// One launch in which every wave walks the Gaussian grid once for four consecutive 64-point tiles
// and writes their lists (tile list with group masks for the backward, four group lists for the
// forward).  Build-time knobs: PIGS_LISTS_TPW, PIGS_TRAV_STEPS (grid_walk.h).
#pragma once
#include "plan_build.h"

#ifndef PIGS_LISTS_PRODUCT
#define PIGS_LISTS_PRODUCT 1      // 0: no block takes the product path of the flush (as the environment word of the same name)
#endif

namespace pigs {

// ------------------------------------------------------------------------------------------
// Launch 5 of a plan build: the tile lists.  One wave = LISTS_TPW consecutive tiles (4 tiles = 256
// consecutive sorted points = one 4 x 4 block of sample cells): ONE traversal of the Gaussian grid
// against the box of all of them -- the traversal is a chain of dependent loads and most of the
// kernel's instructions, so it is shared -- whose survivors (exact ellipse-vs-box test) wait in
// LDS with what the ellipse test needs of them; every 128 survivors, and at the end, each tile's
// four 16-point groups are tested against them and the accepted ones appended to the tile's list
// and group lists; entries with an empty mask are dropped.
//
// PRODUCT BLOCKS.  On an index-tiled lattice a group is a 4 x 4 patch of the lattice, and the 4 TPW group boxes of a
// block are the product of 2 sqrt(TPW) x-intervals and as many y-intervals.  ellipse_min_q_rect splits into terms of
// one interval and terms of both (ellipse_rect.h): a block whose boxes ARE such a product -- decided from the boxes,
// bit for bit, never from the samples' header -- tests every survivor against all its groups at once: the axis terms
// of the 8 intervals, then 16 combinations; no per-tile filter, no `sel`, one read of the survivor.  Every other
// block (points in no lattice, a rotated lattice, a ragged tile) takes the general path.  Both form bit-identical
// minima for the same (ellipse, box); the product path only drops the tile pre-filter, so a (survivor, group) pair
// whose group test passes while its tile's test fails -- the group box lies inside the tile's: rounding alone, at the
// cut-off -- is listed there and not here.  PIGS_LISTS_PRODUCT=0 (-D or environment): the general path everywhere.
// ------------------------------------------------------------------------------------------
constexpr int SURV_CAP = 128;
template <int TPW>
struct ListsLds {
    TravLds trav;
    float4 sa[SURV_CAP];              // survivor: {mux, muy, a, b}
    float4 sb[SURV_CAP];              //           {c, -b/c, -b/a, sorted index (bits)}
    float4 gbox[TPW * 4];       // boxes of the groups: {x0, y0, x1, y1}
    float4 tbox[TPW];           // boxes of the tiles (written once, in the prologue)
    uint32_t sel[SURV_CAP];           // general path: positions of the survivors that reach the tile in hand
};
static_assert(4 * sizeof(ListsLds<4>) <= 32768, "five workgroups of the list launch per CU");
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
    const float* parea;   // per strip: box area / domain area (written by the build's Gaussian pass; null: this build's
    float* strip_cover;   //   statistics are not wanted home, nobody sums them) and their sum (PlanParams::strip_cover)
    // Where this build's statistics come home: the device address of the five words of a slot of the plans' memory
    // (build_choice.h, POINTS_WORDS; pinned host memory that the host zeroed before the launch), or null -- not due, a
    // capture, or they travel by a copy of the workspace header (PIGS_STATS_HOME=0).  Every word is stored where it comes
    // into being and only when it is not zero (stats_home): nothing waits for the end of the launch.  The workspace
    // words stay the kernels' own working state.
    uint32_t* home;
    uint32_t product;     // blocks whose group boxes form a product may take the product path (PIGS_LISTS_PRODUCT != 0)
    uint32_t through;     // headers and lists leave by write-through stores (plan.h, store_through; PIGS_STORE_THROUGH):
                          // read by the host alone, which launches plan_lists_kernel<..., THROUGH> by it
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

// one word of a build's statistics on its way home: a system-scope relaxed store (a plain vector store past the caches;
// the host reads the word behind the event that follows the launch)
__device__ __forceinline__ void stats_home(uint32_t* home, uint32_t word, uint32_t v) {
    __hip_atomic_store(home + word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
constexpr uint32_t HOME_N_POINTS = 0, HOME_STRIP_COVER = 1, HOME_STRIPS = 2, HOME_POINTS_WANTED = 3, HOME_LATTICE_BROKEN = 4;

// the lists of the TPW tiles from tile0 (one wave).  TPW = 4 (a 4 x 4 block of sample cells: the traversal of the grid is
// shared by four tiles) where the launch fills the chip; TPW = 1 for small point sets (LISTS_SMALL_TILES): the launch's
// time is the serial life of ONE wave there (21 us at 65 536 points with four tiles per wave, the chip nearly idle), and
// a wave with a quarter of the work has a shorter life.
// FWD_ONLY (PIGS_BUILD_FORWARD_ONLY; pv.q_max == q_f then): the forward reads the group lists alone, so the tile list
// and its wide masks are not written, one cut-off is tested per group, and a tile whose group lists fit is LIST with a
// count of zero (no tile list a backward could read; there is no TILE_MODE_GROUPS rebuild either).
// PRODUCT = false: the product path is not compiled in (the fused list + forward launch, plan_forward.h: its wave holds
// the forward's registers as well and the two paths together do not fit its 96).
// THROUGH: headers and lists leave by write-through stores (plan.h, store_through).  A template argument, not a word
// of ListArgs read in the kernel: built that way first -- a launch-uniform branch around each store, every address
// handed over as a finished pointer -- the launch was 0.3-0.7 us SLOWER than the parent's with the new stores and
// 1.8 us slower with the plain ones.  The plain instantiations are the parent's code,
// instruction for instruction.  The fused launch keeps plain stores: its waves read their own headers and lists back
// behind a workgroup-scope release.
template <int TPW, bool STRIPS = false, bool FWD_ONLY = false, bool PRODUCT = true, bool THROUGH = false>
__device__ __forceinline__ void build_block_lists(const ListArgs& a, ListsLds<TPW>& lds, uint32_t tile0, int lane) {
    const PlanView& pv = a.pv;
    const uint32_t ntiles = a.sv.ntiles;
    constexpr bool strips = STRIPS;                       // candidates from strip boxes, not from grid cells (PlanParams::strips)
    // (the strips' walk reads nothing of the grid but the finest cell size)
    GaussGrid gg{};
    uint32_t level_mask = 0u, loff = 0u;
    if constexpr (STRIPS) {
        gg.inv_s0 = pv.params->gg.inv_s0;
    } else {
        gg = pv.params->gg;
        level_mask = pv.params->level_mask;
        loff = pv.params->level_off[lane < PLAN_MAX_LEVELS ? lane : 0];   // lane = level: its first counter
    }
    const float INF = __builtin_huge_valf();
    constexpr bool through = THROUGH;
    // lane 0: a tile for the queue of TILE_MODE_POINTS tiles / a block or tile of far-apart points met by a strips build.
    // Whoever counts the first one sends the word home (a word at home says "any", not how many).
    auto queue_points_tile = [&](uint32_t tile) {
        const uint32_t k = atomicAdd(a.n_points, 1u);
        a.ptiles[k] = tile;
        if (k == 0u && a.home) stats_home(a.home, HOME_N_POINTS, 1u);
    };
    auto note_points_wanted = [&]() {
        if (a.home) {
            if (atomicAdd(a.points_wanted, 1u) == 0u) stats_home(a.home, HOME_POINTS_WANTED, 1u);
        } else {
            atomicAdd(a.points_wanted, 1u);
        }
    };
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
    float gx0[TPW], gx1[TPW], gy0[TPW], gy1[TPW];         // every lane: the box of its own group, per tile
    uint32_t has[TPW];                                    // per tile: the groups that hold a point (wave-uniform)
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        float x0 = valid[t] ? sp[t].x : INF, x1 = valid[t] ? sp[t].x : -INF;
        float y0 = valid[t] ? sp[t].y : INF, y1 = valid[t] ? sp[t].y : -INF;
        row_box_dpp(x0, x1, y0, y1);
        if ((lane & 15) == 0) lds.gbox[t * 4 + (lane >> 4)] = make_float4(x0, y0, x1, y1);
        bx0 = fminf(bx0, x0); bx1 = fmaxf(bx1, x1); by0 = fminf(by0, y0); by1 = fmaxf(by1, y1);
        gx0[t] = x0; gx1[t] = x1; gy0[t] = y0; gy1[t] = y1;
        // a group without a point (the ragged last tile) has an inverted box: never needed
        const uint64_t hm = __ballot(x0 <= x1);
        has[t] = (uint32_t)(hm & 1ull) | (uint32_t)(hm >> 15 & 2ull) | (uint32_t)(hm >> 30 & 4ull) | (uint32_t)(hm >> 45 & 8ull);
    }
    wave_box_from_rows_dpp(bx0, bx1, by0, by1);
    // the tiles' boxes, once (lane = tile): the general flush, the guard and the `longest` check read them
    wave_lds_fence();
    if (lane < TPW) {
        const float4 g0 = lds.gbox[lane * 4], g1 = lds.gbox[lane * 4 + 1], g2 = lds.gbox[lane * 4 + 2], g3 = lds.gbox[lane * 4 + 3];
        lds.tbox[lane] = make_float4(fminf(fminf(g0.x, g1.x), fminf(g2.x, g3.x)), fminf(fminf(g0.y, g1.y), fminf(g2.y, g3.y)),
                                     fmaxf(fmaxf(g0.z, g1.z), fmaxf(g2.z, g3.z)), fmaxf(fmaxf(g0.w, g1.w), fmaxf(g2.w, g3.w)));
    }
    wave_lds_fence();
    // Do the group boxes form a product?  Group g of tile t is the 4 x 4 patch (g & 1, g >> 1) of the tile
    // (lattice_index) and tiles t .. t + 3 of a block its 2 x 2 tile columns, lower tile first (lattice_tile_xy), so
    // the group sits in column 2 (t >> 1) + (g & 1) and row 2 (t & 1) + (g >> 1) of the block's groups.  A product:
    // every group holds a point, the groups of a column have bit-equal x0 and x1, those of a row bit-equal y0 and y1.
    constexpr bool CAN_PRODUCT = PRODUCT && PIGS_LISTS_PRODUCT != 0 && (TPW == 1 || TPW == 4);
    constexpr int NI = TPW == 4 ? 4 : 2;                  // intervals per axis
    bool product = false;
    if constexpr (CAN_PRODUCT) {
        auto same = [](float u, float v) { return __builtin_bit_cast(uint32_t, u) == __builtin_bit_cast(uint32_t, v); };
        bool ok = a.product != 0u;
#pragma unroll
        for (int t = 0; t < TPW; ++t) ok = ok && has[t] == 15u;
        if (__builtin_amdgcn_readfirstlane((int)ok)) {      // (wave-uniform: random points leave here)
            if constexpr (TPW == 4) {
                ok = ok && same(gx0[0], gx0[1]) && same(gx1[0], gx1[1]) && same(gx0[2], gx0[3]) && same(gx1[2], gx1[3]);
                ok = ok && same(gy0[0], gy0[2]) && same(gy1[0], gy1[2]) && same(gy0[1], gy0[3]) && same(gy1[1], gy1[3]);
            }
#pragma unroll
            for (int h = 0; h < (TPW == 4 ? 2 : 1); ++h) {   // against the group above (lane ^ 32) and the one beside (lane ^ 16)
                const int tc = 2 * h, tr = h;
                ok = ok && same(gx0[tc], __shfl_xor(gx0[tc], 32)) && same(gx1[tc], __shfl_xor(gx1[tc], 32));
                ok = ok && same(gy0[tr], __shfl_xor(gy0[tr], 16)) && same(gy1[tr], __shfl_xor(gy1[tr], 16));
            }
            product = __ballot(ok) == ~0ull;
        }
    }

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
        if (lane == 0) note_points_wanted();
    }
    if (!strips && (bx1 - bx0) * gg.inv_s0 * ((by1 - by0) * gg.inv_s0) > POINTS_MODE_BLOCK_CELLS && walk_candidates() <= 4.f * (float)cap) {
        for (int t = 0; t < TPW; ++t) {
            if (tile0 + (uint32_t)t >= ntiles) break;
            if (lane < TILE_HDR_WORDS)
                store_through(a.hdr, (size_t)(tile0 + (uint32_t)t) * TILE_HDR_WORDS + lane, lane == 0 ? (TILE_MODE_POINTS << TILE_MODE_SHIFT) : 0u, through);
            if (lane == 0) queue_points_tile(tile0 + (uint32_t)t);
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
    // one step's accepted survivors of tile t (this lane: sorted index j, wide mask gm, narrow mask gf; zero: none)
    // appended to the tile's list and its four group lists (full plans: the tile list's entries hold the masks)
    auto append = [&](int t, uint32_t j, uint32_t gm, uint32_t gf) __attribute__((always_inline)) {
        uint32_t* tl = a.tlist + (size_t)(tile0 + (uint32_t)t) * cap;
        uint32_t* gl = a.glist + (size_t)(tile0 + (uint32_t)t) * 4 * cap;
        if constexpr (!FWD_ONLY) {
            const uint64_t km = __ballot(gm != 0u);
            const uint32_t cnt = (uint32_t)__builtin_popcountll(km);
            if (n[t] + cnt <= cap) {
                if (gm != 0u) store_through(tl, n[t] + (uint32_t)lanes_below(km), j | (gm << LIST_WIDE_SHIFT) | (gf << LIST_NARROW_SHIFT), through);
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
                if (gf >> g & 1u) store_through(gl, g * cap + ng[t][g] + (uint32_t)lanes_below(mg), j, through);
            } else {
                goverflow[t] = true;
            }
            ng[t][g] += cg;
        }
    };
    // A forward-only plan writes no tile list, so nothing needs the masks: one step's accepted survivors of ONE group
    // go to list g of tile t at once.  pass: this lane's compare; have: this lane holds a survivor of this step, and
    // live: the ballot of that.  The ballot of a bare compare is the compare's own scalar result, the count comes from
    // it, the position is v_mbcnt, and one v_add_lshl joins it to the list's place in the block's lists and its running
    // count, both scalar (v_mbcnt takes the mask from a scalar register, and one instruction reads one: the addend
    // cannot ride in it): the store takes the block's base in scalar registers and a 32-bit byte offset (16 lists of
    // cap words).  Groups go to different lists, so their order among each other is free; within a list the entries
    // keep the survivors' order.  The capacity rule is append's: what would pass cap is counted and not stored.  t
    // and g are compile-time constants wherever this is called, and the counts are wave-uniform: ng stays in SGPRs.
    auto append_group = [&](int t, int g, bool pass, bool have, uint64_t live, uint32_t j) __attribute__((always_inline)) {
        uint32_t* gl = a.glist + (size_t)tile0 * 4 * cap;
        const uint64_t mg = __ballot(pass) & live;
        const uint32_t cg = (uint32_t)__builtin_popcountll(mg);
        const uint32_t first = (uint32_t)(4 * t + g) * cap + ng[t][g];      // (read before the count moves: one register per count)
        ng[t][g] += cg;       // (no flag: the counts only grow, so goverflow[t] is read off them after the last flush)
        const bool fits = ng[t][g] <= cap;
        const uint32_t at = __builtin_amdgcn_mbcnt_hi((uint32_t)(mg >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mg, 0u));
        if (fits && pass && have) store_through_at(gl, (at + first) << 2, j, through);
    };
    // the tiles' tests on the survivors in LDS, general path: per tile, (A) the survivors that reach the tile's
    // box, compacted (their positions, one byte each would do: 128 survivors), then (B) the four
    // group tests on those: usually one step of 64 instead of two
    auto flush_general = [&]() __attribute__((always_inline)) {
        wave_lds_fence();
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            if (tile0 + (uint32_t)t >= ntiles) continue;
            float4 gb[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) gb[g] = lds.gbox[t * 4 + g];
            const float4 tb = lds.tbox[t];
            int sel = 0;
            for (int s0 = 0; s0 < sn; s0 += 64) {
                const int k = s0 + lane < sn ? s0 + lane : 0;
                const float4 A = lds.sa[k], B = lds.sb[k];
                Ellipse e;
                e.x = A.x; e.y = A.y; e.a = A.z; e.b = A.w; e.c = B.x; e.nb_c = B.y; e.nb_a = B.z;
                const bool hit = s0 + lane < sn && ellipse_reaches_rect(e, tb.x, tb.y, tb.z, tb.w, pv.q_max);
                const uint64_t hm = __ballot(hit);
                if (hit) lds.sel[sel + lanes_below(hm)] = (uint32_t)k;
                sel += __builtin_popcountll(hm);
            }
            wave_lds_fence();
            for (int s0 = 0; s0 < sel; s0 += 64) {
                const int k = (int)lds.sel[s0 + lane < sel ? s0 + lane : 0];
                const float4 A = lds.sa[k], B = lds.sb[k];
                Ellipse e;
                e.x = A.x; e.y = A.y; e.a = A.z; e.b = A.w; e.c = B.x; e.nb_c = B.y; e.nb_a = B.z;
                const uint32_t j = __builtin_bit_cast(uint32_t, B.w);
                if constexpr (FWD_ONLY) {      // no masks: each group's ballot from its compare, appended at once
                    const bool in = s0 + lane < sel;
                    const uint64_t live = __ballot(in);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float qmin = ellipse_min_q_rect(e, gb[g].x, gb[g].y, gb[g].z, gb[g].w);
                        // (a group without a point has an inverted box, never needed: the ragged last tile alone)
                        const bool held = (has[t] >> g & 1u) != 0u;      // wave-uniform
                        append_group(t, g, !(qmin > a.q_f), in && held, held ? live : 0ull, j);
                    }
                } else {
                    uint32_t gm = 0, gf = 0;       // wide (tile list, backward) and narrow (group lists, forward) masks
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float qmin = ellipse_min_q_rect(e, gb[g].x, gb[g].y, gb[g].z, gb[g].w);
                        if (!(qmin > pv.q_max)) gm |= 1u << g;
                        if (!(qmin > a.q_f)) gf |= 1u << g;
                    }
                    // a group without a point has an inverted box, never needed: the ragged last tile alone (wave-uniform)
                    if (has[t] != 15u) { gm &= has[t]; gf &= has[t]; }
                    if (s0 + lane >= sel) gm = gf = 0u;
                    append(t, j, gm, gf);
                }
            }
            wave_lds_fence();
        }
        sn = 0;
    };
    // ... product path: lane = survivor, all 4 TPW groups of the block from the axis terms of its 2 NI intervals
    // (ellipse_rect.h); bit 4 t + g of the masks = group g of tile t
    auto flush_product = [&]() __attribute__((always_inline)) {
        wave_lds_fence();
        // the group in column i and row i of the block's groups holds x-interval i and y-interval i
        auto diagonal = [](int i) { return TPW == 4 ? 12 * (i >> 1) + 3 * (i & 1) : 3 * i; };
        for (int s0 = 0; s0 < sn; s0 += 64) {
            const bool have = s0 + lane < sn;
            const int k = have ? s0 + lane : 0;
            const float4 A = lds.sa[k], B = lds.sb[k];
            const uint32_t j = __builtin_bit_cast(uint32_t, B.w);
            const float ea = A.z, ec = B.x, b2 = 2.f * A.w;
            if constexpr (FWD_ONLY) {
                // No masks: the group in column c and row r is list g = (c & 1) + 2 (r & 1) of tile t = 2 (c >> 1) +
                // (r >> 1) (bit 4 t + g of the masks below), and the compare's own ballot appends its entries.  Rows
                // and columns unrolled: the running counts are indexed by constants.
                const uint64_t live = __ballot(have);
                // (the intervals are read again in every step: hoisted out of this loop, the 16 of them stay in
                // vector registers across the walk -- 80 -> 86 VGPRs here, scratch in the cells' instantiation)
                asm volatile("" ::: "memory");
                AxisTerms Y[NI];
#pragma unroll
                for (int r = 0; r < NI; ++r) {
                    const float4 d = lds.gbox[diagonal(r)];
                    Y[r] = axis_terms(A.y, ec, b2, B.z, d.y, d.w);
                }
#pragma unroll
                for (int c = 0; c < NI; ++c) {
                    const float4 d = lds.gbox[diagonal(c)];
                    const AxisTerms X = axis_terms(A.x, ea, b2, B.y, d.x, d.z);
#pragma unroll
                    for (int r = 0; r < NI; ++r) {
                        const bool pass = !(min_q_of_terms(X, Y[r], ea, ec) > a.q_f);
                        append_group(2 * (c >> 1) + (r >> 1), (c & 1) + 2 * (r & 1), pass, have, live, j);
                    }
                }
            } else {
                uint32_t gm = 0, gf = 0;
                // Loops, not unrolled (rows and columns are wave-uniform): a fraction of the code and of the registers.
                // A full plan's wave holds more beside the flush, so it takes the rows two at a time -- the columns'
                // terms are then formed once per pair, 28 instructions more per step, for 10 registers fewer.
#pragma nounroll
                for (int r0 = 0; r0 < NI; r0 += 2) {
                    AxisTerms Y[2];
#pragma unroll
                    for (int rr = 0; rr < 2; ++rr) {
                        const float4 d = lds.gbox[diagonal(r0 + rr)];
                        Y[rr] = axis_terms(A.y, ec, b2, B.z, d.y, d.w);
                    }
#pragma nounroll
                    for (int c = 0; c < NI; ++c) {
                        const float4 d = lds.gbox[diagonal(c)];
                        const AxisTerms X = axis_terms(A.x, ea, b2, B.y, d.x, d.z);
                        uint32_t wide = 0, narrow = 0;
#pragma unroll
                        for (int rr = 0; rr < 2; ++rr) {
                            const float qmin = min_q_of_terms(X, Y[rr], ea, ec);
                            if (!(qmin > pv.q_max)) wide |= 1u << 2 * rr;
                            if (!(qmin > a.q_f)) narrow |= 1u << 2 * rr;
                        }
                        // group (column c, row r): tile 2 (c >> 1) + (r >> 1), group (c & 1) + 2 (r & 1); r0 is even
                        const int shift = 8 * (c >> 1) + (c & 1) + 4 * (r0 >> 1);
                        gm |= wide << shift; gf |= narrow << shift;
                    }
                }
                if (!have) gm = gf = 0u;
#pragma unroll
                for (int t = 0; t < TPW; ++t) append(t, j, gm >> (4 * t) & 15u, gf >> (4 * t) & 15u);
            }
        }
        wave_lds_fence();
        sn = 0;
    };
    auto flush = [&]() __attribute__((always_inline)) {
        if (product) flush_product();
        else flush_general();
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
        // (forward-only: unlikely, said aloud -- its unrolled flush wants many scalar registers, and without the hint the
        // walk's own loop counters were the ones kept in lanes of a vector register, 80 VALU instructions per wave;
        // full plans and the fused launch compile as they did without it)
        const bool full = sn + add > SURV_CAP;
        if (FWD_ONLY ? __builtin_expect(full, false) : full) flush();
        if (mask >> lane & 1ull) {
            const Ellipse e = ellipse_of(A, B.x);
            const int k = sn + lanes_below(mask);
            lds.sa[k] = A;
            lds.sb[k] = make_float4(B.x, e.nb_c, e.nb_a, __builtin_bit_cast(float, j));
        }
        sn += add;
    });
    if (sn > 0) flush();
    if constexpr (FWD_ONLY) {
        // an append that did not fit left its list's count above cap, and nothing else can: counts only grow
#pragma unroll
        for (int t = 0; t < TPW; ++t) goverflow[t] = ng[t][0] > cap || ng[t][1] > cap || ng[t][2] > cap || ng[t][3] > cap;
    }

    // A tile list that does not fit while the four group lists do (64 scattered points of a sparse
    // region share few Gaussians: up to 4 x cap distinct ones) is no reason to give the lists up: the
    // forward reads the group lists only, and the backward walks them as four single-group lists
    // (TILE_MODE_GROUPS) -- which must then hold the WIDE set: they are rebuilt below.
    const bool two_cuts = !FWD_ONLY && pv.q_max > a.q_f;
    bool any_rare = false;
    bool rebuild[TPW];
    const bool guard = a.lattice_broken != nullptr;       // launch-uniform
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        rebuild[t] = false;
        if (tile0 + (uint32_t)t >= ntiles) { overflow[t] = false; continue; }
        if (guard) {      // the trusted build's guard (ListArgs::lattice_broken); a comparison that NaN or inf fails: broken
            const float4 tb = lds.tbox[t];
            const float wx = tb.z - tb.x, wy = tb.w - tb.y;
            if (!(wx * a.guard_n[0] <= a.guard_e[0] && wy * a.guard_n[1] <= a.guard_e[1]) && lane == 0) {
                *a.lattice_broken = 1u;
                if (a.home) stats_home(a.home, HOME_LATTICE_BROKEN, 1u);
            }
        }
        const bool tl_over = FWD_ONLY ? goverflow[t] : overflow[t];      // (no tile list: its group lists decide)
        overflow[t] = tl_over && goverflow[t];            // from here on: the tile needs the ranges fallback
        rebuild[t] = tl_over && !goverflow[t] && two_cuts;
        // spread-out points with long lists: the per-point walk is cheaper than the lists (plan.h)
        uint32_t longest = ng[t][0] > ng[t][1] ? ng[t][0] : ng[t][1];
        longest = ng[t][2] > longest ? ng[t][2] : longest;
        longest = ng[t][3] > longest ? ng[t][3] : longest;
        if (longest > POINTS_MODE_MIN_LIST) {      // (strips: the per-point walk needs the grid -- only noted)
            const float4 tb = lds.tbox[t];
            const float wx = tb.z - tb.x, wy = tb.w - tb.y;
            if (strips && wx * gg.inv_s0 * (wy * gg.inv_s0) > POINTS_MODE_MIN_CELLS) {
                if (lane == 0) note_points_wanted();
            }
            if (!strips && wx * gg.inv_s0 * (wy * gg.inv_s0) > POINTS_MODE_MIN_CELLS && walk_candidates() <= 4.f * (float)(longest < cap ? longest : cap)) {
                overflow[t] = false; rebuild[t] = false;
                if (lane < 5)
                    store_through(a.hdr, (size_t)(tile0 + (uint32_t)t) * TILE_HDR_WORDS + lane, lane == 0 ? (TILE_MODE_POINTS << TILE_MODE_SHIFT) : 0u, through);
                if (lane == 0) queue_points_tile(tile0 + (uint32_t)t);
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
            if (lane < 5) store_through(a.hdr, (size_t)(tile0 + (uint32_t)t) * TILE_HDR_WORDS + lane, w, through);      // words 5..7: the block's
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
        const float4 tb = lds.tbox[t];
        const float tx0 = tb.x, ty0 = tb.y, tx1 = tb.z, ty1 = tb.w;
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
                        if (hit) store_through(gl, g * cap + ngw[g] + (uint32_t)lanes_below(mg), j, through);
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
                    store_through(a.hdr, (size_t)(tile0 + (uint32_t)t) * TILE_HDR_WORDS + lane, w, through);
                }
                continue;
            }
            mine = true;          // the wide group lists do not fit either: ranges
        }
        // scattered points (a box of many Gaussian cells for 64 points): no lists, every lane walks the grid
        // around its own point at sampling time (plan.h, TILE_MODE_POINTS)
        if (!strips && (tx1 - tx0) * gg.inv_s0 * ((ty1 - ty0) * gg.inv_s0) > POINTS_MODE_MIN_CELLS && walk_candidates() <= 4.f * (float)cap) {
            if (lane < 5)
                store_through(a.hdr, (size_t)(tile0 + (uint32_t)t) * TILE_HDR_WORDS + lane, lane == 0 ? (TILE_MODE_POINTS << TILE_MODE_SHIFT) : 0u, through);
            if (lane == 0) queue_points_tile(tile0 + (uint32_t)t);
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
                    store_through(tl, p, jb, through); store_through(tl, p + 1, len, through);
                }
            } else {
                fits = false;
            }
            nr += cnt;
        },
                 [](const float4, const float4, uint64_t, uint32_t) {});
        if (!fits && lane == 0) { store_through(tl, 0, 0u, through); store_through(tl, 1, pv.N, through); }
        const uint32_t cnt = fits ? nr : 1u;
        if (lane < 5)
            store_through(a.hdr, (size_t)(tile0 + (uint32_t)t) * TILE_HDR_WORDS + lane, lane == 0 ? (cnt | (TILE_MODE_RANGES << TILE_MODE_SHIFT)) : 0u, through);
    }
}

// the same strips of the domain on the same XCD as in the sampling kernels, which then find a tile's
// lists in the L2 that wrote them (a workgroup here is 4 * TPW tiles; forward 27.05 -> 26.4 us)
template <int TPW>
__device__ __forceinline__ uint32_t lists_tile0(int wave) {
    return (xcd_block_chunk<PIGS_XCD_CHUNK / TPW>(gridDim.x) * 4 + (uint32_t)wave) * TPW;
}
// the first workgroup of a list launch whose statistics are wanted home (ListArgs::parea): the strips' cover of the
// domain (PlanParams::strip_cover), summed from what the build's Gaussian pass left per strip.  Every other launch
// leaves here at once and PlanParams::strip_cover as it was: only the way home reads it.
__device__ __forceinline__ void lists_strip_cover(const ListArgs& a) {
    __shared__ float cover_sh[4];
    if (blockIdx.x != 0 || a.parea == nullptr) return;      // (block-uniform)
    const uint32_t ns = (a.pv.N + STRIP - 1u) / STRIP;
    float sum = 0.f;
    for (uint32_t k = threadIdx.x; k < ns; k += 256u) sum += a.parea[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((threadIdx.x & 63u) == 0u) cover_sh[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float cover = cover_sh[0] + cover_sh[1] + cover_sh[2] + cover_sh[3];
        a.strip_cover[0] = cover;
        const uint32_t w = __builtin_bit_cast(uint32_t, cover);      // (0.0f is the zero word the host left there)
        if (a.home && w != 0u) stats_home(a.home, HOME_STRIP_COVER, w);
    }
}

template <int TPW, bool STRIPS, bool FWD_ONLY = false, bool THROUGH = false>
__global__ __launch_bounds__(256, 5) void plan_lists_kernel(ListArgs a) {
    __shared__ ListsLds<TPW> lds_all[4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    lists_strip_cover(a);
    const uint32_t tile0 = lists_tile0<TPW>(wave);
    if (tile0 >= a.sv.ntiles) return;
    build_block_lists<TPW, STRIPS, FWD_ONLY, true, THROUGH>(a, lds_all[wave], tile0, lane);
}

}  // namespace pigs
