// Binned path, host side: WHICH launches a build issues, as a pure function.  No HIP runtime call, no environment:
// sizes, flags, settings and the memories' last answer in, BuildArgs' flags and the launches out (choose_build),
// plus the two records the library keeps of the last builds of a size (OrderState, PointsState; the table that
// carries them: build_memory.h).  plan.hip's run_build asks, chooses, fills and launches; tests/test_build_choice.py
// holds every rule here against its statement, on a CPU (tests/build_choice_main.hip).
#pragma once
#include "plan.h"
#include <stddef.h>
#include <string.h>

namespace pigs {

// Small point sets (a list launch of fewer tiles than this is one sparse generation of waves): one tile per wave.
constexpr uint32_t LISTS_SMALL_TILES = 4096;
// index-tiled order: from LATTICE_MIN_POINTS points on.  (Until the Gaussians ran one launch ahead -- BuildArgs::ahead
// -- the bar stood at 2^18 points: detecting a lattice adds ~2.5 us to the first launch, sorting one costs ~1 us of
// the count and scatter launches per 131 072 points.  A lattice that is expected now saves a whole launch: 128^2 ...
// 384^2 grids, cold step -4 ... -5 us; BASELINE configs[1] 34.1 -> 31.5 us.)
constexpr int64_t LATTICE_MIN_POINTS = 1 << 12;
// Where the coarse-bin build and the staging records start to pay, measured on uniform random points with one Gaussian
// per 16 points (one box, cold step / forward launches / backward launches, us): 256^2 points: one-pass 49.1 / 18.7 /
// 19.1, coarse-bin 51.1, staged 23.0 / 22.4; 384^2: 61.1 vs 58.9 cold, staged forward 20.8 vs 14.3; 512^2: 70.8 vs
// 66.9 cold, staged 32.2 / 45.2 vs 30.4 / 39.5; 1024^2: 162 vs 122 cold, staged 49 / 104 vs 57 / 110.  Below ~100 k
// points the extra launch of the coarse-bin build costs more than the atomics it saves, and the staging launch more
// than the scattered sectors up to ~500 k.
constexpr int64_t COARSE_MIN_POINTS = 1 << 17;
constexpr int64_t STAGE_MIN_POINTS = 1 << 19;
// A build is trusted from this many verified builds in a row on: longer than any run of lattice builds after which the
// suite switches to other points of the same count and wants them noticed by the very next build
// (tests/test_lattice_gpu.py: 40), short next to a training run.
constexpr uint32_t TRUST_MIN_BUILDS = 64;
constexpr float STRIP_MAX_COVER = 64.f;            // (PointsState::takes_strips)
constexpr int64_t STRIP_MIN_GAUSSIANS = 1024;      // (below, the chain strips replace is not what a step waits for)

// What a caller asks of run_build (pigs_plan_build's PIGS_BUILD_* flags by name).
struct BuildRequest {
    bool do_samples = false, do_plan = false;
    bool plan_ws_clean = false;      // PIGS_BUILD_PLAN_WS_CLEAN
    bool no_lookback = false;        // PIGS_BUILD_DEBUG_NO_LOOKBACK
    bool build_lists = true;
    int order = 0;                   // 0 = ask the memory, 1 = ordered (one pass), 2 = unordered (coarse bins)
    bool defer_lists = false, fwd_only = false;
    int64_t N = 0, M = 0;
    int c = 1;
    float q_max = 1.f, q_max_b = 1.f;
};

// The settings that steer a build, as the environment spells them (plan.hip, build_env; -1: not set).
struct BuildEnv {
    int lattice = -1;            // PIGS_LATTICE=1 / 0: index-tiled order always / never
    int lattice_trust = -1;      // PIGS_LATTICE_TRUST: 0 = never (A/B: the verified chain), 1 = as soon as the memory holds a
                                 // row length and a stable box (tests, tools/lattice_trust_worst_case.py)
    int samples_order = 0;       // PIGS_SAMPLES_ORDER = ordered (1) | unordered (2): overrules BuildRequest::order
    int gauss_strips = -1;       // PIGS_GAUSS_STRIPS=0 / 1: never / always
    int bbox_blocks = -1;        // PIGS_BBOX_BLOCKS (A/B: 256 | 512), read once per process
    bool no_ahead = false;       // PIGS_NO_AHEAD, read once per process
    bool stats_home = true;      // PIGS_STATS_HOME=0: a plan's statistics travel by a copy of its header, not by the list
                                 // launch's own stores (tests, A/B; no launch of the build's own depends on it)
};

// What the memories said of these sizes (all zero: nothing), resolved by the caller for "inside a capture".
struct MemoryAnswer {
    bool coarse = false;         // the last completed build's points came in no order
    uint32_t rf = 0, axis = 0;   // its lattice row length (0: none) and fast axis
    bool box_ok = false;         // the same box in the last two completed builds: box
    float box[4] = {0.f, 0.f, 0.f, 0.f};
    bool trust = false;          // OrderState::trusts, never inside a capture
    bool takes_strips = false;   // PointsState::takes_strips
};

enum BuildKernel : uint32_t {
    K_SAMPLES_BBOX, K_PLAN_ZERO, K_PLAN_COUNT, K_PLAN_SCAN, K_PLAN_SCATTER, K_BINSORT_16, K_BINSORT_1,
    K_LISTS_SMALL,      // plan_lists_kernel<1, strips, fwd_only>
    K_LISTS             // plan_lists_kernel<LISTS_TPW, strips, fwd_only>
};
struct BuildLaunch {
    BuildKernel kernel;
    uint32_t grid, block, lds;      // workgroups, threads of one, dynamic LDS bytes
};
struct BuildChoice {
    // into BuildArgs (plan_build.h)
    bool coarse, no_lattice;
    uint32_t rf_hint, bbox_blocks;
    bool fwd_only, ahead, s_scan_in_scatter, sort_in_count, strips, trusted;
    uint32_t s_blocks;
    float q_max_b;                  // the wide cut-off this build takes
    BuildLaunch launches[7];
    int n = 0;
    void add(BuildKernel k, uint32_t grid, uint32_t block = 256, uint32_t lds = 0) { launches[n++] = BuildLaunch{k, grid, block, lds}; }
};

inline BuildLaunch list_launch(uint32_t ntiles) {
    const bool small = ntiles <= LISTS_SMALL_TILES && LISTS_TPW != 1;
    return small ? BuildLaunch{K_LISTS_SMALL, (ntiles + 3) / 4, 256, 0}
                 : BuildLaunch{K_LISTS, (ntiles + 4 * LISTS_TPW - 1) / (4 * LISTS_TPW), 256, 0};
}

// does the build end in its list launch, lists from strips allowed (PlanParams::strips)?
inline bool strips_allowed(const BuildRequest& r) { return r.do_plan && r.build_lists && !r.defer_lists && !r.no_lookback; }
// ... and is it for the points' memory to say (run_build asks it only then)
inline bool strips_asked(const BuildRequest& r, const BuildEnv& env) {
    return strips_allowed(r) && env.gauss_strips < 0 && r.N >= STRIP_MIN_GAUSSIANS;
}

// p: only read when r.do_plan
inline BuildChoice choose_build(const BuildRequest& r, const SamplesLayout& s, const PlanLayout& p, const BuildEnv& env,
                                const MemoryAnswer& mem) {
    BuildChoice b{};
    const int64_t M = r.M;
    const int order = env.samples_order ? env.samples_order : r.order;
    // which way a samples build sorts its points: unordered points want the coarse-bin path, points in runs the one-pass
    // build (plan.h, SamplesLayout)
    b.coarse = r.do_samples && s.cells_per_bin <= SAMPLES_MAX_CELLS_PER_BIN &&
               (order ? order == 2 : M >= COARSE_MIN_POINTS && mem.coarse);
    b.rf_hint = r.do_samples ? mem.rf : 0u;
    // same box, 1024^2 points: the plain pass 6.6 -> 5.9 us with 512 workgroups, the pass with a row length 7.5 -> 7.8
    b.bbox_blocks = (env.bbox_blocks >= 0 ? env.bbox_blocks == 512 : M >= (int64_t)BBOX_WIDE_POINTS && b.rf_hint == 0u) ? 512u : 256u;
    b.q_max_b = r.q_max_b >= r.q_max ? r.q_max_b : r.q_max;      // <= 0 / NaN: one cut-off
    // a plan for the forward alone is sized with the forward's cut-off throughout (boxes, levels, strips, the walk)
    b.fwd_only = r.fwd_only && r.do_plan && r.build_lists && !r.defer_lists;
    if (b.fwd_only) b.q_max_b = r.q_max;
    b.no_lattice = env.lattice >= 0 ? env.lattice == 0 : M < LATTICE_MIN_POINTS;
    // The Gaussians one launch ahead (BuildArgs::ahead): a lattice is expected, the samples' box was the same in the last
    // two completed builds of this size, the plan workspace's counters are zero.
    b.ahead = r.do_samples && r.do_plan && r.plan_ws_clean && !b.coarse && !r.no_lookback && !env.no_ahead &&
              b.rf_hint != 0u && !b.no_lattice && mem.box_ok && s.scan_blocks <= 1024u;
    b.s_scan_in_scatter = b.ahead;
    // Gaussians whose order in the caller's array is already spatial keep it (PlanParams::strips): one pass instead of
    // count, scan and scatter.  (A build that also sorts or looks at the samples saves no launch by it -- the Gaussians'
    // count, scan and scatter ride along in launches that exist anyway -- but the lists from strips are the faster ones
    // since the survivors wait for a full buffer: 20.0 against 21.3 us at C3, 55 against 60 at kappa 1.3, and the scan /
    // scatter launches carry less)
    b.strips = strips_allowed(r) && (env.gauss_strips >= 0 ? env.gauss_strips == 1 : r.N >= STRIP_MIN_GAUSSIANS && mem.takes_strips);
    // TRUSTED: point sets of this size have been the same compact lattice for TRUST_MIN_BUILDS verified builds and three
    // copies in a row -- this build does not look again.  It launches what a build on a finished samples workspace
    // launches, the Gaussians' pack and the lists; the pack's first workgroup writes the samples header the decision
    // would have written, the list launch reads the points through it and holds every tile's real box against the
    // remembered one (ListArgs::lattice_broken), and that word goes home with the plan's statistics every 8th build
    // (plan.hip, points_landed turns the memory around).  Results never depend on it: the lists come from the groups'
    // real boxes.
    const uint32_t rf = b.rf_hint;
    b.trusted = b.ahead && b.strips && mem.trust && r.order == 0 && rf >= 8u && (rf & 7u) == 0u && M >= 64 && M % rf == 0 &&
                ((M / rf) & 7) == 0;
    const uint32_t gb = r.do_plan ? (uint32_t)((r.N + 255) / 256) : 0u;
    const uint32_t s_blocks = (uint32_t)((M + 1023) / 1024), s_eighth = (s_blocks + 7u) / 8u;
    b.s_blocks = b.trusted ? 0u : s_blocks;
    if (b.trusted) {
        b.ahead = b.s_scan_in_scatter = false;
        b.add(K_PLAN_COUNT, gb);
    } else if (b.ahead && b.strips) {
        // nothing of the Gaussians is left for launches 2 and 3: the samples' fall-back moves into launch 2 whole
        // (samples_sort_in_count; at most 256 workgroups: they meet at device-wide barriers) -- FOUR launches up to the forward
        b.sort_in_count = true; b.s_scan_in_scatter = false;
        b.add(K_SAMPLES_BBOX, b.bbox_blocks + gb, BBOX_THREADS);
        b.add(K_PLAN_COUNT, s_eighth < 256u ? s_eighth : 256u);
    } else if (b.ahead) {
        b.add(K_SAMPLES_BBOX, b.bbox_blocks + gb, BBOX_THREADS);
        b.add(K_PLAN_COUNT, p.scan_blocks + s_eighth);
        b.add(K_PLAN_SCATTER, gb + (uint32_t)((M + 255) / 256));
    } else {
        if (r.do_samples) b.add(K_SAMPLES_BBOX, b.bbox_blocks, BBOX_THREADS);
        else if (!r.plan_ws_clean) b.add(K_PLAN_ZERO, 64);
        // a lattice expected (the row length of the last build of this size): an eighth of the one-pass count's workgroups
        // -- they leave at once when the points are index-tiled, and stride over the blocks when they are not
        const uint32_t count_wgs = b.coarse ? s.h_wgs : (b.rf_hint && !b.no_lattice ? s_eighth : s_blocks);
        b.add(K_PLAN_COUNT, gb + (r.do_samples ? count_wgs : 0u));
        const uint32_t s_scan_blocks = b.coarse ? s.h_scan_blocks : s.scan_blocks;
        const uint32_t scan_wgs = (r.do_plan && !b.strips ? p.scan_blocks : 0u) + (r.do_samples ? s_scan_blocks : 0u);
        if (scan_wgs) b.add(K_PLAN_SCAN, scan_wgs);
        const bool staged = b.coarse && s.h_chunk <= SCATTER_STAGE_MAX;
        const uint32_t scatter_wgs = (b.strips ? 0u : gb) + (r.do_samples ? (staged ? s.h_wgs : (uint32_t)((M + 255) / 256)) : 0u);
        if (scatter_wgs)
            b.add(K_PLAN_SCATTER, scatter_wgs, 256,
                  staged ? (uint32_t)(s.h_chunk * sizeof(uint4) + 2 * SAMPLES_COARSE_BINS * sizeof(uint32_t)) : 0u);
        if (b.coarse) {
            if (s.cells_per_bin * 16u <= SAMPLES_MAX_CELLS_PER_BIN)      // the LDS holds 16 sub-cell counters per cell
                b.add(K_BINSORT_16, SAMPLES_COARSE_BINS, 1024, s.cells_per_bin * 16u * (uint32_t)sizeof(uint32_t));
            else
                b.add(K_BINSORT_1, SAMPLES_COARSE_BINS, 1024, s.cells_per_bin * (uint32_t)sizeof(uint32_t));
        }
    }
    if (r.do_plan && r.build_lists && !r.defer_lists) b.launches[b.n++] = list_launch(s.ntiles);
    return b;
}

// ---- the samples' memory: which way a samples build sorts its points, and what it may take for granted ----
// The host cannot look at the points without a synchronisation.  So every build of a point set leaves {runs, points}
// of a sample of its waves, its box and its lattice in the workspace header, the library copies those 64 bytes to
// pinned memory on the build's stream behind the build (no wait), and the NEXT build of a point set of the same size on
// the same device takes what the last completed copy says: a training loop that draws new random collocation points
// every step (main_pn.py:103, test_no_mlp.py:86) switches to the coarse bins after its first step or two, a lattice
// never does.  A capture neither asks nor copies (it keeps the mode of the moment).  PIGS_SAMPLES_ORDER, or the
// PIGS_BUILD_POINTS_* flags, overrule the memory; the result is the same either way (order inside a fine cell aside),
// only the time differs.
constexpr uint32_t ORDER_WORDS = 16;        // the first 64 bytes of SampleParams (box, grid, order_stat, lat_cand, lat)
static_assert(offsetof(SampleParams, box) == 0 && offsetof(SampleParams, order_stat) == 40 && offsetof(SampleParams, lat) == 56,
              "the order copy: the first 64 bytes of SampleParams");
struct OrderState {
    bool coarse = false;
    uint32_t rf = 0;               // the row length of the last completed build when it took the index-tiled order (else 0)
    uint32_t axis = 0;             // the fast axis that goes with `rf` (SampleParams::lat_cand[1])
    float box[4] = {0.f, 0.f, 0.f, 0.f};   // the samples' bounding box of the last completed build
    bool box_seen = false;         // ... and whether the completed build before it had the same one: a box to build the
    bool box_stable = false;       //     Gaussians' grid on before this build's own is known (BuildArgs::ahead)
    uint32_t same = 0;             // completed copies in a row that said the same (row length, box): the copies get rarer
    uint32_t streak = 0;           // verified builds since a completed copy last said anything but (rf, box): builds between
                                   // two copies are taken on the word of the copies around them
    uint32_t trusted = 0;          // trusted builds of this (device, M) so far
    uint32_t broken = 0;           // times the list launch's guard turned this memory around
    uint32_t builds = 0;           // samples builds of this (device, M) so far

    void absorb(const uint32_t* w) {          // a copy has landed
        const uint32_t rf_before = rf;
        rf = w[14];           // SampleParams::lat[0]
        axis = w[13];         // SampleParams::lat_cand[1]
        if (rf != 0u) coarse = false;      // index-tiled: the points arrived in order (and left no run statistic)
        else if (w[11] > 0u) coarse = (uint64_t)w[10] * 100u > (uint64_t)w[11] * 55u;
        float b[4];
        memcpy(b, w, sizeof(b));
        const auto fin = [](float x) { return __builtin_fabsf(x) < 3.0e38f; };
        const bool finite = fin(b[0]) && fin(b[1]) && fin(b[2]) && fin(b[3]) && b[2] > b[0] && b[3] > b[1];
        box_stable = finite && box_seen && memcmp(b, box, sizeof(b)) == 0;
        same = box_stable && rf == rf_before ? same + 1u : 0u;
        if (rf == 0u || rf != rf_before || !box_stable) streak = 0u;
        box_seen = finite;
        memcpy(box, b, sizeof(b));
    }
    // the list launch's guard met points that are no compact lattice in the remembered order: the next build searches,
    // verifies and, if need be, sorts, as a first build does
    void turn_around() { rf = 0u; same = 0u; box_stable = false; streak = 0u; ++broken; }
    // may a build of this size go without looking at the points?  mode: BuildEnv::lattice_trust
    bool trusts(int mode) const {
        if (mode == 0 || rf == 0u || !box_stable) return false;
        return mode == 1 || (same >= 2u && streak >= TRUST_MIN_BUILDS);
    }
    // is the copy asked for behind build number `nth` (from 0)?  After the first two, every 16th (the samples' copy is
    // a blit kernel of ~4 us in the build's stream: its order_stat words are sums that are final at the kernel's end
    // only, so they cannot be stored home the way the plans' words are -- and a trusted build asks for none).  With a row length in the memory the build runs on expectations -- an eighth of the
    // count's workgroups, the Gaussians one launch ahead -- and a point set that stopped meeting them should not be met
    // 15 more times: every 8th build then, every 32nd once three copies in a row have said the same.
    bool copy_due(uint32_t nth) const { return nth < 2u || (nth & (rf ? (same >= 2u ? 31u : 7u) : 15u)) == 0u; }
};

// ---- the plans' memory: does a plan of these sizes hold tiles in TILE_MODE_POINTS, do its Gaussians come in strips? ----
// The fused first forward walks such tiles in their own list wave (right, and slow when there are hundreds: the thin
// outskirts of a clustered cloud), the two-launch path spreads them over helper workgroups.  Which one a plan wants is
// known on the device only, so the library remembers, per device and (N, M): the list launch of the first two plans of
// a size and of every 16th stores five words -- the ones from PlanParams::n_points on, each reduced to "zero or not"
// but the cover -- into pinned memory that the device addresses, where they come into being, and an event follows the
// launch (nobody waits, and no launch is added; PIGS_STATS_HOME=0: the five words are copied out of the header by a blit
// behind the build instead); a first forward takes the fused launch unless the last completed picture for its sizes
// showed such tiles.  Never inside a capture.  ("Copy" below: such a picture, whichever way it came.)
constexpr uint32_t POINTS_WORDS = 5;        // {n_points, strip_cover, strips, points_wanted, lattice_broken}
static_assert(offsetof(PlanParams, strip_cover) == offsetof(PlanParams, n_points) + 4 && offsetof(PlanParams, strips) == offsetof(PlanParams, n_points) + 8 &&
              offsetof(PlanParams, points_wanted) == offsetof(PlanParams, n_points) + 12 && offsetof(PlanParams, lattice_broken) == offsetof(PlanParams, n_points) + 16,
              "one copy: n_points, strip_cover, strips, points_wanted, lattice_broken");      // (plan_lists.h, HOME_*: the same order)
struct PointsState {
    bool has_points = false;
    float cover = -1.f;            // PlanParams::strip_cover of the last completed build (< 0: none yet)
    bool strips = false;           // ... and whether that build kept the caller's order
    uint32_t same = 0;             // completed copies in a row that led to the same choice: the copies get rarer
    uint32_t builds = 0;

    // Does the next build of these sizes keep the caller's order (PlanParams::strips)?  Yes when the last completed build's
    // strips covered the samples' domain at most STRIP_MAX_COVER times -- that number is about how many strips a block of
    // tiles meets (a lattice in row order, a strip of 1 x 16 widened by its ellipses' reach on every side: ~10 times at
    // kappa = 0.5, ~17 at 0.8, ~33 at 1.3; Gaussians in no order: every strip covers the domain, N / 16 times).
    // (Tiles of far-apart points -- a cloud's thin outskirts -- are walked point by point through the GRID at sampling
    // time, TILE_MODE_POINTS: a plan that had such tiles keeps the cells.  Measured without: clamped normals
    // sigma = 0.15 over lattice Gaussians, warm step 111 -> 1 126 us.)
    bool takes_strips() const { return cover >= 0.f && cover <= STRIP_MAX_COVER && !has_points; }
    // a copy has landed; true: a trusted build's guard said lattice_broken (the caller turns the samples' memory around).
    // Words 0, 3 and 4 count as "zero or not": stored home by the list launch they are 0 or 1, copied they are counts.
    bool absorb(const uint32_t* w) {
        const bool took_before = takes_strips();
        has_points = w[0] != 0u || w[3] != 0u;
        memcpy(&cover, &w[1], sizeof(float));
        if (!(cover >= 0.f)) cover = 3.0e38f;      // NaN: as bad as it gets
        strips = w[2] != 0u;
        same = takes_strips() == took_before ? same + 1u : 0u;
        return w[4] != 0u;
    }
    // as OrderState::copy_due.  Builds that keep the caller's order run on an expectation -- strips that cover the domain
    // a few times over -- and Gaussians that stopped meeting it should not be met 15 more times; nor points that stopped
    // being the lattice a trusted build takes them for 31 more times: every 8th
    bool copy_due(uint32_t nth, bool trusted) const {
        return nth < 2u || (nth & (trusted ? 7u : strips ? (same >= 2u ? 31u : 7u) : 15u)) == 0u;
    }
};

}  // namespace pigs
