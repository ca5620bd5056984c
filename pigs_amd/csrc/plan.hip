// Binned (culled) sampler: preprocess (samples build + plan build) + forward + backward, float32, d = 2.
// Data structures and the cut-off rule: plan.h.  Per-pair arithmetic: pair_math.h.
//
// One translation unit; the device code lies in four headers, by stage, each included here alone:
//   plan_build.h     samples build and the Gaussians' chain: bbox -> cell key + rank -> scan -> scatter
//   plan_lists.h     the tile lists: one wave walks the Gaussian grid once for four consecutive 64-point tiles
//   plan_forward.h   one wave = one tile; what forward and backward share, the forward, the fused list + forward launch
//   plan_backward.h  the backward over the tile lists, the way back to the caller's order
// This file: the host half -- workspaces, entry points, and a build in five steps (run_build).  Which launches a build
// issues is build_choice.h's pure function; the library's memory of the last builds is build_memory.h's table.
//
// Build-time knobs (defaults measured on MI355X): PIGS_FWD_WAVES, PIGS_FWD_WG_WAVES,
// PIGS_FWD_UNROLL, PIGS_GROUP_CAP (plan_forward.h), PIGS_BWD_WAVES, PIGS_BWD_STEP (plan_backward.h),
// PIGS_LISTS_TPW (plan_lists.h), PIGS_XCD_CHUNK (plan_build.h), PIGS_TRAV_STEPS (grid_walk.h).
#include "pair_math.h"
#include "plan.h"
#include "grid_walk.h"
#include "launch.h"
#include "plan_build.h"
#include "plan_lists.h"
#include "plan_forward.h"
#include "plan_backward.h"
#include "build_choice.h"
#include "build_memory.h"
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <mutex>
#include <unordered_map>

namespace pigs {

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static bool samples_supported(int64_t M) { return M >= 1 && M < (1LL << 31) - 64; }
static bool plan_supported(int64_t N, int64_t M, int c) {
    return samples_supported(M) && N >= 1 && c >= 1 && c <= 2 && N < (1LL << LIST_IDX_BITS);
}

static SamplesView make_samples_view(const SamplesLayout& p, const void* sws) {
    const char* b = (const char*)sws;
    SamplesView v{};
    v.params = (const SampleParams*)(b + p.off_params);
    v.spts = (const SPoint*)(b + p.off_spts);
    v.M = (uint32_t)p.M;
    v.ntiles = p.ntiles;
    return v;
}

static PlanView make_view(const PlanLayout& p, void* ws, float q_max) {
    char* b = (char*)ws;
    PlanView v{};
    v.params = (const PlanParams*)(b + p.off_params);
    v.starts = (const uint32_t*)(b + p.off_starts);
    v.rec = (const float4*)(b + p.off_rec);
    v.gbox = (const float4*)(b + p.off_box);
    v.g2o = (const uint32_t*)(b + p.off_g2o);
    v.hdr = (const uint32_t*)(b + p.off_hdr);
    v.tlist = (const uint32_t*)(b + p.off_tlist);
    v.glist = (const uint32_t*)(b + p.off_glist);
    v.ptiles = (const uint32_t*)(b + p.off_ptiles);
    v.N = (uint32_t)p.N;
    v.list_cap = p.list_cap;
    v.G0 = p.G0; v.L = p.L;
    for (int l = 0; l <= PLAN_MAX_LEVELS; ++l) v.level_off[l] = p.level_off[l];
    v.q_max = q_max;
    v.gacc = (float*)(b + p.off_gacc);
    v.pbox = (const float4*)(b + p.off_pbox);
    v.sbox = (const float4*)(b + p.off_sbox);
    v.stage = (float4*)(b + p.off_stage);
    return v;
}

size_t samples_error_offset() { return offsetof(SampleParams, scan_error); }
size_t plan_error_offset() { return offsetof(PlanParams, scan_error); }
size_t samples_lattice_offset() { return offsetof(SampleParams, lat); }
size_t plan_strips_offset() { return offsetof(PlanParams, strips); }      // (the parameters open the workspace)

int plan_layout_info(int64_t N, int64_t M, int c, int64_t* info) {
    if (!plan_supported(N, M, c)) return PIGS_ERR_UNSUPPORTED;
    const PlanLayout p = make_plan_layout(N, M, c);
    info[0] = p.ntiles; info[1] = p.list_cap; info[2] = (int64_t)p.off_hdr; info[3] = (int64_t)p.off_tlist;
    info[4] = (int64_t)p.off_g2o; info[5] = (int64_t)p.off_glist;
    return PIGS_OK;
}

int plan_records_info(int64_t N, int64_t M, int c, int64_t* info) {
    if (!plan_supported(N, M, c)) return PIGS_ERR_UNSUPPORTED;
    const PlanLayout p = make_plan_layout(N, M, c);
    info[0] = (int64_t)p.off_rec; info[1] = (int64_t)p.off_pbox; info[2] = (int64_t)p.off_sbox; info[3] = 0;
    return PIGS_OK;
}

int samples_layout_info(int64_t M, int64_t* info) {
    if (!samples_supported(M)) return PIGS_ERR_UNSUPPORTED;
    const SamplesLayout s = make_samples_layout(M);
    info[0] = s.ntiles; info[1] = (int64_t)s.off_spts; info[2] = (int64_t)sizeof(SPoint); info[3] = 0;
    return PIGS_OK;
}

size_t samples_workspace_bytes(int64_t M) {
    if (!samples_supported(M)) return 0;
    return make_samples_layout(M).total_bytes;
}

size_t plan_workspace_bytes(int64_t N, int64_t M, int c) {
    if (!plan_supported(N, M, c)) return 0;
    return make_plan_layout(N, M, c).total_bytes;
}

static void fill_samples_args(BuildArgs& a, const SamplesLayout& s, void* sws, const void* samples, bool coarse) {
    char* b = (char*)sws;
    a.sparams = (SampleParams*)(b + s.off_params);
    a.sboxes = (float4*)(b + s.off_boxes);
    a.slat = (float4*)(b + s.off_lat);
    a.skey = (uint2*)(b + s.off_skey);
    a.spts = (SPoint*)(b + s.off_spts);
    a.samples = (const float*)samples;
    a.M = (uint32_t)s.M;
    a.scells_cap = s.scells_cap;
    a.coarse = coarse;
    a.cells_per_bin = s.cells_per_bin; a.h_chunk = s.h_chunk; a.h_wgs = s.h_wgs;
    a.tmp = (STmp*)(b + s.off_tmp);
    if (coarse) {      // the scan runs over the (bin, workgroup) count matrix, which every build overwrites whole
        a.scounts = (uint32_t*)(b + s.off_hist);
        a.sagg = (unsigned long long*)(b + s.off_hagg);
        a.sstarts = (uint32_t*)(b + s.off_hstarts);
        a.s_scan_blocks = s.h_scan_blocks;
        a.szero = (uint32_t*)(b + s.off_hagg);
        a.s_zero_words = (uint32_t)((s.off_hstarts - s.off_hagg) / 4);    // the scan's aggregates
    } else {
        a.scounts = (uint32_t*)(b + s.off_counts);
        a.sagg = (unsigned long long*)(b + s.off_agg);
        a.sstarts = (uint32_t*)(b + s.off_starts);
        a.s_scan_blocks = s.scan_blocks;
        a.szero = a.scounts;
        a.s_zero_words = (uint32_t)((s.off_starts - s.off_counts) / 4);     // counters + aggregates
    }
}

// ---- the settings that steer a build (build_choice.h, BuildEnv): read here and nowhere else ----
static int samples_order_setting() {      // PIGS_SAMPLES_ORDER
    const char* e = getenv("PIGS_SAMPLES_ORDER");
    return !e ? 0 : !strcmp(e, "ordered") ? 1 : !strcmp(e, "unordered") ? 2 : 0;
}
// PIGS_LISTS_PRODUCT=0: no block of a list launch takes the product path of the flush (plan_lists.h; tests and the A/B).
// Read at every build like the others; it steers no launch choice, so it rides in ListArgs, not in BuildEnv.
static uint32_t lists_product_setting() {
    const char* e = getenv("PIGS_LISTS_PRODUCT");
    return e && e[0] == '0' ? 0u : 1u;
}
// PIGS_STORE_THROUGH=0: no list launch sends its headers and lists by write-through stores (plan.h, store_through;
// launch_lists says which do; the A/B and tests/test_store_through_gpu.py).  Read at every build like the others; it steers no
// launch choice, only the instantiation of the list kernel, so it rides in ListArgs, not in BuildEnv.  (The strips pack
// had such stores too, `=pack`: slower by the bench line, taken out -- DESIGN.md section 3.3.)
static uint32_t store_through_setting() {
    const char* e = getenv("PIGS_STORE_THROUGH");
    return e && e[0] == '0' ? 0u : 1u;
}
static BuildEnv build_env() {
    static const char* const bbox = getenv("PIGS_BBOX_BLOCKS");      // the two A/B settings: once per process
    static const bool no_ahead = getenv("PIGS_NO_AHEAD") != nullptr;
    BuildEnv env;      // the others at every build: the tests flip them inside one process
    if (const char* e = getenv("PIGS_LATTICE")) env.lattice = e[0] != '0';
    if (const char* e = getenv("PIGS_LATTICE_TRUST")) env.lattice_trust = e[0] == '0' ? 0 : e[0] == '1' ? 1 : -1;
    env.samples_order = samples_order_setting();
    if (const char* e = getenv("PIGS_GAUSS_STRIPS")) env.gauss_strips = e[0] == '1';
    if (const char* e = getenv("PIGS_STATS_HOME")) env.stats_home = e[0] != '0';
    if (bbox) env.bbox_blocks = atoi(bbox) == 512 ? 512 : 256;
    env.no_ahead = no_ahead;
    return env;
}

// ---- the library's memory of the last builds: the records and their rules in build_choice.h, the table in
// build_memory.h.  Process-global, per device and size; one mutex for both tables (a plan's copy can turn the samples'
// record around).
struct OrderKey {
    int64_t M;
    bool operator==(const OrderKey& o) const { return M == o.M; }
};
struct PointsKey {
    int64_t N, M;
    bool operator==(const PointsKey& o) const { return N == o.N && M == o.M; }
};
using OrderMemory = BuildMemory<OrderKey, OrderState, ORDER_WORDS>;
using PointsMemory = BuildMemory<PointsKey, PointsState, POINTS_WORDS>;
static void order_landed(OrderMemory::Slot& s) { s.st.absorb(s.host); }
static void points_landed(PointsMemory::Slot& s);
static std::mutex g_memory_mu;
static OrderMemory g_order{order_landed};
static PointsMemory g_points{points_landed};
static void points_landed(PointsMemory::Slot& s) {
    // a trusted build met points that are no compact lattice in the remembered order (plan_lists.h, the guard): the
    // samples' memory of this size turns around
    if (s.st.absorb(s.host))
        if (auto* o = g_order.find(s.device, OrderKey{s.key.M})) o->st.turn_around();
}

// What the memories say to a build.  The samples' is asked by every build that sorts points, the plans' only where
// its word decides (strips_asked); a capture reads what is there and looks at no copy.
static MemoryAnswer ask_memories(const BuildRequest& r, const BuildEnv& env, hipStream_t stream) {
    MemoryAnswer m;
    const bool points = strips_asked(r, env);
    int dev = 0;
    if ((!r.do_samples && !points) || !current_device(&dev)) return m;
    const bool cap = stream_capturing(stream);
    std::lock_guard<std::mutex> lock(g_memory_mu);
    if (r.do_samples)
        if (auto* o = g_order.find(dev, OrderKey{r.M})) {
            if (!cap) g_order.poll(*o);
            m.coarse = o->st.coarse; m.rf = o->st.rf; m.axis = o->st.axis;
            if (o->st.box_stable) { m.box_ok = true; memcpy(m.box, o->st.box, sizeof(m.box)); }
            m.trust = !cap && o->st.trusts(env.lattice_trust);
        }
    if (points)
        if (auto* h = g_points.find(dev, PointsKey{r.N, r.M})) {
            if (!cap) g_points.poll(*h);
            m.takes_strips = h->st.takes_strips();
        }
    return m;
}

// behind a samples build: count it and, when one is due, ask for its header's words (a trusted build left none)
static void note_order(const SamplesLayout& s, const void* sws, hipStream_t stream, bool trusted) {
    if (!trusted && (s.M < 64 || stream_capturing(stream))) return;
    int dev = 0;
    if (!current_device(&dev)) return;
    std::lock_guard<std::mutex> lock(g_memory_mu);
    auto* o = g_order.find(dev, OrderKey{s.M}, !trusted);
    if (!o) return;
    if (trusted) { ++o->st.trusted; return; }
    const uint32_t nth = o->st.builds++;
    if (o->st.rf != 0u) ++o->st.streak;
    if (!o->pending && o->st.copy_due(nth)) g_order.request(*o, (const char*)sws + s.off_params, stream);
}
// In front of a build that ends in its list launch: count it and, when its statistics are due at home, reserve the slot
// they go to (null: not due, or inside a capture).  trusted: its guard's word is wanted home soon.
static PointsMemory::Slot* points_due(const PlanLayout& p, hipStream_t stream, bool trusted) {
    int dev = 0;
    if (stream_capturing(stream) || !current_device(&dev)) return nullptr;
    std::lock_guard<std::mutex> lock(g_memory_mu);
    auto* h = g_points.find(dev, PointsKey{p.N, p.M}, true);
    if (!h) return nullptr;
    const uint32_t nth = h->st.builds++;
    if (h->pending || !h->st.copy_due(nth, trusted)) return nullptr;
    g_points.reserve(*h);
    return h;
}
// ... the slot's words as the list launch addresses them, zeroed but for the one the host knows (ListArgs::home)
static uint32_t* points_home(PointsMemory::Slot& h, bool strips) {
    std::lock_guard<std::mutex> lock(g_memory_mu);
    uint32_t* home = g_points.home(h);
    h.host[HOME_STRIPS] = strips ? 1u : 0u;
    return home;
}
// ... and behind the build's launches (ok: they were issued): the event behind the list launch's stores, or
// (home == null, PIGS_STATS_HOME=0) the copy of the five words from PlanParams::n_points on and its event
static void note_points(PointsMemory::Slot& h, bool ok, const uint32_t* home, const PlanLayout& p, const void* ws, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(g_memory_mu);
    if (!ok) g_points.release(h);
    else if (home) g_points.sent(h, stream);
    else g_points.request(h, &((const PlanParams*)((const char*)ws + p.off_params))->n_points, stream);
}

// behind the list launch of a plan with deferred lists (the first sampling call's): count it and, when due, copy
static void note_deferred_points(const PlanLayout& p, const void* ws, hipStream_t stream) {
    if (PointsMemory::Slot* due = points_due(p, stream, false)) note_points(*due, true, nullptr, p, ws, stream);
}

// The sampling launches' question (staging, PlanView::stage): did the point set of this size arrive in no order?
// A pending statistic is looked at here too -- a point set that is built once and sampled many times (fixed random
// collocation points) never comes back to a build -- unless the stream is being captured.
static bool points_unordered(int64_t M, hipStream_t stream) {
    if (const char* e = getenv("PIGS_STAGE")) return e[0] == '1';          // tests / A-B runs: staging on or off whatever the memory and the size
    if (M < STAGE_MIN_POINTS) return false;
    if (getenv("PIGS_SAMPLES_ORDER")) return samples_order_setting() == 2;
    int dev = 0;
    if (!current_device(&dev)) return false;
    const bool cap = stream_capturing(stream);
    std::lock_guard<std::mutex> lock(g_memory_mu);
    auto* o = g_order.peek(dev, OrderKey{M});
    if (!o) return false;
    if (!cap) g_order.poll(*o);
    return o->st.coarse;
}
// a first forward takes the fused launch unless the last completed copy for its sizes showed TILE_MODE_POINTS tiles
static bool plan_expects_points(int64_t N, int64_t M, hipStream_t stream) {
    int dev = 0;
    if (!current_device(&dev)) return false;
    const bool cap = stream_capturing(stream);
    std::lock_guard<std::mutex> lock(g_memory_mu);
    auto* h = g_points.find(dev, PointsKey{N, M});
    if (!h) return false;
    if (!cap) g_points.poll(*h);
    return h->st.has_points;
}

int samples_order_hint(int64_t M) {
    int dev = 0;
    if (!current_device(&dev)) return -1;
    std::lock_guard<std::mutex> lock(g_memory_mu);
    auto* o = g_order.find(dev, OrderKey{M});
    if (!o) return -1;
    g_order.poll(*o);
    return o->st.coarse ? 1 : 0;
}

int samples_trust_info(int64_t M, int64_t* info) {
    info[0] = info[1] = info[2] = info[3] = 0;
    int dev = 0;
    if (!current_device(&dev)) return PIGS_OK;
    std::lock_guard<std::mutex> lock(g_memory_mu);
    for (auto& h : g_points.slots)      // (the guard's word comes home with the copies of every plan size with M points)
        if (h.device == dev && h.key.M == M) g_points.poll(h);
    auto* o = g_order.find(dev, OrderKey{M});
    if (!o) return PIGS_OK;
    g_order.poll(*o);
    info[0] = o->st.trusts(build_env().lattice_trust) ? 1 : 0;
    info[1] = o->st.trusted; info[2] = o->st.broken; info[3] = o->st.streak;
    return PIGS_OK;
}

static void fill_plan_args(BuildArgs& a, const PlanLayout& p, void* ws, float q_f, float q_b, const void* means,
                           const void* conics, const void* values) {
    char* b = (char*)ws;
    a.params = (PlanParams*)(b + p.off_params);
    a.counts = (uint32_t*)(b + p.off_counts);
    a.agg = (unsigned long long*)(b + p.off_agg);
    a.starts = (uint32_t*)(b + p.off_starts);
    a.gkey = (uint2*)(b + p.off_gkey);
    a.rec = (float4*)(b + p.off_rec);
    a.gbox = (float4*)(b + p.off_box);
    a.gacc = (float*)(b + p.off_gacc);
    a.g2o = (uint32_t*)(b + p.off_g2o);
    a.pbox = (float4*)(b + p.off_pbox);
    a.sbox = (float4*)(b + p.off_sbox);
    a.parea = (float*)(b + p.off_parea);
    a.means = (const float*)means; a.conics = (const float*)conics; a.values = (const float*)values;
    a.N = (uint32_t)p.N; a.c = p.c; a.G0 = p.G0; a.L = p.L;
    a.scan_blocks = p.scan_blocks;
    a.zero_words = (uint32_t)((p.off_starts - p.off_counts) / 4);
    for (int l = 0; l <= PLAN_MAX_LEVELS; ++l) a.level_off[l] = p.level_off[l];
    a.q_f = q_f; a.q_b = q_b;
    a.q_max = q_b > q_f ? q_b : q_f;
}

// ---- deferred tile lists (PIGS_BUILD_DEFER_LISTS) ----
// A plan built with the flag has everything but its tile lists; the first pigs_plan_forward / pigs_plan_backward /
// pigs_residual_* call on that workspace builds them -- a forward in the SAME launch (plan_lists_forward_kernel).
// Which workspaces are waiting is the library's to remember (the sampling entry points carry no flags): keyed by
// the workspace's address, set or cleared by every build into it, cleared by the first sampling call.
struct DeferredLists { float q_f, q_wide; };
static std::mutex g_defer_mu;
static std::unordered_map<const void*, DeferredLists> g_deferred;
static void defer_set(const void* ws, bool on, float q_f, float q_wide) {
    std::lock_guard<std::mutex> lock(g_defer_mu);
    if (on) g_deferred[ws] = DeferredLists{q_f, q_wide};
    else g_deferred.erase(ws);
}
static bool defer_take(const void* ws, DeferredLists& d) {
    std::lock_guard<std::mutex> lock(g_defer_mu);
    auto it = g_deferred.find(ws);
    if (it == g_deferred.end()) return false;
    d = it->second;
    g_deferred.erase(it);
    return true;
}

static ListArgs make_list_args(const PlanLayout& p, const SamplesLayout& s, void* ws, const void* sws, float q_f, float q_wide) {
    ListArgs la{};
    la.pv = make_view(p, ws, q_wide);
    la.q_f = q_f;
    la.sv = make_samples_view(s, sws);
    la.hdr = (uint32_t*)((char*)ws + p.off_hdr);
    la.tlist = (uint32_t*)((char*)ws + p.off_tlist);
    la.glist = (uint32_t*)((char*)ws + p.off_glist);
    la.ptiles = (uint32_t*)((char*)ws + p.off_ptiles);
    la.n_points = &((PlanParams*)((char*)ws + p.off_params))->n_points;
    la.points_wanted = &((PlanParams*)((char*)ws + p.off_params))->points_wanted;
    la.parea = (const float*)((char*)ws + p.off_parea);      // (run_build: null unless the build's statistics are wanted home)
    la.strip_cover = &((PlanParams*)((char*)ws + p.off_params))->strip_cover;
    la.product = lists_product_setting();
    la.through = store_through_setting();
    return la;
}
// the list launch (build_choice.h, list_launch); fwd_only: PIGS_BUILD_FORWARD_ONLY (build_block_lists<..., FWD_ONLY>)
// ... and la.through: headers and lists leave by write-through stores (plan.h, store_through) -- in the launch that was
// measured to gain by them, the forward-only build of more than LISTS_SMALL_TILES tiles (the cold step's).  Full plans
// and small point sets keep plain stores: one `--full` line each of parent and branch showed the training step and the
// c2 step no better or worse with them, and nothing there was measured twice.
static void launch_lists(const BuildLaunch& l, const ListArgs& la, hipStream_t stream, bool strips = false, bool fwd_only = false) {
    const bool small = l.kernel == K_LISTS_SMALL;
    const dim3 grid(l.grid), block(l.block);
    if (fwd_only) {
        if (small && strips) hipLaunchKernelGGL((plan_lists_kernel<1, true, true>), grid, block, 0, stream, la);
        else if (small) hipLaunchKernelGGL((plan_lists_kernel<1, false, true>), grid, block, 0, stream, la);
        else if (strips && la.through) hipLaunchKernelGGL((plan_lists_kernel<LISTS_TPW, true, true, true>), grid, block, 0, stream, la);
        else if (strips) hipLaunchKernelGGL((plan_lists_kernel<LISTS_TPW, true, true>), grid, block, 0, stream, la);
        else if (la.through) hipLaunchKernelGGL((plan_lists_kernel<LISTS_TPW, false, true, true>), grid, block, 0, stream, la);
        else hipLaunchKernelGGL((plan_lists_kernel<LISTS_TPW, false, true>), grid, block, 0, stream, la);
        return;
    }
    if (small && strips) hipLaunchKernelGGL((plan_lists_kernel<1, true>), grid, block, 0, stream, la);
    else if (small) hipLaunchKernelGGL((plan_lists_kernel<1, false>), grid, block, 0, stream, la);
    else if (strips) hipLaunchKernelGGL((plan_lists_kernel<LISTS_TPW, true>), grid, block, 0, stream, la);
    else hipLaunchKernelGGL((plan_lists_kernel<LISTS_TPW, false>), grid, block, 0, stream, la);
}

// The chain bbox -> count -> scan -> scatter for the samples (build_samples), the Gaussians (build_plan) or both in
// the same launches, then the tile lists.  Which launches: build_choice.h.
static int run_build(const BuildRequest& r, void* sws, size_t sws_bytes, void* ws, size_t ws_bytes, const void* means,
                     const void* conics, const void* values, const void* samples, hipStream_t stream) {
    // 1. what cannot be built
    if (!samples_supported(r.M)) return PIGS_ERR_UNSUPPORTED;
    const SamplesLayout s = make_samples_layout(r.M);
    if (!sws || sws_bytes < s.total_bytes) return PIGS_ERR_WORKSPACE;
    PlanLayout p{};
    if (r.do_plan) {
        if (!plan_supported(r.N, r.M, r.c)) return PIGS_ERR_UNSUPPORTED;
        if (!(r.q_max > 0.f)) return PIGS_ERR_INVALID;
        p = make_plan_layout(r.N, r.M, r.c);
        if (!ws || ws_bytes < p.total_bytes) return PIGS_ERR_WORKSPACE;
    }
    // 2. what the memories say, 3. which launches
    const BuildEnv env = build_env();
    const MemoryAnswer mem = ask_memories(r, env, stream);
    const BuildChoice b = choose_build(r, s, p, env, mem);
    // 4. the kernels' arguments
    BuildArgs a{};
    a.do_samples = r.do_samples; a.do_plan = r.do_plan; a.no_lookback = r.no_lookback;
    a.zero_gacc = !r.plan_ws_clean;
    fill_samples_args(a, s, sws, samples, b.coarse);
    if (r.do_plan) fill_plan_args(a, p, ws, r.q_max, b.q_max_b, means, conics, values);
    a.no_lattice = b.no_lattice; a.rf_hint = b.rf_hint; a.bbox_blocks = b.bbox_blocks; a.s_blocks = b.s_blocks;
    a.hint_axis = mem.axis;
    memcpy(a.hint_box, mem.box, sizeof(a.hint_box));
    a.fwd_only = b.fwd_only; a.ahead = b.ahead; a.s_scan_in_scatter = b.s_scan_in_scatter; a.sort_in_count = b.sort_in_count;
    a.strips = b.strips; a.trusted = b.trusted;
    const bool lists = r.do_plan && r.build_lists && !r.defer_lists;
    // Are this build's statistics due at home (PointsState::copy_due)?  Then the pack leaves its strips' areas, the list
    // launch sums them and stores every word that is not zero into the memory's slot itself (ListArgs::home).  With
    // PIGS_STATS_HOME=0 every build measures, as every build did, and a due one is followed by a copy.
    PointsMemory::Slot* due = lists ? points_due(p, stream, b.trusted) : nullptr;
    // (Deferred lists are built by the first sampling call, which knows nothing of this one: they measure every time and
    // keep the copy -- note_deferred_points.)
    const bool deferred = r.do_plan && r.build_lists && r.defer_lists;
    const bool measure = deferred || (lists && (due || !env.stats_home));
    if (!measure) a.parea = nullptr;
    ListArgs la{};
    if (lists) {
        la = make_list_args(p, s, ws, sws, r.q_max, a.q_max);
        if (!measure) la.parea = nullptr;
        if (due && env.stats_home) la.home = points_home(*due, b.strips);
        if (b.trusted) {      // the guard (plan_lists.h): every tile's real box against its share of the remembered one
            la.lattice_broken = &a.params->lattice_broken;
            const float rf = (float)a.rf_hint, rs = (float)(r.M / a.rf_hint);
            la.guard_n[0] = a.hint_axis ? rs : rf; la.guard_n[1] = a.hint_axis ? rf : rs;      // points along x / along y
            la.guard_e[0] = 16.f * (a.hint_box[2] - a.hint_box[0]) * 1.001f;
            la.guard_e[1] = 16.f * (a.hint_box[3] - a.hint_box[1]) * 1.001f;
        }
    }
    // 5. the launches, then a note for the next build of these sizes
    clear_hip_error();
    for (int i = 0; i < b.n; ++i) {
        const BuildLaunch& l = b.launches[i];
        const dim3 grid(l.grid), block(l.block);
        switch (l.kernel) {
            case K_SAMPLES_BBOX: hipLaunchKernelGGL(samples_bbox_kernel, grid, block, l.lds, stream, a); break;
            case K_PLAN_ZERO: hipLaunchKernelGGL(plan_zero_kernel, grid, block, l.lds, stream, a); break;
            case K_PLAN_COUNT: hipLaunchKernelGGL(plan_count_kernel, grid, block, l.lds, stream, a); break;
            case K_PLAN_SCAN: hipLaunchKernelGGL(plan_scan_kernel, grid, block, l.lds, stream, a); break;
            case K_PLAN_SCATTER: hipLaunchKernelGGL(plan_scatter_kernel, grid, block, l.lds, stream, a); break;
            case K_BINSORT_16: hipLaunchKernelGGL(samples_binsort_kernel<16>, grid, block, l.lds, stream, a); break;
            case K_BINSORT_1: hipLaunchKernelGGL(samples_binsort_kernel<1>, grid, block, l.lds, stream, a); break;
            case K_LISTS_SMALL:
            case K_LISTS: launch_lists(l, la, stream, b.strips, b.fwd_only); break;
        }
    }
    const int rc = launch_status();
    if (r.do_plan) defer_set(ws, r.build_lists && r.defer_lists && rc == PIGS_OK, r.q_max, a.q_max);
    if (due) note_points(*due, rc == PIGS_OK, la.home, p, ws, stream);
    if (rc != PIGS_OK) return rc;
    // (the samples header of a trusted build holds only what the build put there: nothing to ask for, one more to count)
    if (b.trusted || (r.do_samples && r.order == 0)) note_order(s, sws, stream, b.trusted);
    return rc;
}

// ---- the Gaussian grid alone, for the neighbour lists of aggregate_neighbors (aggregate.hip): the
// Gaussians' own centres play the sample points (they only size the grid's domain), no tile lists.
// Workspace = samples workspace (M = N) followed by a plan workspace (N, M = N, c = 1).
size_t aggregate_grid_bytes(int64_t N) {
    if (!plan_supported(N, N, 1)) return 0;
    return align_up(make_samples_layout(N).total_bytes, 256) + make_plan_layout(N, N, 1).total_bytes;
}

int aggregate_grid_build(void* ws, size_t ws_bytes, int64_t N, float q_grid, const float* means, const float* conics,
                         hipStream_t stream) {
    if (!plan_supported(N, N, 1)) return PIGS_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < aggregate_grid_bytes(N)) return PIGS_ERR_WORKSPACE;
    const size_t sb = align_up(make_samples_layout(N).total_bytes, 256);
    BuildRequest r;
    r.do_samples = r.do_plan = true; r.build_lists = false;
    r.N = r.M = N; r.c = 1; r.q_max = r.q_max_b = q_grid;
    // values: any N readable floats (the records' value slot is never read by the neighbour lists)
    return run_build(r, ws, sb, (char*)ws + sb, ws_bytes - sb, means, conics, means, means, stream);
}

// info[0] = byte offset of PlanParams::level_mask inside the grid workspace, info[1] = levels of the grid
void aggregate_grid_levels(int64_t N, int64_t* info) {
    const PlanLayout p = make_plan_layout(N, N, 1);
    info[0] = (int64_t)(align_up(make_samples_layout(N).total_bytes, 256) + p.off_params + offsetof(PlanParams, level_mask));
    info[1] = p.L;
}

PlanView aggregate_grid_view(void* ws, int64_t N, float q_grid) {
    const size_t sb = align_up(make_samples_layout(N).total_bytes, 256);
    return make_view(make_plan_layout(N, N, 1), (char*)ws + sb, q_grid);
}

int samples_build(void* sws, size_t sws_bytes, int64_t M, const void* samples, hipStream_t stream) {
    BuildRequest r;
    r.do_samples = true; r.M = M;
    return run_build(r, sws, sws_bytes, nullptr, 0, nullptr, nullptr, nullptr, samples, stream);
}

int plan_build(void* ws, size_t ws_bytes, void* sws, size_t sws_bytes, int flags, int64_t N, int64_t M, int c,
               float q_max, float q_max_backward, const void* means, const void* conics, const void* values, const void* samples,
               hipStream_t stream) {
    BuildRequest r;
    r.do_plan = true;
    r.do_samples = (flags & PIGS_BUILD_SAMPLES) != 0;
    r.plan_ws_clean = (flags & PIGS_BUILD_PLAN_WS_CLEAN) != 0;
    r.no_lookback = (flags & PIGS_BUILD_DEBUG_NO_LOOKBACK) != 0;
    r.order = (flags & PIGS_BUILD_POINTS_ORDERED) ? 1 : (flags & PIGS_BUILD_POINTS_UNORDERED) ? 2 : 0;
    r.defer_lists = (flags & PIGS_BUILD_DEFER_LISTS) != 0;
    r.fwd_only = (flags & PIGS_BUILD_FORWARD_ONLY) != 0;
    r.N = N; r.M = M; r.c = c; r.q_max = q_max; r.q_max_b = q_max_backward;
    return run_build(r, sws, sws_bytes, ws, ws_bytes, means, conics, values, samples, stream);
}

// a fused output whose coefficient block the caller left out (SampleArgs: terms, coupling, vort, fit)
static bool block_missing(int mask, const SampleArgs& a) {
    switch (mask) {
        case ORDG: return !a.terms;
        case ORDC: return !a.coupling;
        case ORDN: return !a.vort;
        case ORDF: return !a.fit;
        case ORDI:
        case ORDJ: return !a.net;
        default: return false;
    }
}

template <int C>
static int plan_forward_c(const PlanView& pv_in, const SamplesView& sv, int mask, float* const* out, const SampleArgs& a,
                          hipStream_t stream, const ListArgs* first) {
    // + the helper workgroups of the TILE_MODE_POINTS tiles (they leave at once when the plan queued none)
    const dim3 grid((sv.ntiles + PIGS_FWD_WG_WAVES - 1) / PIGS_FWD_WG_WAVES + POINT_HELPER_BLOCKS * 4 / PIGS_FWD_WG_WAVES),
        block(64 * PIGS_FWD_WG_WAVES);
    // points that arrive in no order send their outputs through the staging records (PlanView::stage)
    PlanView pv = pv_in;
    const bool staged = C == 1 && (mask == 7 || mask == 19) && points_unordered(sv.M, stream);
    if (!staged) pv.stage = nullptr;
    clear_hip_error();
    bool done = false;
    if (first) {
        // the plan's tile lists are still to be built (PIGS_BUILD_DEFER_LISTS): in this launch where a fused kernel
        // is compiled for the mask (instances.h), in a launch of their own in front of the forward otherwise
        ListArgs la = *first;
        la.pv.stage = pv.stage;
        const dim3 lgrid((sv.ntiles + 4 * LISTS_TPW - 1) / (4 * LISTS_TPW));
#define PIGS_FUSED(MK)                                                                                                  \
    case MK:                                                                                                            \
        hipLaunchKernelGGL((plan_lists_forward_kernel<C, MK>), lgrid, dim3(256), 0, stream, la, out[0], out[1], out[2], \
                           out[3], rz_of<float, MK>(a, false));                                                         \
        done = true;                                                                                                    \
        break;
        if (fused_first_compiled(C, mask) && !getenv("PIGS_NO_FUSED_FIRST") && !plan_expects_points(pv.N, sv.M, stream)) {
            if constexpr (C == 1) {
                switch (mask) { PIGS_FUSED_FIRST_C1_MASKS(PIGS_FUSED) }
            } else {
                switch (mask) { PIGS_FUSED_FIRST_C2_MASKS(PIGS_FUSED) }
            }
        }
#undef PIGS_FUSED
        if (!done) launch_lists(list_launch(sv.ntiles), la, stream);
    }
    if (block_missing(mask, a)) return PIGS_ERR_INVALID;
    // every compiled mask: the lists of instances.h (the fused outputs are never fused with the list launch, the linear residual apart)
#define PIGS_CASE(MK)                                                                                            \
    case MK:                                                                                                     \
        hipLaunchKernelGGL((tile_forward_kernel<C, MK>), grid, block, 0, stream, pv, sv, out[0], out[1], out[2], \
                           out[3], rz_of<float, MK>(a, false));                                                  \
        done = true;                                                                                             \
        break;
    if (!done) switch (mask) {
        PIGS_PLAIN_MASKS(PIGS_CASE)
        default: break;
    }
    // the vorticity terms and residual and the coupled residual: two channels, the only instantiations compiled
    if constexpr (C == 2) {
        switch (mask) {
            PIGS_BINNED_C2_MASKS(PIGS_CASE)
            PIGS_BINNED_FIT_MASKS(PIGS_CASE)
            default: break;
        }
    }
    // the network inputs: the forward-only list, each member for the channel counts network_instance names
#define PIGS_CASE_FORWARD(MK)                                                                                        \
    case MK:                                                                                                         \
        if constexpr (network_instance(2, C, MK)) {                                                                  \
            hipLaunchKernelGGL((tile_forward_kernel<C, MK>), grid, block, 0, stream, pv, sv, out[0], out[1], out[2], \
                               out[3], rz_of<float, MK>(a, false));                                                  \
            done = true;                                                                                             \
        }                                                                                                            \
        break;
    switch (mask) {
        PIGS_BINNED_NETWORK_MASKS(PIGS_CASE_FORWARD)
        default: break;
    }
#undef PIGS_CASE_FORWARD
#undef PIGS_CASE
    if (!done) return PIGS_ERR_UNSUPPORTED;
    if (staged) {
        const dim3 g2((sv.M + 255) / 256), b2(256);
        if (mask == 7) hipLaunchKernelGGL(stage_to_outputs_kernel<7>, g2, b2, 0, stream, pv.stage, sv.M, out[0], out[1], out[2]);
        else hipLaunchKernelGGL(stage_to_outputs_kernel<19>, g2, b2, 0, stream, pv.stage, sv.M, out[0], out[1], out[2]);
    }
    return launch_status();
}

template <int C>
static int plan_backward_c(const PlanView& pv_in, const SamplesView& sv, int mask, const float* const* g, const SampleArgs& a,
                           hipStream_t stream) {
    const dim3 grid((sv.ntiles + 3) / 4 + POINT_HELPER_BLOCKS), block(256);
    // points that arrive in no order fetch their incoming gradients from the staging records (PlanView::stage)
    PlanView pv = pv_in;
    const bool staged = C == 1 && (mask == 7 || mask == 19) && points_unordered(sv.M, stream);
    if (!staged) pv.stage = nullptr;
    clear_hip_error();
    if (staged) {
        const dim3 g2((sv.M + 255) / 256), b2(256);
        if (mask == 7) hipLaunchKernelGGL(gradients_to_stage_kernel<7>, g2, b2, 0, stream, pv.stage, sv.M, g[0], g[1], g[2]);
        else hipLaunchKernelGGL(gradients_to_stage_kernel<19>, g2, b2, 0, stream, pv.stage, sv.M, g[0], g[1], g[2]);
    }
    if (block_missing(mask, a)) return PIGS_ERR_INVALID;
    bool done = false;
#define PIGS_CASE(MK)                                                                                                \
    case MK:                                                                                                         \
        hipLaunchKernelGGL((tile_backward_kernel<C, MK>), grid, block, 0, stream, pv, sv, g[0], g[1], g[2], g[3],    \
                           rz_of<float, MK>(a, true));                                                               \
        done = true;                                                                                                 \
        break;
    switch (mask) {
        PIGS_PLAIN_MASKS(PIGS_CASE)
        default: break;
    }
    if constexpr (C == 2) {      // as in plan_forward_c
        switch (mask) {
            PIGS_BINNED_C2_MASKS(PIGS_CASE)
            PIGS_BINNED_FIT_MASKS(PIGS_CASE)
            default: break;
        }
    }
#undef PIGS_CASE
    if (!done) return PIGS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL((plan_unpermute_kernel<C>), dim3((pv.N + 255) / 256), dim3(256), 0, stream, pv, (float*)a.g_means,
                       (float*)a.g_conics, (float*)a.g_values);
    return launch_status();
}

int plan_forward(void* ws, size_t ws_bytes, const void* sws, size_t sws_bytes, float q_max, const SampleArgs& a,
                 hipStream_t stream) {
    if (!plan_supported(a.N, a.M, a.c)) return PIGS_ERR_UNSUPPORTED;
    const PlanLayout p = make_plan_layout(a.N, a.M, a.c);
    const SamplesLayout s = make_samples_layout(a.M);
    if (!ws || ws_bytes < p.total_bytes || !sws || sws_bytes < s.total_bytes) return PIGS_ERR_WORKSPACE;
    const PlanView pv = make_view(p, ws, q_max);
    const SamplesView sv = make_samples_view(s, sws);
    float* o[4];
    for (int k = 0; k < 4; ++k) o[k] = mask_uses_slot(a.orders_mask, k) ? (float*)a.out[k] : nullptr;
    const int cm = covering_mask_of(a.orders_mask);
    if (a.c != 1 && a.c != 2) return PIGS_ERR_UNSUPPORTED;
    DeferredLists d{};
    ListArgs la{};
    const bool first = defer_take(ws, d);
    if (first) la = make_list_args(p, s, ws, sws, d.q_f, d.q_wide);
    const int rc = a.c == 1 ? plan_forward_c<1>(pv, sv, cm, o, a, stream, first ? &la : nullptr)
                            : plan_forward_c<2>(pv, sv, cm, o, a, stream, first ? &la : nullptr);
    if (first && rc == PIGS_OK) note_deferred_points(p, ws, stream);
    return rc;
}

int plan_backward(void* ws, size_t ws_bytes, const void* sws, size_t sws_bytes, float q_max, const SampleArgs& a,
                  hipStream_t stream) {
    if (!plan_supported(a.N, a.M, a.c)) return PIGS_ERR_UNSUPPORTED;
    const PlanLayout p = make_plan_layout(a.N, a.M, a.c);
    const SamplesLayout s = make_samples_layout(a.M);
    if (!ws || ws_bytes < p.total_bytes || !sws || sws_bytes < s.total_bytes) return PIGS_ERR_WORKSPACE;
    const PlanView pv = make_view(p, ws, q_max);
    const SamplesView sv = make_samples_view(s, sws);
    {   // a backward as the first sampling call on a plan with deferred lists: the list launch first
        DeferredLists d{};
        if (defer_take(ws, d)) {
            clear_hip_error();
            launch_lists(list_launch(s.ntiles), make_list_args(p, s, ws, sws, d.q_f, d.q_wide), stream);
            const int rc = launch_status();
            if (rc != PIGS_OK) return rc;
            note_deferred_points(p, ws, stream);
        }
    }
    const float* g[4];
    for (int k = 0; k < 4; ++k) g[k] = mask_uses_slot(a.orders_mask, k) ? (const float*)a.gout[k] : nullptr;
    const int cm = covering_mask_of(a.orders_mask);
    switch (a.c) {
        case 1: return plan_backward_c<1>(pv, sv, cm, g, a, stream);
        case 2: return plan_backward_c<2>(pv, sv, cm, g, a, stream);
    }
    return PIGS_ERR_UNSUPPORTED;
}

}  // namespace pigs
