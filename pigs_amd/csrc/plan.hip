// Binned (culled) sampler: preprocess (samples build + plan build) + forward + backward, float32, d = 2.
// Data structures and the cut-off rule: plan.h.  Per-pair arithmetic: pair_math.h.
//
// One translation unit; the device code lies in four headers, by stage, each included here alone:
//   plan_build.h     samples build and the Gaussians' chain: bbox -> cell key + rank -> scan -> scatter
//   plan_lists.h     the tile lists: one wave walks the Gaussian grid once for four consecutive 64-point tiles
//   plan_forward.h   one wave = one tile; what forward and backward share, the forward, the fused list + forward launch
//   plan_backward.h  the backward over the tile lists, the way back to the caller's order
// This file: the host half -- workspaces, the library's memory of the last builds, launch policy, entry points.
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

constexpr int64_t LATTICE_MIN_POINTS = 1 << 12;
static void fill_samples_args(BuildArgs& a, const SamplesLayout& s, void* sws, const void* samples, bool coarse) {
    char* b = (char*)sws;
    a.sparams = (SampleParams*)(b + s.off_params);
    a.sboxes = (float4*)(b + s.off_boxes);
    a.slat = (float4*)(b + s.off_lat);
    {   // index-tiled order: from LATTICE_MIN_POINTS points on.  (Until the Gaussians ran one launch ahead -- BuildArgs::ahead
        // -- the bar stood at 2^18 points: detecting a lattice adds ~2.5 us to the first launch, sorting one costs ~1 us of
        // the count and scatter launches per 131 072 points.  A lattice that is expected now saves a whole launch: 128^2 ...
        // 384^2 grids, cold step -4 ... -5 us; BASELINE configs[1] 34.1 -> 31.5 us.)  PIGS_LATTICE=1 / 0: always / never
        const char* e = getenv("PIGS_LATTICE");
        a.no_lattice = e ? e[0] == '0' : s.M < LATTICE_MIN_POINTS;
    }
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

// ---- which way a samples build sorts its points (plan.h, SamplesLayout) ----
// Unordered points want the coarse-bin path, points in runs the one-pass build, and the host cannot look at
// the points without a synchronisation.  So every build of a large point set leaves {runs, points} of a sample
// of its waves in the workspace header, the library copies that pair to pinned memory on the build's stream
// behind the build (no wait), and the NEXT build of a point set of the same size on the same device takes what
// the last completed copy says: a training loop that draws new random collocation points every step
// (main_pn.py:103, test_no_mlp.py:86) switches after its first step or two, a lattice never does.  A capture
// neither asks nor copies (it keeps the mode of the moment).  PIGS_SAMPLES_ORDER = ordered | unordered in the
// environment, or the PIGS_BUILD_POINTS_* flags, overrule the memory; the result is the same either way
// (order inside a fine cell aside), only the time differs.
// Where the two mechanisms start to pay, measured on uniform random points with one Gaussian per 16 points (one box,
// cold step / forward launches / backward launches, us): 256^2 points: one-pass 49.1 / 18.7 / 19.1, coarse-bin 51.1,
// staged 23.0 / 22.4; 384^2: 61.1 vs 58.9 cold, staged forward 20.8 vs 14.3; 512^2: 70.8 vs 66.9 cold, staged
// 32.2 / 45.2 vs 30.4 / 39.5; 1024^2: 162 vs 122 cold, staged 49 / 104 vs 57 / 110.  Below ~100 k points the extra
// launch of the coarse-bin build costs more than the atomics it saves, and the staging launch more than the
// scattered sectors up to ~500 k.
constexpr int64_t COARSE_MIN_POINTS = 1 << 17;
constexpr int64_t STAGE_MIN_POINTS = 1 << 19;
struct OrderHint {
    int device = -1;
    int64_t M = 0;
    bool coarse = false, pending = false;
    uint32_t builds = 0;           // samples builds of this (device, M) so far: the statistic is asked for after the first
                                   // two and after every 16th (the 8-byte copy is a 4 us blit in the build's stream)
    hipEvent_t ev = nullptr;
    uint32_t* host = nullptr;      // pinned: the first 64 bytes of SampleParams (box, grid, order_stat, lat_cand, lat)
    uint32_t rf = 0;               // the row length of the last completed build when it took the index-tiled order (else 0)
    float box[4] = {0.f, 0.f, 0.f, 0.f};   // the samples' bounding box of the last completed build
    bool box_seen = false;         // ... and whether the completed build before it had the same one: a box to build the
    bool box_stable = false;       //     Gaussians' grid on before this build's own is known (BuildArgs::ahead)
    uint32_t same = 0;             // completed copies in a row that said the same (row length, box): the copies get rarer
    // TRUSTED builds (run_build): once the memory has held the same lattice for long enough, a build stops looking
    uint32_t axis = 0;             // the fast axis that goes with `rf` (SampleParams::lat_cand[1])
    uint32_t streak = 0;           // verified builds since a completed copy last said anything but (rf, box): builds between
                                   // two copies are taken on the word of the copies around them
    uint32_t trusted = 0;          // trusted builds of this (device, M) so far
    uint32_t broken = 0;           // times the list launch's guard turned this memory around (phint_poll)
    uint64_t stamp = 0;
};
constexpr uint32_t HINT_WORDS = 16;
// A build is trusted from this many verified builds in a row on: longer than any run of lattice builds after which the
// suite switches to other points of the same count and wants them noticed by the very next build
// (tests/test_lattice_gpu.py: 40), short next to a training run.
constexpr uint32_t TRUST_MIN_BUILDS = 64;
// PIGS_LATTICE_TRUST, read at every build: 0 = never (A/B: the verified chain), 1 = as soon as the memory holds a row
// length and a stable box (tests, tools/lattice_trust_worst_case.py); otherwise the memory decides (-1)
static int trust_mode() {
    const char* e = getenv("PIGS_LATTICE_TRUST");
    return !e ? -1 : e[0] == '0' ? 0 : e[0] == '1' ? 1 : -1;
}
static bool hint_trusts(const OrderHint& h) {      // g_hint_mu held; the samples' side of the conditions (run_build)
    const int mode = trust_mode();
    if (mode == 0 || h.rf == 0u || !h.box_stable) return false;
    return mode == 1 || (h.same >= 2u && h.streak >= TRUST_MIN_BUILDS);
}
static_assert(offsetof(SampleParams, box) == 0 && offsetof(SampleParams, order_stat) == 40 && offsetof(SampleParams, lat) == 56,
              "the hint copy: the first 64 bytes of SampleParams");
static std::mutex g_hint_mu;
static OrderHint g_hints[16];
static uint64_t g_hint_clock = 0;

static void hint_poll(OrderHint& h);
static OrderHint* hint_entry(int device, int64_t M, bool create) {      // g_hint_mu held; create: never inside a capture
    OrderHint* lru = nullptr;
    for (auto& h : g_hints) {
        if (h.device == device && h.M == M) { h.stamp = ++g_hint_clock; return &h; }
        if (!h.pending && (!lru || h.stamp < lru->stamp)) lru = &h;
    }
    if (!create) return nullptr;
    if (!lru) {
        // every slot waits for a copy (sizes that were built once and never came back): the copies have long
        // landed -- take note of them and give the least recently used slot away
        for (auto& h : g_hints) {
            hint_poll(h);
            if (!h.pending && (!lru || h.stamp < lru->stamp)) lru = &h;
        }
        if (!lru) return nullptr;
    }
    if (lru->ev && lru->device != device) {      // an event belongs to the device it was created on
        (void)hipEventDestroy(lru->ev);
        lru->ev = nullptr;
    }
    if (!lru->ev && hipEventCreateWithFlags(&lru->ev, hipEventDisableTiming) != hipSuccess) { lru->ev = nullptr; (void)hipGetLastError(); return nullptr; }
    if (!lru->host && hipHostMalloc((void**)&lru->host, HINT_WORDS * sizeof(uint32_t), hipHostMallocPortable) != hipSuccess) { lru->host = nullptr; (void)hipGetLastError(); return nullptr; }
    lru->device = device; lru->M = M; lru->coarse = false; lru->pending = false; lru->builds = 0; lru->rf = 0; lru->stamp = ++g_hint_clock;
    lru->box_seen = lru->box_stable = false; lru->same = 0;
    lru->axis = 0; lru->streak = 0; lru->trusted = 0; lru->broken = 0;
    return lru;
}

static bool stream_capturing(hipStream_t stream) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
    return st != hipStreamCaptureStatusNone;
}

static void hint_poll(OrderHint& h) {           // g_hint_mu held
    if (!h.pending) return;
    const hipError_t q = hipEventQuery(h.ev);
    (void)hipGetLastError();          // hipErrorNotReady is an answer, not a failure
    if (q == hipSuccess) {
        h.pending = false;
        const uint32_t rf_before = h.rf;
        h.rf = h.host[14];         // SampleParams::lat[0]
        h.axis = h.host[13];       // SampleParams::lat_cand[1]
        if (h.rf != 0u) h.coarse = false;      // index-tiled: the points arrived in order (and left no run statistic)
        else if (h.host[11] > 0u) h.coarse = (uint64_t)h.host[10] * 100u > (uint64_t)h.host[11] * 55u;
        float b[4];
        memcpy(b, h.host, sizeof(b));
        const bool finite = fabsf(b[0]) < 3.0e38f && fabsf(b[1]) < 3.0e38f && fabsf(b[2]) < 3.0e38f && fabsf(b[3]) < 3.0e38f && b[2] > b[0] && b[3] > b[1];
        h.box_stable = finite && h.box_seen && memcmp(b, h.box, sizeof(b)) == 0;
        h.same = h.box_stable && h.rf == rf_before ? h.same + 1u : 0u;
        if (h.rf == 0u || h.rf != rf_before || !h.box_stable) h.streak = 0u;
        h.box_seen = finite;
        memcpy(h.box, b, sizeof(b));
    }
}
// order: 0 = ask the memory, 1 = one pass, 2 = coarse bins
static bool samples_take_coarse(const SamplesLayout& s, int order, hipStream_t stream) {
    if (s.cells_per_bin > SAMPLES_MAX_CELLS_PER_BIN) return false;
    if (const char* e = getenv("PIGS_SAMPLES_ORDER")) {
        if (!strcmp(e, "ordered")) order = 1;
        else if (!strcmp(e, "unordered")) order = 2;
    }
    if (order) return order == 2;
    if (s.M < COARSE_MIN_POINTS) return false;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return false; }
    std::lock_guard<std::mutex> lock(g_hint_mu);
    OrderHint* h = hint_entry(dev, s.M, false);
    if (!h) return false;
    if (!stream_capturing(stream)) hint_poll(*h);
    return h->coarse;
}

// the row length the last completed build of M points found (index-tiled order), or 0
// *box_ok / box: the same box in the last two completed builds; *axis: the fast axis; *trust: the memory would let a build
// of this size go without looking at the points (never inside a capture)
static uint32_t samples_rf_hint(const SamplesLayout& s, hipStream_t stream, bool* box_ok = nullptr, float* box = nullptr,
                                uint32_t* axis = nullptr, bool* trust = nullptr) {
    if (box_ok) *box_ok = false;
    if (trust) *trust = false;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0u; }
    std::lock_guard<std::mutex> lock(g_hint_mu);
    OrderHint* h = hint_entry(dev, s.M, false);
    if (!h) return 0u;
    const bool cap = stream_capturing(stream);
    if (!cap) hint_poll(*h);
    if (box_ok && box && h->box_stable) { *box_ok = true; memcpy(box, h->box, 4 * sizeof(float)); }
    if (axis) *axis = h->axis;
    if (trust) *trust = !cap && hint_trusts(*h);
    return h->rf;
}
static void samples_note_trusted(const SamplesLayout& s) {      // behind a trusted build: nothing to ask for, one more to count
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return; }
    std::lock_guard<std::mutex> lock(g_hint_mu);
    if (OrderHint* h = hint_entry(dev, s.M, false)) ++h->trusted;
}

// behind a samples build: ask for its {runs, points}
static void samples_note_order(const SamplesLayout& s, void* sws, hipStream_t stream) {
    if (s.M < 64) return;          // (the same record carries the lattice row length: wanted for every size)
    if (stream_capturing(stream)) return;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return; }
    std::lock_guard<std::mutex> lock(g_hint_mu);
    OrderHint* h = hint_entry(dev, s.M, true);
    if (!h) return;
    const uint32_t nth = h->builds++;
    if (h->rf != 0u) ++h->streak;
    // (with a row length in the memory the build runs on expectations -- an eighth of the count's workgroups, the
    // Gaussians one launch ahead -- and a point set that stopped meeting them should not be met 15 more times: every 8th
    // build then; the copy is a ~4 us blit in the build's stream)
    // ... every 32nd once three copies in a row have said the same)
    if (h->pending || (nth >= 2u && (nth & (h->rf ? (h->same >= 2u ? 31u : 7u) : 15u)) != 0u)) return;
    const SampleParams* sp = (const SampleParams*)((const char*)sws + s.off_params);
    if (hipMemcpyAsync(h->host, sp, HINT_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream) == hipSuccess &&
        hipEventRecord(h->ev, stream) == hipSuccess)
        h->pending = true;
    (void)hipGetLastError();
}

// The sampling launches' question (staging, PlanView::stage): did the point set of this size arrive in no order?
// A pending statistic is looked at here too -- a point set that is built once and sampled many times (fixed random
// collocation points) never comes back to samples_take_coarse -- unless the stream is being captured.
static bool points_unordered(int64_t M, hipStream_t stream) {
    if (const char* e = getenv("PIGS_STAGE")) return e[0] == '1';          // tests / A-B runs: staging on or off whatever the memory and the size
    if (M < STAGE_MIN_POINTS) return false;
    if (const char* e = getenv("PIGS_SAMPLES_ORDER")) return !strcmp(e, "unordered");
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return false; }
    const bool cap = stream_capturing(stream);
    std::lock_guard<std::mutex> lock(g_hint_mu);
    for (auto& h : g_hints)
        if (h.device == dev && h.M == M) {
            if (!cap) hint_poll(h);
            return h.coarse;
        }
    return false;
}

int samples_order_hint(int64_t M) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return -1; }
    std::lock_guard<std::mutex> lock(g_hint_mu);
    OrderHint* h = hint_entry(dev, M, false);
    if (!h) return -1;
    hint_poll(*h);
    return h->coarse ? 1 : 0;
}

static void phint_poll_size(int device, int64_t M);
int samples_trust_info(int64_t M, int64_t* info) {
    info[0] = info[1] = info[2] = info[3] = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return PIGS_OK; }
    std::lock_guard<std::mutex> lock(g_hint_mu);
    phint_poll_size(dev, M);           // (the guard's word comes home with the plans' copies)
    OrderHint* h = hint_entry(dev, M, false);
    if (!h) return PIGS_OK;
    hint_poll(*h);
    info[0] = hint_trusts(*h) ? 1 : 0;
    info[1] = h->trusted; info[2] = h->broken; info[3] = h->streak;
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
// ---- does a plan of these sizes hold tiles in TILE_MODE_POINTS? ----
// The fused first forward walks such tiles in their own list wave (right, and slow when there are hundreds: the
// thin outskirts of a clustered cloud), the two-launch path spreads them over helper workgroups.  Which one a plan
// wants is known on the device only, so -- like the order of the points (OrderHint above) -- the library remembers,
// per device and (N, M): behind the list build of the first two plans of a size and of every 16th, PlanParams::
// n_points is copied to pinned memory on the build's stream (nobody waits); a first forward takes the fused launch
// unless the last completed copy for its sizes showed such tiles.  Never inside a capture.
constexpr float STRIP_MAX_COVER = 64.f;      // (plan_takes_strips below)
struct PointsHint {
    int device = -1;
    int64_t N = 0, M = 0;
    bool has_points = false, pending = false;
    float cover = -1.f;            // PlanParams::strip_cover of the last completed build (< 0: none yet)
    bool strips = false;           // ... and whether that build kept the caller's order
    uint32_t same = 0;             // completed copies in a row that led to the same choice: the copies get rarer
    uint32_t builds = 0;
    hipEvent_t ev = nullptr;
    uint32_t* host = nullptr;      // pinned {n_points, strip_cover, strips, points_wanted, lattice_broken}
    uint64_t stamp = 0;
};
constexpr uint32_t PHINT_WORDS = 5;
static_assert(offsetof(PlanParams, strip_cover) == offsetof(PlanParams, n_points) + 4 && offsetof(PlanParams, strips) == offsetof(PlanParams, n_points) + 8 &&
              offsetof(PlanParams, points_wanted) == offsetof(PlanParams, n_points) + 12 && offsetof(PlanParams, lattice_broken) == offsetof(PlanParams, n_points) + 16,
              "one copy: n_points, strip_cover, strips, points_wanted, lattice_broken");
static PointsHint g_phints[16];
static void phint_poll(PointsHint& h) {          // g_hint_mu held
    if (!h.pending) return;
    const hipError_t q = hipEventQuery(h.ev);
    (void)hipGetLastError();
    if (q == hipSuccess) {
        h.pending = false;
        const bool took_before = h.cover >= 0.f && h.cover <= STRIP_MAX_COVER && !h.has_points;
        h.has_points = h.host[0] != 0u || h.host[3] != 0u;
        memcpy(&h.cover, &h.host[1], sizeof(float));
        if (!(h.cover >= 0.f)) h.cover = 3.0e38f;      // NaN: as bad as it gets
        h.strips = h.host[2] != 0u;
        h.same = (h.cover <= STRIP_MAX_COVER && !h.has_points) == took_before ? h.same + 1u : 0u;
        if (h.host[4] != 0u) {
            // a trusted build met points that are no compact lattice in the remembered order (plan_lists.h, the guard): the
            // samples' memory of this size turns around -- the next build searches, verifies and, if need be, sorts, as
            // a first build does
            if (OrderHint* o = hint_entry(h.device, h.M, false)) {
                o->rf = 0u; o->same = 0u; o->box_stable = false; o->streak = 0u;
                ++o->broken;
            }
        }
    }
}
static void phint_poll_size(int device, int64_t M) {      // g_hint_mu held: every plan size with M points
    for (auto& h : g_phints)
        if (h.device == device && h.M == M) phint_poll(h);
}
static PointsHint* phint_entry(int device, int64_t N, int64_t M, bool create) {      // g_hint_mu held
    PointsHint* lru = nullptr;
    for (auto& h : g_phints) {
        if (h.device == device && h.N == N && h.M == M) { h.stamp = ++g_hint_clock; return &h; }
        if (!h.pending && (!lru || h.stamp < lru->stamp)) lru = &h;
    }
    if (!create) return nullptr;
    if (!lru) {
        for (auto& h : g_phints) {
            phint_poll(h);
            if (!h.pending && (!lru || h.stamp < lru->stamp)) lru = &h;
        }
        if (!lru) return nullptr;
    }
    if (lru->ev && lru->device != device) { (void)hipEventDestroy(lru->ev); lru->ev = nullptr; }
    if (!lru->ev && hipEventCreateWithFlags(&lru->ev, hipEventDisableTiming) != hipSuccess) { lru->ev = nullptr; (void)hipGetLastError(); return nullptr; }
    if (!lru->host && hipHostMalloc((void**)&lru->host, PHINT_WORDS * sizeof(uint32_t), hipHostMallocPortable) != hipSuccess) { lru->host = nullptr; (void)hipGetLastError(); return nullptr; }
    lru->device = device; lru->N = N; lru->M = M; lru->has_points = false; lru->pending = false; lru->builds = 0; lru->stamp = ++g_hint_clock;
    lru->cover = -1.f; lru->strips = false; lru->same = 0;
    return lru;
}
static bool plan_expects_points(int64_t N, int64_t M, hipStream_t stream) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return false; }
    const bool cap = stream_capturing(stream);
    std::lock_guard<std::mutex> lock(g_hint_mu);
    PointsHint* h = phint_entry(dev, N, M, false);
    if (!h) return false;
    if (!cap) phint_poll(*h);
    return h->has_points;
}
// Does the next build of these sizes keep the caller's order (PlanParams::strips)?  Yes when the last completed build's
// strips covered the samples' domain at most STRIP_MAX_COVER times -- that number is about how many strips a block of
// tiles meets (a lattice in row order, a strip of 1 x 16 widened by its ellipses' reach on every side: ~10 times at
// kappa = 0.5, ~17 at 0.8, ~33 at 1.3; Gaussians in no order: every strip covers the domain, N / 16 times).
// PIGS_GAUSS_STRIPS=0 / 1: never / always.
constexpr int64_t STRIP_MIN_GAUSSIANS = 1024;      // (below, the chain it replaces is not what a step waits for)
static bool plan_takes_strips(int64_t N, int64_t M, hipStream_t stream) {
    if (const char* e = getenv("PIGS_GAUSS_STRIPS")) return e[0] == '1';
    // (a build that also sorts or looks at the samples saves no launch by it -- the Gaussians' count, scan and scatter ride
    // along in launches that exist anyway -- but the lists from strips are the faster ones since the survivors wait for a
    // full buffer: 20.0 against 21.3 us at C3, 55 against 60 at kappa 1.3, and the scan / scatter launches carry less)
    if (N < STRIP_MIN_GAUSSIANS) return false;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return false; }
    const bool cap = stream_capturing(stream);
    std::lock_guard<std::mutex> lock(g_hint_mu);
    PointsHint* h = phint_entry(dev, N, M, false);
    if (!h) return false;
    if (!cap) phint_poll(*h);
    // (tiles of far-apart points -- a cloud's thin outskirts -- are walked point by point through the GRID at sampling
    // time, TILE_MODE_POINTS: a plan that had such tiles keeps the cells.  Measured without this line: clamped normals
    // sigma = 0.15 over lattice Gaussians, warm step 111 -> 1 126 us.)
    return h->cover >= 0.f && h->cover <= STRIP_MAX_COVER && !h->has_points;
}
// trusted: the build took the samples' lattice on trust (run_build) -- its guard's word is wanted home soon
static void plan_note_points(const PlanLayout& p, const void* ws, hipStream_t stream, bool trusted = false) {      // behind a list build
    if (stream_capturing(stream)) return;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return; }
    std::lock_guard<std::mutex> lock(g_hint_mu);
    PointsHint* h = phint_entry(dev, p.N, p.M, true);
    if (!h) return;
    const uint32_t nth = h->builds++;
    // (builds that keep the caller's order run on an expectation -- strips that cover the domain a few times over -- and
    // Gaussians that stopped meeting it should not be met 15 more times)
    // ... and points that stopped being the lattice a trusted build takes them for not 31 more times either: every 8th)
    if (h->pending || (nth >= 2u && (nth & (trusted ? 7u : h->strips ? (h->same >= 2u ? 31u : 7u) : 15u)) != 0u)) return;
    const PlanParams* pp = (const PlanParams*)((const char*)ws + p.off_params);
    if (hipMemcpyAsync(h->host, &pp->n_points, PHINT_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream) == hipSuccess &&
        hipEventRecord(h->ev, stream) == hipSuccess)
        h->pending = true;
    (void)hipGetLastError();
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
    la.parea = (const float*)((char*)ws + p.off_parea);
    la.strip_cover = &((PlanParams*)((char*)ws + p.off_params))->strip_cover;
    return la;
}
// Small point sets (a list launch of fewer tiles than this is one sparse generation of waves): one tile per wave.
constexpr uint32_t LISTS_SMALL_TILES = 4096;
// fwd_only: PIGS_BUILD_FORWARD_ONLY (build_block_lists<..., FWD_ONLY>)
static void launch_lists(uint32_t ntiles, const ListArgs& la, hipStream_t stream, bool strips = false, bool fwd_only = false) {
    const bool small = ntiles <= LISTS_SMALL_TILES && LISTS_TPW != 1;
    const dim3 grid(small ? (ntiles + 3) / 4 : (ntiles + 4 * LISTS_TPW - 1) / (4 * LISTS_TPW));
    if (fwd_only) {
        if (small && strips) hipLaunchKernelGGL((plan_lists_kernel<1, true, true>), grid, dim3(256), 0, stream, la);
        else if (small) hipLaunchKernelGGL((plan_lists_kernel<1, false, true>), grid, dim3(256), 0, stream, la);
        else if (strips) hipLaunchKernelGGL((plan_lists_kernel<LISTS_TPW, true, true>), grid, dim3(256), 0, stream, la);
        else hipLaunchKernelGGL((plan_lists_kernel<LISTS_TPW, false, true>), grid, dim3(256), 0, stream, la);
        return;
    }
    if (small && strips) hipLaunchKernelGGL((plan_lists_kernel<1, true>), grid, dim3(256), 0, stream, la);
    else if (small) hipLaunchKernelGGL((plan_lists_kernel<1, false>), grid, dim3(256), 0, stream, la);
    else if (strips) hipLaunchKernelGGL((plan_lists_kernel<LISTS_TPW, true>), grid, dim3(256), 0, stream, la);
    else hipLaunchKernelGGL((plan_lists_kernel<LISTS_TPW, false>), grid, dim3(256), 0, stream, la);
}

// The chain bbox -> count -> scan -> scatter for the samples (build_samples), the Gaussians
// (build_plan) or both in the same four launches, then the tile lists.
static int run_build(bool do_samples, bool do_plan, bool plan_ws_clean, bool no_lookback, void* sws, size_t sws_bytes, void* ws, size_t ws_bytes, int64_t N,
                     int64_t M, int c, float q_max, float q_max_b, const void* means, const void* conics, const void* values,
                     const void* samples, hipStream_t stream, bool build_lists = true, int order = 0, bool defer_lists = false,
                     bool fwd_only = false) {
    if (!samples_supported(M)) return PIGS_ERR_UNSUPPORTED;
    const SamplesLayout s = make_samples_layout(M);
    if (!sws || sws_bytes < s.total_bytes) return PIGS_ERR_WORKSPACE;
    BuildArgs a{};
    a.do_samples = do_samples; a.do_plan = do_plan; a.no_lookback = no_lookback;
    a.zero_gacc = !plan_ws_clean;
    const bool coarse = do_samples && samples_take_coarse(s, order, stream);
    fill_samples_args(a, s, sws, samples, coarse);
    bool box_ok = false, trust = false;
    a.rf_hint = do_samples ? samples_rf_hint(s, stream, &box_ok, a.hint_box, &a.hint_axis, &trust) : 0u;
    {
        static const char* e = getenv("PIGS_BBOX_BLOCKS");      // (A/B: 256 | 512)
        // same box, 1024^2 points: the plain pass 6.6 -> 5.9 us with 512 workgroups, the pass with a row length 7.5 -> 7.8
        a.bbox_blocks = e ? (uint32_t)atoi(e) : (M >= (int64_t)BBOX_WIDE_POINTS && a.rf_hint == 0u ? 512u : 256u);
        if (a.bbox_blocks != 512u) a.bbox_blocks = 256u;
    }
    PlanLayout p{};
    if (do_plan) {
        if (!plan_supported(N, M, c)) return PIGS_ERR_UNSUPPORTED;
        if (!(q_max > 0.f)) return PIGS_ERR_INVALID;
        if (!(q_max_b >= q_max)) q_max_b = q_max;      // <= 0 / NaN: one cut-off
        // a plan for the forward alone is sized with the forward's cut-off throughout (boxes, levels, strips, the walk)
        fwd_only = fwd_only && build_lists && !defer_lists;
        if (fwd_only) q_max_b = q_max;
        p = make_plan_layout(N, M, c);
        if (!ws || ws_bytes < p.total_bytes) return PIGS_ERR_WORKSPACE;
        fill_plan_args(a, p, ws, q_max, q_max_b, means, conics, values);
        a.fwd_only = fwd_only;
    }
    clear_hip_error();
    const uint32_t gb = do_plan ? (uint32_t)((N + 255) / 256) : 0u;
    // The Gaussians one launch ahead (BuildArgs::ahead): a lattice is expected, the samples' box was the same in the last
    // two completed builds of this size, the plan workspace's counters are zero.
    static const bool no_ahead = getenv("PIGS_NO_AHEAD") != nullptr;
    const bool ahead = do_samples && do_plan && plan_ws_clean && !coarse && !no_lookback && !no_ahead &&
                       a.rf_hint != 0u && !a.no_lattice && box_ok && s.scan_blocks <= 1024u;
    a.ahead = ahead; a.s_scan_in_scatter = ahead;
    // Gaussians whose order in the caller's array is already spatial keep it (PlanParams::strips): one pass instead of
    // count, scan and scatter
    const bool strips = do_plan && build_lists && !defer_lists && !no_lookback &&
                        plan_takes_strips(N, M, stream);
    a.strips = strips;
    // TRUSTED: point sets of this size have been the same compact lattice for TRUST_MIN_BUILDS verified builds and three
    // copies in a row -- this build does not look again.  It launches what a build on a finished samples workspace
    // launches, the Gaussians' pack and the lists; the pack's first workgroup writes the samples header the decision
    // would have written, the list launch reads the points through it and holds every tile's real box against the
    // remembered one (ListArgs::lattice_broken), and that word rides home with the plan's statistics every 8th build
    // (phint_poll turns the memory around).  Results never depend on it: the lists come from the groups' real boxes.
    const bool trusted = ahead && strips && trust && order == 0 && a.rf_hint >= 8u && (a.rf_hint & 7u) == 0u && M >= 64 && M % a.rf_hint == 0 &&
                         ((M / a.rf_hint) & 7) == 0;
    if (trusted) {
        a.trusted = 1; a.ahead = 0; a.s_scan_in_scatter = 0;
        hipLaunchKernelGGL(plan_count_kernel, dim3(gb), dim3(256), 0, stream, a);
    } else if (ahead && strips) {
        // nothing of the Gaussians is left for launches 2 and 3: the samples' fall-back moves into launch 2 whole
        // (samples_sort_in_count; at most 256 workgroups: they meet at device-wide barriers) -- FOUR launches up to the forward
        a.sort_in_count = 1; a.s_scan_in_scatter = 0;
        a.s_blocks = (uint32_t)((M + 1023) / 1024);
        const uint32_t swgs = (a.s_blocks + 7u) / 8u < 256u ? (a.s_blocks + 7u) / 8u : 256u;
        hipLaunchKernelGGL(samples_bbox_kernel, dim3(a.bbox_blocks + gb), dim3(BBOX_THREADS), 0, stream, a);
        hipLaunchKernelGGL(plan_count_kernel, dim3(swgs), dim3(256), 0, stream, a);
    } else if (ahead) {
        a.s_blocks = (uint32_t)((M + 1023) / 1024);
        hipLaunchKernelGGL(samples_bbox_kernel, dim3(a.bbox_blocks + gb), dim3(BBOX_THREADS), 0, stream, a);
        hipLaunchKernelGGL(plan_count_kernel, dim3(p.scan_blocks + (a.s_blocks + 7u) / 8u), dim3(256), 0, stream, a);
        hipLaunchKernelGGL(plan_scatter_kernel, dim3(gb + (uint32_t)((M + 255) / 256)), dim3(256), 0, stream, a);
    } else
    if (do_samples) hipLaunchKernelGGL(samples_bbox_kernel, dim3(a.bbox_blocks), dim3(BBOX_THREADS), 0, stream, a);
    else if (!plan_ws_clean) hipLaunchKernelGGL(plan_zero_kernel, dim3(64), dim3(256), 0, stream, a);
    if (ahead) {
        // (launched above)
    } else {
        // a lattice expected (the row length of the last build of this size): an eighth of the one-pass count's workgroups
        // -- they leave at once when the points are index-tiled, and stride over the blocks when they are not
        a.s_blocks = (uint32_t)((M + 1023) / 1024);
        const uint32_t count_wgs = coarse ? s.h_wgs : (a.rf_hint && !a.no_lattice ? (a.s_blocks + 7u) / 8u : a.s_blocks);
        hipLaunchKernelGGL(plan_count_kernel, dim3(gb + (do_samples ? count_wgs : 0u)), dim3(256), 0, stream, a);
        const uint32_t scan_wgs = (do_plan && !strips ? p.scan_blocks : 0u) + (do_samples ? a.s_scan_blocks : 0u);
        if (scan_wgs) hipLaunchKernelGGL(plan_scan_kernel, dim3(scan_wgs), dim3(256), 0, stream, a);
        const bool staged = coarse && s.h_chunk <= SCATTER_STAGE_MAX;
        const uint32_t scatter_wgs = (strips ? 0u : gb) + (do_samples ? (staged ? s.h_wgs : (uint32_t)((M + 255) / 256)) : 0u);
        if (scatter_wgs)
            hipLaunchKernelGGL(plan_scatter_kernel, dim3(scatter_wgs), dim3(256),
                               staged ? s.h_chunk * sizeof(uint4) + 2 * SAMPLES_COARSE_BINS * sizeof(uint32_t) : 0, stream, a);
        if (coarse) {
            if (s.cells_per_bin * 16u <= SAMPLES_MAX_CELLS_PER_BIN)      // the LDS holds 16 sub-cell counters per cell
                hipLaunchKernelGGL(samples_binsort_kernel<16>, dim3(SAMPLES_COARSE_BINS), dim3(1024),
                                   s.cells_per_bin * 16u * sizeof(uint32_t), stream, a);
            else
                hipLaunchKernelGGL(samples_binsort_kernel<1>, dim3(SAMPLES_COARSE_BINS), dim3(1024),
                                   s.cells_per_bin * sizeof(uint32_t), stream, a);
        }
    }
    if (do_plan && build_lists && !defer_lists) {
        ListArgs la = make_list_args(p, s, ws, sws, q_max, a.q_max);
        if (trusted) {
            la.lattice_broken = &a.params->lattice_broken;
            const float rf = (float)a.rf_hint, rs = (float)(M / a.rf_hint);
            la.guard_n[0] = a.hint_axis ? rs : rf; la.guard_n[1] = a.hint_axis ? rf : rs;      // points along x / along y
            la.guard_e[0] = 16.f * (a.hint_box[2] - a.hint_box[0]) * 1.001f;
            la.guard_e[1] = 16.f * (a.hint_box[3] - a.hint_box[1]) * 1.001f;
        }
        launch_lists(s.ntiles, la, stream, strips, fwd_only);
    }
    const int rc = launch_status();
    if (do_plan) defer_set(ws, build_lists && defer_lists && rc == PIGS_OK, q_max, a.q_max);
    if (do_plan && build_lists && !defer_lists && rc == PIGS_OK) plan_note_points(p, ws, stream, trusted);
    if (trusted) {      // (the samples header holds only what this build put there: nothing to ask for)
        if (rc == PIGS_OK) samples_note_trusted(s);
    } else if (do_samples && rc == PIGS_OK && order == 0) samples_note_order(s, sws, stream);
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
    // values: any N readable floats (the records' value slot is never read by the neighbour lists)
    return run_build(true, true, false, false, ws, sb, (char*)ws + sb, ws_bytes - sb, N, N, 1, q_grid, q_grid, means, conics,
                     means, means, stream, false);
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
    return run_build(true, false, false, false, sws, sws_bytes, nullptr, 0, 0, M, 1, 1.f, 1.f, nullptr, nullptr, nullptr, samples, stream);
}

int plan_build(void* ws, size_t ws_bytes, void* sws, size_t sws_bytes, int flags, int64_t N, int64_t M, int c,
               float q_max, float q_max_backward, const void* means, const void* conics, const void* values, const void* samples,
               hipStream_t stream) {
    return run_build((flags & 1) != 0, true, (flags & 2) != 0, (flags & 4) != 0, sws, sws_bytes, ws, ws_bytes, N, M, c, q_max, q_max_backward, means, conics, values,
                     samples, stream, true, (flags & 8) ? 1 : (flags & 16) ? 2 : 0, (flags & PIGS_BUILD_DEFER_LISTS) != 0,
                     (flags & PIGS_BUILD_FORWARD_ONLY) != 0);
}

// the masks the fused first forward is compiled for (the rest: the list launch, then the forward launch)
template <int C> static bool fused_first_compiled(int mask) { return C == 1 ? (mask == 1 || mask == 7 || mask == 19 || mask == 32) : mask == 7; }

// a fused output whose coefficient block the caller left out (SampleArgs: terms, coupling, vort)
static bool block_missing(int mask, const SampleArgs& a) {
    switch (mask) {
        case ORDG: return !a.terms;
        case ORDC: return !a.coupling;
        case ORDN: return !a.vort;
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
        // is compiled for the mask, in a launch of their own in front of the forward otherwise
        ListArgs la = *first;
        la.pv.stage = pv.stage;
        const dim3 lgrid((sv.ntiles + 4 * LISTS_TPW - 1) / (4 * LISTS_TPW));
#define PIGS_FUSED(MK)                                                                                                  \
    case MK:                                                                                                            \
        hipLaunchKernelGGL((plan_lists_forward_kernel<C, MK>), lgrid, dim3(256), 0, stream, la, out[0], out[1], out[2], \
                           out[3], rz_of<float, MK>(a, false));                                                         \
        done = true;                                                                                                    \
        break;
        if (fused_first_compiled<C>(mask) && !getenv("PIGS_NO_FUSED_FIRST") && !plan_expects_points(pv.N, sv.M, stream)) {
            if constexpr (C == 1) {
                switch (mask) { PIGS_FUSED(1) PIGS_FUSED(7) PIGS_FUSED(19) PIGS_FUSED(32) }
            } else {
                switch (mask) { PIGS_FUSED(7) }
            }
        }
#undef PIGS_FUSED
        if (!done) launch_lists(sv.ntiles, la, stream);
    }
    if (block_missing(mask, a)) return PIGS_ERR_INVALID;
    // every compiled mask (the fused outputs are never fused with the list launch, the linear residual apart)
#define PIGS_CASE(MK)                                                                                            \
    case MK:                                                                                                     \
        hipLaunchKernelGGL((tile_forward_kernel<C, MK>), grid, block, 0, stream, pv, sv, out[0], out[1], out[2], \
                           out[3], rz_of<float, MK>(a, false));                                                  \
        done = true;                                                                                             \
        break;
    if (!done) switch (mask) {
        PIGS_CASE(1) PIGS_CASE(2) PIGS_CASE(4) PIGS_CASE(8) PIGS_CASE(7) PIGS_CASE(15) PIGS_CASE(16) PIGS_CASE(19)
        PIGS_CASE(ORDR) PIGS_CASE(ORDG)
        default: break;
    }
    // the vorticity terms and residual and the coupled residual: two channels, the only instantiations compiled
    if constexpr (C == 2) {
        switch (mask) {
            PIGS_CASE(ORDV) PIGS_CASE(ORDC) PIGS_CASE(ORDN)
            default: break;
        }
    }
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
        PIGS_CASE(1) PIGS_CASE(2) PIGS_CASE(4) PIGS_CASE(8) PIGS_CASE(7) PIGS_CASE(15) PIGS_CASE(16) PIGS_CASE(19)
        PIGS_CASE(ORDR) PIGS_CASE(ORDG)
        default: break;
    }
    if constexpr (C == 2) {      // as in plan_forward_c
        switch (mask) {
            PIGS_CASE(ORDV) PIGS_CASE(ORDC) PIGS_CASE(ORDN)
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
    if (first && rc == PIGS_OK) plan_note_points(p, ws, stream);
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
            launch_lists(s.ntiles, make_list_args(p, s, ws, sws, d.q_f, d.q_wide), stream);
            const int rc = launch_status();
            if (rc != PIGS_OK) return rc;
            plan_note_points(p, ws, stream);
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
