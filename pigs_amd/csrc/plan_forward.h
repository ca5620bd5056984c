// Binned sampler, sampling kernels: what forward and backward share (records, the per-point walk, the steps
// through a tile's lists) and the forward.  Included by plan.hip alone.
//
// Sampling kernels: one wave = one tile of 64 consecutive sorted points (lane = point), one DPP row =
// one 16-point group.  Forward: every row streams its own group list, gathers the 32-byte records
// into its LDS queue and the rows are evaluated together -- in one instruction every row works on
// its OWN Gaussian, read from LDS with a row-uniform address.  No workgroup barriers;
// HBM traffic is the point stream (sorted points in, outputs out through the points' original
// indices) plus list and record reads that mostly hit L2.
// Build-time knobs: PIGS_FWD_WAVES, PIGS_FWD_WG_WAVES, PIGS_FWD_UNROLL, PIGS_GROUP_CAP.
#pragma once
#include "plan_lists.h"

#ifndef PIGS_FWD_WAVES
#define PIGS_FWD_WAVES 8      // waves per SIMD the forward kernel's register budget is held to
#endif
#ifndef PIGS_FWD_WG_WAVES
#define PIGS_FWD_WG_WAVES 4   // waves (= tiles) per workgroup of the forward kernel
#endif
#ifndef PIGS_FWD_UNROLL
#define PIGS_FWD_UNROLL 2     // list rows evaluated per loop iteration
#endif

namespace pigs {

// ------------------------------------------------------------------------------------------
// Sampling kernels.  One wave = one tile.
// ------------------------------------------------------------------------------------------
struct Rec {
    float mu[2], con[3], v[2];
};

// TILE_MODE_POINTS: this lane's own walk of the Gaussian grid around the point (x, y): in every occupied
// level the 3 x 3 cells around the point's cell hold every Gaussian of that level whose q <= cut ellipse can
// contain the point (a Gaussian lives in the lowest level whose cell side covers its ellipse's half extent;
// out-of-domain coordinates clamp the same monotone way the build binned them).  `body(j, A, B)` gets the
// sorted index and the record of every candidate; lanes run their own trip counts.
template <int STRIDE, typename Body>      // the lanes i = 0 .. STRIDE-1 of a point share its candidates: lane i takes j0 + i, j0 + i + STRIDE, ...
__device__ __forceinline__ void walk_point(const PlanView& pv, float x, float y, int i, Body&& body) {
    const GaussGrid gg = pv.params->gg;
    const uint32_t level_mask = pv.params->level_mask;
    for (int l = 0; l < pv.L; ++l) {
        if (!(level_mask >> l & 1u)) continue;
        const int G = pv.G0 >> l;
        const float inv_s = gg.inv_s0 * __builtin_amdgcn_ldexpf(1.f, -l);
        const float gmax = (float)(G - 1);
        const int cx = (int)clampf(floorf((x - gg.ox) * inv_s), 0.f, gmax);
        const int cy = (int)clampf(floorf((y - gg.oy) * inv_s), 0.f, gmax);
        const int cx0 = cx > 0 ? cx - 1 : 0, cx1 = cx < G - 1 ? cx + 1 : G - 1;
        const int cy0 = cy > 0 ? cy - 1 : 0, cy1 = cy < G - 1 ? cy + 1 : G - 1;
        const int csh = level_shift((uint32_t)(G * G));
        // the (up to) three rows' record ranges first -- six independent loads, one round trip -- then the records
        uint32_t j0[3], j1[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int yy = cy0 + r;
            const uint32_t row = (uint32_t)((yy <= cy1 ? yy : cy1) * G);
            j0[r] = pv.starts[pv.level_off[l] + ((row + (uint32_t)cx0) << csh)];
            j1[r] = yy <= cy1 ? pv.starts[pv.level_off[l] + ((row + (uint32_t)cx1 + 1u) << csh)] : j0[r];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
            for (uint32_t j = j0[r] + (uint32_t)i; j < j1[r]; j += STRIDE) body(j, pv.rec[2 * (size_t)j], pv.rec[2 * (size_t)j + 1]);
    }
}
// The same walk with the whole wave in step (four points per wave, 16 lanes per point, STRIDE = 16): `body(have, j, A,
// B)` is called by all 64 lanes together -- `have` says whether this lane holds a candidate (lanes without one get the
// all-zero record N) -- as many times per cell row as the longest of the four points' ranges needs, so that the body may
// exchange data between lanes.  Called with the same (wave-uniform) set of levels by every lane.
template <typename Body>
__device__ __forceinline__ void walk_point_instep(const PlanView& pv, float x, float y, int i, Body&& body) {
    const GaussGrid gg = pv.params->gg;
    const uint32_t level_mask = pv.params->level_mask;
    for (int l = 0; l < pv.L; ++l) {
        if (!(level_mask >> l & 1u)) continue;
        const int G = pv.G0 >> l;
        const float inv_s = gg.inv_s0 * __builtin_amdgcn_ldexpf(1.f, -l);
        const float gmax = (float)(G - 1);
        const int cx = (int)clampf(floorf((x - gg.ox) * inv_s), 0.f, gmax);
        const int cy = (int)clampf(floorf((y - gg.oy) * inv_s), 0.f, gmax);
        const int cx0 = cx > 0 ? cx - 1 : 0, cx1 = cx < G - 1 ? cx + 1 : G - 1;
        const int cy0 = cy > 0 ? cy - 1 : 0, cy1 = cy < G - 1 ? cy + 1 : G - 1;
        const int csh = level_shift((uint32_t)(G * G));
        uint32_t j0[3], j1[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int yy = cy0 + r;
            const uint32_t row = (uint32_t)((yy <= cy1 ? yy : cy1) * G);
            j0[r] = pv.starts[pv.level_off[l] + ((row + (uint32_t)cx0) << csh)];
            j1[r] = yy <= cy1 ? pv.starts[pv.level_off[l] + ((row + (uint32_t)cx1 + 1u) << csh)] : j0[r];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            uint32_t len = j1[r] - j0[r];                  // the same in the 16 lanes of a point
#pragma unroll
            for (int o = 16; o < 64; o <<= 1) len = max(len, (uint32_t)__shfl_xor((int)len, o));
            len = (uint32_t)__builtin_amdgcn_readfirstlane((int)len);
            for (uint32_t o = 0; o < len; o += 16u) {
                const uint32_t j = j0[r] + o + (uint32_t)i;
                const bool have = j < j1[r];
                const size_t jj = have ? j : pv.N;
                body(have, (uint32_t)jj, pv.rec[2 * jj], pv.rec[2 * jj + 1]);
            }
        }
    }
}
__device__ __forceinline__ float pair_q(const float4 A, const float4 B, float x, float y) {
    const float dx = x - A.x, dy = y - A.y;
    return A.z * dx * dx + (2.f * A.w * dx + B.x * dy) * dy;
}
__device__ __forceinline__ Rec make_rec(const float4 A, const float4 B) {
    Rec r;
    r.mu[0] = A.x; r.mu[1] = A.y; r.con[0] = A.z; r.con[1] = A.w; r.con[2] = B.x;
    r.v[0] = B.y; r.v[1] = B.z;
    return r;
}

// Walks a tile's list (or its ranges): `step(idx, gm, have)` for every STEP entries (lane = entry; the
// lanes from STEP on hold none).  A tile in ranges mode has no masks: `ranges_mask()` is called once and
// returns the functor `mask(idx, have)` that finds an entry's (the caller's kernel keeps its `step` free
// of that rare case).
template <int STEP, bool WIDE, typename Step, typename RangesMask>
__device__ __forceinline__ void for_each_step(const PlanView& pv, uint32_t tile, int lane, Step&& step,
                                              RangesMask&& ranges_mask) {
    const uint32_t hdr = pv.hdr[(size_t)tile * TILE_HDR_WORDS];
    const uint32_t count = hdr & TILE_COUNT_MASK;
    const uint32_t* slab = pv.tlist + (size_t)tile * pv.list_cap;
    if ((hdr >> TILE_MODE_SHIFT) == TILE_MODE_LIST) {
        for (uint32_t e0 = 0; e0 < count; e0 += STEP) {
            const bool have = lane < STEP && e0 + (uint32_t)lane < count;
            const uint32_t e = have ? slab[e0 + lane] : 0u;
            step(e & LIST_IDX_MASK, WIDE ? (e >> LIST_WIDE_SHIFT) & 15u : e >> LIST_NARROW_SHIFT, have);
        }
    } else if ((hdr >> TILE_MODE_SHIFT) == TILE_MODE_GROUPS) {
        // the four group lists, one after the other, as lists of single-group entries (a Gaussian that
        // reaches two groups comes twice, each time for one of them)
        for (uint32_t g = 0; g < 4; ++g) {
            const uint32_t ng = pv.hdr[(size_t)tile * TILE_HDR_WORDS + 1 + g];
            const uint32_t* gl = pv.glist + ((size_t)tile * 4 + g) * pv.list_cap;
            for (uint32_t e0 = 0; e0 < ng; e0 += STEP) {
                const bool have = lane < STEP && e0 + (uint32_t)lane < ng;
                step(have ? gl[e0 + lane] : 0u, have ? 1u << g : 0u, have);
            }
        }
    } else {
        auto mask = ranges_mask();
        for (uint32_t r = 0; r < count; ++r) {
            const uint32_t j0 = slab[2 * r], len = slab[2 * r + 1];
            for (uint32_t o = 0; o < len; o += STEP) {
                const bool have = lane < STEP && o + (uint32_t)lane < len;
                const uint32_t idx = have ? j0 + o + (uint32_t)lane : j0;
                step(idx, mask(idx, have), have);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// Forward.  Every group (DPP row) of the wave keeps its own queue of RECORDS in LDS and fills it from
// ITS OWN list (the group lists of the plan; 32 positions per chunk, two rounds of 16 gathers in
// flight), the all-zero record behind the list's end (v = 0: contributes nothing); then the queues
// are evaluated row-wise up to the longest list: in one instruction every row works on its OWN
// Gaussian, read from LDS at an address that is affine in the loop counter (no index indirection:
// the reads of the next rows are in flight while the current ones are evaluated).  A tile in
// record-range mode fills the queues by testing the ranges' records against the group boxes.
// A record in LDS is {mux, muy, a, b}, {c, v0, v1, -}: one ds_read_b128 + one ds_read_b64 (c = 1).
// The reads are inline asm: hipcc fuses 8-byte LDS reads of neighbouring rows into ds_read2_b64,
// which moves 16 bytes in 8 LDS cycles where ds_read_b128 takes 4 (MI355X_MICROARCH.md, LDS
// table), and collapses a source-level prefetch into load-then-wait.
// ------------------------------------------------------------------------------------------
#ifndef PIGS_GROUP_CAP
#define PIGS_GROUP_CAP 32        // records per group queue
#endif
constexpr int GROUP_CAP = PIGS_GROUP_CAP;
static_assert(GROUP_CAP >= 8 && GROUP_CAP % PIGS_FWD_UNROLL == 0, "queue capacity");

struct FwdLds {
    static constexpr int GSTRIDE = GROUP_CAP * 32 + 32;            // bytes; + 32: the four queues start on different banks
    float4 rec[(4 * GSTRIDE + PIGS_FWD_UNROLL * 32) / 16];        // tail: the prefetch behind the last row
};

typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));

// LDS byte address of a __shared__ object (for ds_* inline asm)
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}
template <int C> struct LdsRec;
template <> struct LdsRec<1> { f4v a; f2v b; };
template <> struct LdsRec<2> { f4v a; f4v b; };
// issue the reads of the record at addr + OFF (no wait: lds_rec_wait before the first use)
template <int OFF>
__device__ __forceinline__ void lds_rec_issue(LdsRec<1>& r, uint32_t addr) {
    asm volatile("ds_read_b128 %0, %2 offset:%3\n\tds_read_b64 %1, %2 offset:%4"
                 : "=v"(r.a), "=v"(r.b) : "v"(addr), "i"(OFF), "i"(OFF + 16));
}
template <int OFF>
__device__ __forceinline__ void lds_rec_issue(LdsRec<2>& r, uint32_t addr) {
    asm volatile("ds_read_b128 %0, %2 offset:%3\n\tds_read_b128 %1, %2 offset:%4"
                 : "=v"(r.a), "=v"(r.b) : "v"(addr), "i"(OFF), "i"(OFF + 16));
}
template <int C>
__device__ __forceinline__ void lds_rec_wait(LdsRec<C>* r) {      // r[0], r[1]: every pending destination
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(r[0].a), "+v"(r[0].b), "+v"(r[1].a), "+v"(r[1].b));
}
template <int C>
__device__ __forceinline__ Rec rec_of(const LdsRec<C>& x) {
    Rec r;
    r.mu[0] = x.a.x; r.mu[1] = x.a.y; r.con[0] = x.a.z; r.con[1] = x.a.w; r.con[2] = x.b.x; r.v[0] = x.b.y;
    if constexpr (C == 2) r.v[1] = x.b.z;
    else r.v[1] = 0.f;
    return r;
}

// rows: a multiple of 2.  Two register sets take turns: while one pair of rows is evaluated the
// reads of the next pair are in flight (the last issue reads the two rows behind the queue: inside
// the LDS block, never used).
template <int C, int MASK>
__device__ __forceinline__ void evaluate_rows(float* acc, const float* s, const FwdLds& lds, int rows, int lane,
                                              const RzOf<float, MASK>& rz) {
    static_assert(PIGS_FWD_UNROLL == 2, "two rows per register set");
    uint32_t q = lds_addr(lds.rec) + (uint32_t)(lane >> 4) * FwdLds::GSTRIDE;
    LdsRec<C> ra[2], rb[2];
    auto eval2 = [&](const LdsRec<C>* r) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const Rec x = rec_of<C>(r[u]);
            fwd_accumulate<float, 2, C, MASK>(acc, s, x.mu, x.con, x.v, &rz);
        }
    };
    lds_rec_issue<0>(ra[0], q);
    lds_rec_issue<32>(ra[1], q);
    int k = 0;
    for (; k + 4 <= rows; k += 4) {
        lds_rec_wait<C>(ra);
        lds_rec_issue<64>(rb[0], q);
        lds_rec_issue<96>(rb[1], q);
        eval2(ra);
        lds_rec_wait<C>(rb);
        lds_rec_issue<128>(ra[0], q);
        lds_rec_issue<160>(ra[1], q);
        q += 128;
        eval2(rb);
    }
    lds_rec_wait<C>(ra);
    if (k < rows) eval2(ra);
}

// register budget: 8 waves/SIMD (64 VGPRs) for the narrow variants, fewer waves for the wide ones
// (c = 2 with orders up to 3: 12-20 accumulators) so that they do not spill
template <int C, int MASK>
constexpr int fwd_waves() {
    constexpr int n = FwdLayout<2, C, MASK>::N;
    // the coupled residual (c = 2, 4 accumulators): 65 VGPRs -- 7 waves; held to 8 waves' 64 it puts two registers in scratch
    if (MASK == ORDC) return 7;
    return n > 12 ? 4 : n > 10 ? 5 : (C == 1 && (MASK == 7 || MASK == 19 || MASK == 1 || MASK == ORDR || MASK == ORDG)) ? PIGS_FWD_WAVES : 6;
}
constexpr bool fwd_can_stage(int C, int MASK) { return C == 1 && (MASK == 7 || MASK == 19); }
// staged outputs (PlanView::stage): one record per point at its original index instead of the three stores
template <int C, int MASK>
__device__ __forceinline__ void stage_store(const PlanView& pv, const float* acc, uint32_t m) {
    using L = FwdLayout<2, C, MASK>;
    if constexpr (C == 1 && MASK == 7) {
        pv.stage[2 * (size_t)m] = make_float4(acc[L::O0], -acc[L::O1], -acc[L::O1 + 1], acc[L::O2]);
        pv.stage[2 * (size_t)m + 1] = make_float4(acc[L::O2 + 1], acc[L::O2 + 1], acc[L::O2 + 2], 0.f);
    } else if constexpr (C == 1 && MASK == 19) {
        pv.stage[2 * (size_t)m] = make_float4(acc[L::O0], -acc[L::O1], -acc[L::O1 + 1], acc[L::O2]);
    }
}

// TILE_MODE_POINTS (plan.h): four points of tile `tile` at a time (quad = 0 .. 15), 16 lanes per point, lane = candidate
template <int C, int MASK>
__device__ __forceinline__ void forward_points_quad(const PlanView& pv, const SamplesView& sv, uint32_t tile, uint32_t quad, int lane,
                                                    float q_f, float* __restrict__ o0, float* __restrict__ o1,
                                                    float* __restrict__ o2, float* __restrict__ o3, const RzOf<float, MASK>& rz) {
    using L = FwdLayout<2, C, MASK>;
    const int row = lane >> 4, i = lane & 15;
    const uint32_t m = tile * TILE_POINTS + quad * 4u + (uint32_t)row;
    const bool valid = m < sv.M;
    const SPoint sp = tile_point(sv, point_order(sv), tile, quad * 4u + (uint32_t)row);
    const float s[2] = {sp.x, sp.y};
    float acc[L::N];
#pragma unroll
    for (int k = 0; k < L::N; ++k) acc[k] = 0.f;
    // !(q > cut): a degenerate conic (NaN) is evaluated, as the list build's tests would have kept it
    walk_point<16>(pv, sp.x, sp.y, i, [&](uint32_t, const float4 A, const float4 B) {
        if (!(pair_q(A, B, sp.x, sp.y) > q_f)) {
            const Rec r = make_rec(A, B);
            fwd_accumulate<float, 2, C, MASK>(acc, s, r.mu, r.con, r.v, &rz);
        }
    });
#pragma unroll
    for (int k = 0; k < L::N; ++k) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) acc[k] += __shfl_xor(acc[k], o);
    }
    if (i == 0 && valid) {
        if (fwd_can_stage(C, MASK) && pv.stage) stage_store<C, MASK>(pv, acc, sp.m);
        else fwd_store<float, 2, C, MASK, false>(acc, (int64_t)sp.m, o0, o1, o2, o3, &rz);
    }
}

// one tile (one wave) through its group lists / record ranges; a tile in TILE_MODE_POINTS is left to the caller
template <int C, int MASK>
__device__ __forceinline__ void forward_tile(const PlanView& pv, const SamplesView& sv, uint32_t tile, int lane, FwdLds& lds,
                                             float* __restrict__ o0, float* __restrict__ o1, float* __restrict__ o2,
                                             float* __restrict__ o3, const RzOf<float, MASK>& rz) {
    using L = FwdLayout<2, C, MASK>;
    constexpr int U = PIGS_FWD_UNROLL;
    constexpr bool CAN_STAGE = fwd_can_stage(C, MASK);
    __builtin_amdgcn_s_setprio(3);
    char* const qbase = (char*)lds.rec;
    const uint32_t m = tile * TILE_POINTS + (uint32_t)lane;
    const bool valid = m < sv.M;
    // The head of a wave: the point's address waits for the order of the points, which is in memory; the
    // tile header and the first chunk's list entries wait for nothing but kernel arguments.  So the question for the
    // order leaves first (one scalar load), header and entries leave behind it, and only then is the order used: the
    // wave's first wait covers all three, and the records are its second round trip.  (Scalar loads return in no
    // order -- a wait for one is a wait for all -- so the arguments that header and entries are addressed by are in
    // registers before the question leaves: the empty asm.  Checked in the ISA of hipcc 7.2.26015, clang 22.0.0git
    // roc-7.2.0: the four global loads and the s_load_dwordx4 of lat / src, then s_waitcnt lgkmcnt(0).)
    const int g = lane >> 4, i = lane & 15;
    asm volatile("" ::"s"(sv.params), "s"(sv.M), "s"(pv.hdr), "s"(pv.glist), "s"(pv.list_cap));
    const PointOrderWords pw = point_order_words(sv);
    // (word 0 through a lane index the compiler cannot see through: a load it knows to be uniform is followed by its
    // v_readfirstlane, and the wait for the header would stand in front of the point's load)
    const uint32_t* hd = pv.hdr + (size_t)tile * TILE_HDR_WORDS;
    uint32_t zero = 0u;
    asm("" : "+v"(zero));
    const uint32_t h0v = hd[zero];
    const uint32_t ngv = hd[1 + g];           // this row's list length (a tile without group lists: not used)
    // the first chunk's entries are loaded whether or not they lie inside the list -- or the tile has group lists at all
    // (every tile has the slab, and list_cap is a multiple of 16: in bounds)
    const uint32_t* gl = pv.glist + ((size_t)tile * 4 + g) * pv.list_cap;
    uint32_t e0 = gl[(uint32_t)i < pv.list_cap ? i : 0], e1 = gl[16u + (uint32_t)i < pv.list_cap ? 16 + i : 0];
    const SPoint sp = tile_point(sv, point_order(pw), tile, (uint32_t)lane);      // lanes behind the last point repeat it (never stored)
    const uint32_t h0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)h0v);
    const float s[2] = {sp.x, sp.y};
    float acc[L::N];
#pragma unroll
    for (int k = 0; k < L::N; ++k) acc[k] = 0.f;
    // one chunk: every row fills its queue with `rows` records (its own list's, or the all-zero record
    // behind the list's end), two rounds of 16 in flight together, and the rows are evaluated
    auto chunk = [&](int rows, auto&& index_of) {
        static_assert(GROUP_CAP == 32, "two rounds of 16 records per chunk");
        rows = __builtin_amdgcn_readfirstlane((rows + U - 1) / U * U);
        const uint32_t j0 = index_of(0, i), j1 = index_of(1, 16 + i);      // (round of the chunk, position in it)
        const float4 A0 = pv.rec[2 * (size_t)j0], B0 = pv.rec[2 * (size_t)j0 + 1];
        float4 A1 = A0, B1 = B0;
        if (rows > 16) { A1 = pv.rec[2 * (size_t)j1]; B1 = pv.rec[2 * (size_t)j1 + 1]; }
        float4* dst = (float4*)(qbase + g * FwdLds::GSTRIDE + i * 32);
        wave_lds_fence();
        dst[0] = A0;
        *(float2*)(dst + 1) = make_float2(B0.x, B0.y);
        if constexpr (C == 2) *(float2*)((char*)(dst + 1) + 8) = make_float2(B0.z, 0.f);
        if (rows > 16) {
            dst[32] = A1;
            *(float2*)(dst + 33) = make_float2(B1.x, B1.y);
            if constexpr (C == 2) *(float2*)((char*)(dst + 33) + 8) = make_float2(B1.z, 0.f);
        }
        wave_lds_fence();
        // waves outside the row loop (issuing loads, filling queues, storing) go first: their memory
        // requests are what the others' arithmetic hides (27.5 -> 27.3 us; the other way round 28.1)
        __builtin_amdgcn_s_setprio(0);
        evaluate_rows<C, MASK>(acc, s, lds, rows, lane, rz);
        __builtin_amdgcn_s_setprio(3);
    };
    if ((h0 >> TILE_MODE_SHIFT) == TILE_MODE_POINTS) {
        return;                                   // scattered points: the caller's (helper workgroups / the fused launch's own walk)
    } else if ((h0 >> TILE_MODE_SHIFT) != TILE_MODE_RANGES) {            // LIST or GROUPS: the group lists are there
        const uint32_t ng = ngv;
        const uint32_t n0 = (uint32_t)__builtin_amdgcn_readlane((int)ngv, 0), n1 = (uint32_t)__builtin_amdgcn_readlane((int)ngv, 16);
        const uint32_t n2 = (uint32_t)__builtin_amdgcn_readlane((int)ngv, 32), n3 = (uint32_t)__builtin_amdgcn_readlane((int)ngv, 48);
        uint32_t nmax = n0 > n1 ? n0 : n1;
        nmax = n2 > nmax ? n2 : nmax;
        nmax = n3 > nmax ? n3 : nmax;
        for (uint32_t base = 0; base < nmax; base += GROUP_CAP) {
            const int rows = (int)(nmax - base < GROUP_CAP ? nmax - base : GROUP_CAP);
            // the entry is loaded whether or not it lies inside the list (the slab has the room, and
            // the load then does not wait for the header): one dependent round trip less per tile
            chunk(rows, [&](int round, int p) { return base + p < ng ? (round == 0 ? e0 : e1) : pv.N; });
            if (base + GROUP_CAP < nmax) {                  // the next chunk's (where the parent's loop loaded them: behind this chunk's rows)
                const uint32_t p0 = base + GROUP_CAP + (uint32_t)i, p1 = p0 + 16u;
                e0 = gl[p0 < pv.list_cap ? p0 : 0u];
                e1 = gl[p1 < pv.list_cap ? p1 : 0u];
            }
        }
    } else {
        // Record ranges (a group list did not fit): the ranges hold every Gaussian near the tile.  Every
        // row tests them, 16 at a time, against the box of ITS group and packs the hits into its queue;
        // the queues are evaluated when one could overflow, and at the end.  With scattered points
        // (which is when lists overflow) a row keeps a small part of what the ranges hold.
        const uint32_t* slab = pv.tlist + (size_t)tile * pv.list_cap;
        const uint32_t count = h0 & TILE_COUNT_MASK;
        const float INF = __builtin_huge_valf();
        const float q_f = pv.params->q_f;
        float x0 = valid ? sp.x : INF, x1 = valid ? sp.x : -INF, y0 = valid ? sp.y : INF, y1 = valid ? sp.y : -INF;
        row_box_dpp(x0, x1, y0, y1);                  // every lane: the box of its own row's group
        const bool row_has_points = x0 <= x1;
        float4* const q = (float4*)(qbase + g * FwdLds::GSTRIDE);
        int qn = 0;                                    // records in this row's queue (the same in its 16 lanes)
        auto drain = [&]() {
            // rows = the longest queue, the others padded with all-zero records
            int rows = qn;
#pragma unroll
            for (int o = 16; o < 64; o <<= 1) rows = max(rows, __shfl_xor(rows, o));
            rows = __builtin_amdgcn_readfirstlane((rows + U - 1) / U * U);
            wave_lds_fence();
            for (int k = qn + i; k < rows; k += 16) {
                q[2 * k] = make_float4(0.f, 0.f, 0.f, 0.f);
                q[2 * k + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            wave_lds_fence();
            if (rows > 0) {
                __builtin_amdgcn_s_setprio(0);
                evaluate_rows<C, MASK>(acc, s, lds, rows, lane, rz);
                __builtin_amdgcn_s_setprio(3);
            }
            qn = 0;
        };
        for (uint32_t r = 0; r < count; ++r) {
            const uint32_t j0 = slab[2 * r], len = slab[2 * r + 1];
            for (uint32_t base = 0; base < len; base += 16) {
                const bool in = base + (uint32_t)i < len;
                const size_t j = in ? j0 + base + (uint32_t)i : pv.N;
                const float4 A = pv.rec[2 * j], B = pv.rec[2 * j + 1];
                const bool hit = in && row_has_points && ellipse_reaches_rect(ellipse_of(A, B.x), x0, y0, x1, y1, q_f);
                const uint32_t rm = (uint32_t)(__ballot(hit) >> (16 * g)) & 0xffffu;      // this row's hits
                if (hit) {
                    const int k = qn + __builtin_popcount(rm & ((1u << i) - 1u));
                    q[2 * k] = A;
                    *(float2*)(q + 2 * k + 1) = make_float2(B.x, B.y);
                    if constexpr (C == 2) *(float2*)((char*)(q + 2 * k + 1) + 8) = make_float2(B.z, 0.f);
                }
                qn += __builtin_popcount(rm);
                if (__any(qn > GROUP_CAP - 16)) drain();
            }
        }
        drain();
    }
    // The outputs go back through the points' original indices.  Where those run in the caller's order
    // (a grid: runs of 4 or more consecutive points per cell row) a tile's stores fill whole 32..128-byte
    // segments and leave through non-temporal stores: nothing in the launch reads them again, and
    // streamed they do not wait in the L2 for the end-of-kernel write-back (28.0 -> 26.6 us).  Where
    // the points came in no order (shuffled grids, random points) every store is a lone 4..16 bytes and
    // needs the L2's write combining: streamed, the same launch takes 115 us instead of 54.
    const uint32_t m_other = (uint32_t)__shfl_xor((int)sp.m, 1);
    const uint32_t dist = sp.m > m_other ? sp.m - m_other : m_other - sp.m;
    const bool stream = __builtin_popcountll(__ballot(valid && dist == 1u)) >= 48;
    if (CAN_STAGE && pv.stage) {
        if (valid) stage_store<C, MASK>(pv, acc, sp.m);
    } else if (valid) {
        if (stream) {
            fwd_store<float, 2, C, MASK, true>(acc, (int64_t)sp.m, o0, o1, o2, o3, &rz);
            asm volatile("" ::: "memory");       // keeps the two branches' stores apart: merged into a common tail they lose the hint
        } else {
            fwd_store<float, 2, C, MASK, false>(acc, (int64_t)sp.m, o0, o1, o2, o3, &rz);
        }
    }
}

template <int C, int MASK>
__global__ __launch_bounds__(64 * PIGS_FWD_WG_WAVES, (fwd_waves<C, MASK>())) void tile_forward_kernel(
    PlanView pv, SamplesView sv, float* __restrict__ o0, float* __restrict__ o1, float* __restrict__ o2,
    float* __restrict__ o3, RzOf<float, MASK> rz) {
    constexpr uint32_t FW = PIGS_FWD_WG_WAVES;
    __shared__ FwdLds lds_all[FW];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nmain = (sv.ntiles + FW - 1u) / FW;
    // The helper workgroups come FIRST in the launch (round 4): their walks are chains of dependent loads that take
    // many times a tile's life, and dispatched behind the main ones (round 3) they were the launch's tail -- a
    // clamped-normal cloud's forward took 56 us for 30 us of tile work.  They leave at once when the plan queued no
    // TILE_MODE_POINTS tile.  Their number is a multiple of 8: workgroup i of the main ones still runs on XCD i % 8.
    constexpr uint32_t NHELP = POINT_HELPER_BLOCKS * 4u / FW;
    static_assert(NHELP % 8u == 0u, "the main workgroups keep their XCD");
    if (blockIdx.x < NHELP) {
        // helper workgroups (plan.h, TILE_MODE_POINTS): four points at a time, 16 lanes per point, lane = candidate
        const uint32_t n = pv.params->n_points;
        if (n == 0u) return;
        const float q_f = pv.params->q_f;
        const uint32_t hw = blockIdx.x * FW + (uint32_t)wave, nhw = NHELP * FW;
        for (uint32_t qd = hw; qd < n * 16u; qd += nhw)
            forward_points_quad<C, MASK>(pv, sv, pv.ptiles[qd >> 4], qd & 15u, lane, q_f, o0, o1, o2, o3, rz);
        return;
    }
    const uint32_t tile = xcd_block_chunk<PIGS_XCD_CHUNK * 4 / FW>(nmain, blockIdx.x - NHELP) * FW + (uint32_t)wave;
    if (tile >= sv.ntiles) return;
    forward_tile<C, MASK>(pv, sv, tile, lane, lds_all[wave], o0, o1, o2, o3, rz);
}

// ------------------------------------------------------------------------------------------
// The FIRST forward of a plan in the launch that builds its tile lists (PIGS_BUILD_DEFER_LISTS; round 4).  The
// list build is a chain of dependent loads (a wave issues in 38 % of its cycles), the forward is float32
// arithmetic: in two launches neither hides the other, and the forward's own first loads have nothing to hide
// behind.  Here a wave builds the lists of its four tiles (written out as ever: the backward and every further
// sample_*() of the same preprocess read them) and evaluates those tiles at once -- while it computes, the other
// waves of its SIMD are still walking the grid.  One kernel boundary and the forward's cold start go away.
// A tile in TILE_MODE_POINTS is walked by its own wave here (the helper workgroups of the two-launch path read a
// queue that is complete only when this launch ends): right, and slower for clouds with thin outskirts -- the
// hosts defer the lists for every plan all the same, because a cloud's first step is one of thousands.
// ------------------------------------------------------------------------------------------
template <int C, int MASK>
__global__ __launch_bounds__(256, 5) void plan_lists_forward_kernel(ListArgs a, float* __restrict__ o0, float* __restrict__ o1,
                                                                 float* __restrict__ o2, float* __restrict__ o3, RzOf<float, MASK> rz) {
    __shared__ ListsLds<LISTS_TPW> lds_all[4];
    static_assert(sizeof(FwdLds) <= sizeof(ListsLds<LISTS_TPW>), "the forward's queues live in the list build's LDS");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    lists_strip_cover(a);
    const uint32_t tile0 = lists_tile0<LISTS_TPW>(wave);
    const uint32_t ntiles = a.sv.ntiles;
    if (tile0 >= ntiles) return;
    build_block_lists<LISTS_TPW, false, false, false>(a, lds_all[wave], tile0, lane);      // (general path, plain stores: plan_lists.h)
    // what this wave's lanes stored (headers, group lists) is read back by other lanes of it: the stores have
    // reached the L2 before the first load is issued
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    FwdLds& flds = *reinterpret_cast<FwdLds*>(&lds_all[wave]);
    for (int t = 0; t < LISTS_TPW; ++t) {
        const uint32_t tile = tile0 + (uint32_t)t;
        if (tile >= ntiles) break;
        const uint32_t h0 = __hip_atomic_load(a.pv.hdr + (size_t)tile * TILE_HDR_WORDS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if ((h0 >> TILE_MODE_SHIFT) == TILE_MODE_POINTS) {
            for (uint32_t quad = 0; quad < 16u; ++quad) forward_points_quad<C, MASK>(a.pv, a.sv, tile, quad, lane, a.q_f, o0, o1, o2, o3, rz);
        } else {
            forward_tile<C, MASK>(a.pv, a.sv, tile, lane, flds, o0, o1, o2, o3, rz);
        }
    }
}

// ------------------------------------------------------------------------------------------
// staging launches (PlanView::stage): thread = point in the CALLER's order, everything coalesced
// ------------------------------------------------------------------------------------------
template <int MASK>
__global__ __launch_bounds__(256) void stage_to_outputs_kernel(const float4* __restrict__ stage, uint32_t M, float* __restrict__ o0,
                                                               float* __restrict__ o1, float* __restrict__ o2) {
    const uint32_t m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const float4 a = stage[2 * (size_t)m];
    if (o0) __builtin_nontemporal_store(a.x, &o0[m]);
    if (o1) { __builtin_nontemporal_store(a.y, &o1[2 * (size_t)m]); __builtin_nontemporal_store(a.z, &o1[2 * (size_t)m + 1]); }
    if constexpr (MASK == 7) {
        const float4 b = stage[2 * (size_t)m + 1];
        if (o2) {
            float* h = o2 + 4 * (size_t)m;
            __builtin_nontemporal_store(a.w, h); __builtin_nontemporal_store(b.x, h + 1);
            __builtin_nontemporal_store(b.y, h + 2); __builtin_nontemporal_store(b.z, h + 3);
        }
    } else {
        if (o2) __builtin_nontemporal_store(a.w, &o2[m]);
    }
}

}  // namespace pigs
