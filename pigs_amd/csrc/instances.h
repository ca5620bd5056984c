// The order masks of the sampling kernels and THE lists of their compiled instantiations, once: dense.hip's and
// plan.hip's switches are generated from the lists below, and tests/launch_choice_main.cpp prints them for the tests'
// coverage tables.  No device code, no HIP call.
#pragma once

namespace pigs {

// Order masks: bit k < 4 = derivative order k (pointer slot k); bit 4 (16) = the TRACE of the order-2
// output (the Laplacian), which takes pointer slot 2 in place of the full Hessian, [M][c].
// The fused outputs: one mask each, alone, the output in slot 0, reachable through their own entry points only.  The
// kernels know them as ORDR, ORDG, ORDV, ORDC, ORDN (pair_math.h; dense.hip asserts that the two sets agree).  The network
// inputs (ORDI, ORDJ) are fused outputs too, but forward only and through all four slots.
constexpr int MASK_RESIDUAL = 32;             // the linear residual, [M][c] -- pigs_residual_*
constexpr int MASK_TERMS = 64;                // the general residual, [M][c] -- pigs_residual_terms_*
constexpr int MASK_VORTICITY = 128;           // the vorticity terms (d = 2, c = 2), [M][7] -- pigs_vorticity_*
constexpr int MASK_COUPLED = 256;             // the coupled residual (c >= 2), [M][c] -- pigs_residual_coupled_*
constexpr int MASK_VORT_RESIDUAL = 512;       // the vorticity residual (d = 2, c = 2), [M][2] -- pigs_vorticity_residual_*
constexpr int MASK_VORT_FIT = 4096;           // the vorticity residual + its data term, [M][3] -- pigs_vorticity_fit_*
// the model's sample features (d = 2), [M][c], [M][2c], [M][2c], [M][p] in slots 0..3 -- pigs_network_inputs_forward
constexpr int MASK_NET_INPUTS = 1024;         // the right-hand sides zero, diffusion, burgers, wave
constexpr int MASK_NET_INPUTS_NS = 2048;      // Navier-Stokes (c = 2)
inline bool is_network_inputs(int m) { return m == MASK_NET_INPUTS || m == MASK_NET_INPUTS_NS; }
inline bool is_fused_output(int m) {
    return m == MASK_RESIDUAL || m == MASK_TERMS || m == MASK_VORTICITY || m == MASK_COUPLED || m == MASK_VORT_RESIDUAL ||
           m == MASK_VORT_FIT || is_network_inputs(m);
}
inline bool mask_valid(int m) { return m > 0 && m < 32 && !((m & 4) && (m & 16)); }
inline bool mask_uses_slot(int m, int k) {
    return is_network_inputs(m) ? true : is_fused_output(m) ? k == 0 : (m >> k & 1) || (k == 2 && (m & 16));
}
// Smallest compiled mask covering the request (compiled: single orders, 0..2, 0..3, the trace alone
// and orders 0, 1 + trace); 0 = no compiled kernel (trace together with order 3).
inline int covering_mask_of(int mask) {
    if (is_fused_output(mask)) return mask;
    if (mask & 16) return mask == 16 ? 16 : (mask & ~19) == 0 ? 19 : 0;
    if (mask == 1 || mask == 2 || mask == 4 || mask == 8) return mask;
    if ((mask & ~7) == 0) return 7;
    return 15;
}

// ---- the compiled covering masks, as X-macro lists: LIST(X) expands to X(mask) for every member
// every (d, c) of the dense path, c = 1 and 2 of the binned one
#define PIGS_PLAIN_MASKS(X) X(1) X(2) X(4) X(8) X(7) X(15) X(16) X(19) X(32) X(64)
// the binned path: the vorticity terms, the coupled residual and the vorticity residual, two channels only
#define PIGS_BINNED_C2_MASKS(X) X(128) X(256) X(512)
// the dense path: the vorticity terms and residual are a two-channel field in two dimensions; the coupled residual
// mixes channels, two and more
#define PIGS_DENSE_VORT_MASKS(X) X(128) X(512)
#define PIGS_DENSE_COUPLED_MASKS(X) X(256)
constexpr bool dense_vort_instance(int d, int c) { return d == 2 && c == 2; }
constexpr bool dense_coupled_instance(int c) { return c >= 2; }
// the binned path's fused first launch (plan_lists_forward_kernel: the list build and the forward in one), per
// channel count; the rest: the list launch, then the forward launch
#define PIGS_FUSED_FIRST_C1_MASKS(X) X(1) X(7) X(19) X(32)
#define PIGS_FUSED_FIRST_C2_MASKS(X) X(7)

// the network inputs: FORWARD ONLY -- the forward switches of dense.hip and plan.hip expand these two lists in addition to
// the ones above, the backward switches expand neither; which (d, c) a member is compiled for: network_instance
#define PIGS_DENSE_NETWORK_MASKS(X) X(1024) X(2048)
#define PIGS_BINNED_NETWORK_MASKS(X) X(1024) X(2048)
constexpr bool network_instance(int d, int c, int mask) {
    return d == 2 && (mask == MASK_NET_INPUTS || (mask == MASK_NET_INPUTS_NS && c == 2));
}

// the vorticity fit (d = 2, c = 2: dense_vort_instance): lists of its own, which the forward and the backward switches of
// dense.hip and plan.hip expand beside PIGS_DENSE_VORT_MASKS / PIGS_BINNED_C2_MASKS
#define PIGS_DENSE_FIT_MASKS(X) X(4096)
#define PIGS_BINNED_FIT_MASKS(X) X(4096)

#define PIGS_OR_MASK_IS(MK) || mask == (MK)
constexpr bool dense_compiled(int d, int c, int mask) {
    return (false PIGS_PLAIN_MASKS(PIGS_OR_MASK_IS)) ||
           (dense_vort_instance(d, c) && (false PIGS_DENSE_VORT_MASKS(PIGS_OR_MASK_IS) PIGS_DENSE_FIT_MASKS(PIGS_OR_MASK_IS))) ||
           (dense_coupled_instance(c) && (false PIGS_DENSE_COUPLED_MASKS(PIGS_OR_MASK_IS)));
}
constexpr bool binned_compiled(int c, int mask) {
    return (c == 1 || c == 2) && ((false PIGS_PLAIN_MASKS(PIGS_OR_MASK_IS)) ||
                                  (c == 2 && (false PIGS_BINNED_C2_MASKS(PIGS_OR_MASK_IS) PIGS_BINNED_FIT_MASKS(PIGS_OR_MASK_IS))));
}
constexpr bool fused_first_compiled(int c, int mask) {
    return c == 1 ? (false PIGS_FUSED_FIRST_C1_MASKS(PIGS_OR_MASK_IS)) : c == 2 ? (false PIGS_FUSED_FIRST_C2_MASKS(PIGS_OR_MASK_IS)) : false;
}

}  // namespace pigs
