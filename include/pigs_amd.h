/*
 * pigs_amd -- C ABI of the MI355X-native differentiable Gaussian sampler.
 *
 * This is the drop-in boundary for the hot path of kr4b/pigs: the native half of
 * `diff_gaussian_sampling.GaussianSampler`.  The reference's own native extension is an
 * un-vendored submodule (/root/reference/.gitmodules:1-3), so its C++ interface cannot be
 * cited; each entry point below replaces the native work behind one Python-visible method of
 * that class, cited by its call sites:
 *
 *   pigs_sample_forward   GaussianSampler.sample_gaussians()                (model_pn.py:650,770; test_gaussian_sampling.py:57)
 *                         .sample_gaussians_derivative()                    (model_pn.py:651,771; test_derivatives.py:124)
 *                         .sample_gaussians_laplacian()  [full Hessian]     (model_pn.py:652,772; test_derivatives.py:220)
 *                         .sample_gaussians_third_derivative()              (model_pn.py:654,778; test_pde.py:53)
 *   pigs_sample_backward  autograd backward of those outputs wrt (means, values, conics)
 *                         (test_derivatives.py:123,214-215,349-352; main_pn.py:220; test_no_mlp.py:146)
 *   pigs_samples_build,
 *   pigs_plan_*           GaussianSampler.preprocess(means, values, covariances, conics, samples)
 *                         (model_pn.py:648,768,784; test_gaussian_sampling.py:56; test_1d.py:30)
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HIP), row-major contiguous; nothing here takes or
 *     returns a torch type.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - all calls are asynchronous on `stream`; none allocates, frees or synchronises, so they
 *     can be captured into a hipGraph.
 *   - layouts: means[N][d], conics[N][d(d+1)/2] (upper triangle row-major: d=2 -> xx,xy,yy,
 *     gaussians.py:186-189), values[N][c], samples[M][d];
 *     out0[M][c], out1[M][d][c], out2[M][d][d][c], out3[M][d][d][d][c]  (model_pn.py:650-654).
 *   - orders_mask: bit k (k = 0..3) set = derivative order k is requested (outputs) / has an incoming
 *     gradient (backward).  Pointers of orders outside the mask may be NULL.
 *     Bit 4 (value 16) = the TRACE of the order-2 output, u_xx + u_yy, as [M][c] -- the Laplacian
 *     the PDE residuals consume (model_pn.py:614-617) -- written to / read from the out2 / gout2
 *     slot in place of the full Hessian; bits 2 and 4 exclude each other (PIGS_ERR_INVALID), the
 *     trace together with order 3 has no fused kernel (PIGS_ERR_UNSUPPORTED: two calls).
 *     The composed outputs have entry points of their own and no mask bit a caller may pass (PIGS_ERR_INVALID):
 *     the library's masks 32, 64, 128, 256 and 512 stand for pigs_residual_*, pigs_residual_terms_*,
 *     pigs_vorticity_*, pigs_residual_coupled_*, pigs_vorticity_residual_* and pigs_vorticity_fit_*.
 *   - supported: d in {1,2}, c in {1..4}, dtype f32/f64 (binned plan: d=2, f32).
 *   - return value: PIGS_OK or an error code; pigs_status_string() names it.
 */
#ifndef PIGS_AMD_H
#define PIGS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PIGS_ABI_VERSION 10

enum pigs_status {
    PIGS_OK = 0,
    PIGS_ERR_INVALID = 1,      /* bad argument (negative size, null required pointer, ...) */
    PIGS_ERR_UNSUPPORTED = 2,  /* d / c / dtype / mask combination not compiled            */
    PIGS_ERR_LAUNCH = 3,       /* HIP reported a launch error                              */
    PIGS_ERR_WORKSPACE = 4     /* workspace too small for the plan                         */
};

enum pigs_dtype { PIGS_F32 = 0, PIGS_F64 = 1 };

int pigs_abi_version(void);
const char* pigs_status_string(int status);
/* text of the HIP error behind the calling thread's last PIGS_ERR_LAUNCH */
const char* pigs_last_hip_error(void);

/* Dense forward: out_k = sum over ALL N Gaussians (exact reference semantics, no culling). */
int pigs_sample_forward(int dtype, int d, int c, int orders_mask, int64_t N, int64_t M,
                        const void* means, const void* conics, const void* values, const void* samples,
                        void* out0, void* out1, void* out2, void* out3, void* stream);

/* Dense backward: gradients of sum_k <gout_k, out_k> wrt means [N][d], flat conics
 * [N][d(d+1)/2] and values [N][c].  The three gradient buffers are overwritten. */
int pigs_sample_backward(int dtype, int d, int c, int orders_mask, int64_t N, int64_t M,
                         const void* means, const void* conics, const void* values, const void* samples,
                         const void* gout0, const void* gout1, const void* gout2, const void* gout3,
                         void* g_means, void* g_conics, void* g_values, void* stream);

/*
 * Fused covariance builder -- the caller-side step in front of preprocess():
 * gaussians.build_covariances(scaling, transform) (gaussians.py:163-193; model_pn.py:499-502,
 * 538-541, 607-610, 695-698; test_gaussian_sampling.py:36; test_derivatives.py:55-58).  d = 2.
 *   scaling [N][2] (variances, > 0), transform [N] (raw correlation, squashed by tanh)
 *   -> covariances [N][3] and conics [N][3], flat (xx, xy, yy); either output may be NULL.
 * The backward returns the gradients of <g_covariances, cov> + <g_conics, conic> wrt scaling
 * [N][2] and transform [N]; a NULL incoming gradient reads as zero.
 */
int pigs_build_covariances(int dtype, int64_t N, const void* scaling, const void* transform,
                           void* covariances, void* conics, void* stream);
int pigs_build_covariances_backward(int dtype, int64_t N, const void* scaling, const void* transform,
                                    const void* g_covariances, const void* g_conics,
                                    void* g_scaling, void* g_transform, void* stream);

/*
 * Binned ("plan") path -- float32, d = 2, c <= 2.  preprocess() builds, in caller-owned device
 * memory, two position independent workspaces:
 *
 *   SAMPLES workspace (pigs_samples_workspace_bytes(M) bytes, 256-byte aligned): the sample points
 *     sorted into ~16-point cells; tiles of 64 / groups of 16 consecutive sorted points are the
 *     units of work.  Built from `samples` alone and immutable afterwards, so it may be shared by
 *     any number of plans: the reference re-binds new Gaussians to an unchanged sample set on every
 *     step of a roll-out (main_pn.py:317-324), and so does any fixed collocation grid.
 *   PLAN workspace (pigs_plan_workspace_bytes(N, M, c) bytes): the Gaussians binned by centre into a
 *     multi-level cell grid (packed, sorted 32-byte records) and, for every tile, the list of
 *     Gaussians whose q <= q_max ellipse reaches the tile (with the 16-point groups each one
 *     reaches).  Forward, backward and every further sample_*() of the same preprocess() read the
 *     lists; none walks the grid again.
 *
 * The sampling entry points evaluate, for every point, only the Gaussians whose q <= q_max ellipse
 * reaches the bounding box of the point's group (dropped terms are below exp(-q_max/2) of a term's
 * scale; q_max = 36 -> 1.5e-8).  A plan holds TWO cut-offs (ABI 6): `q_max` for the forward and for
 * the backward of gradients that arrive at orders 0 and 1, and `q_max_backward` >= q_max for the
 * backward of gradients that arrive at order 2, order 3 or the trace (a value <= q_max, 0 included,
 * means one cut-off).  Why: the conic gradient of a second-derivative term carries a q^2 prefactor and
 * its sum over the points nearly cancels, so with thousands of points per Gaussian and one-signed
 * incoming gradients the tail beyond q = 36 was 2.5e-5 of the largest entry; at 40 (the Python host's
 * default) it is 3.5e-6, the dense kernel's own float32 error level (DESIGN.md "Cut-off").  The same (N, M, c) and the same samples workspace must be passed to every
 * call on a plan workspace; the plan remembers its cut-offs (the q_max argument of pigs_plan_forward /
 * pigs_plan_backward is kept for ABI shape and ignored since ABI 6).  pigs_plan_backward uses scratch
 * inside the plan workspace: calls sharing one must be stream ordered.
 */
size_t pigs_samples_workspace_bytes(int64_t M);                  /* 0 = unsupported size */
size_t pigs_plan_workspace_bytes(int64_t N, int64_t M, int c);   /* 0 = unsupported sizes */

/* samples workspace alone (4 launches; 5 on the coarse-bin path).
 * Two ways to sort the points, same result (the order inside a 16-point cell aside): ONE PASS -- one returning
 * atomic per run of consecutive points that share a cell, right for lattices in row order -- and COARSE BINS --
 * per-workgroup LDS ranking inside 256 coarse bins, a scan of the (bin, workgroup) counts, a scatter into bin
 * segments and a per-bin LDS sort; right for points in no order (torch.rand collocation points, main_pn.py:103),
 * which otherwise pay one global atomic and one 12-byte scattered write each.  The host cannot see which it
 * has without a synchronisation, so the library remembers, per device and M: every build of M >= 131 072
 * points leaves {runs, points} of a sample of its waves in the workspace, copied to pinned memory on `stream`
 * behind the build (nobody waits); the next build of the same M takes the path the last completed copy
 * recommends (more than 0.55 runs per point: coarse bins).  Captured builds neither ask nor copy.
 * PIGS_SAMPLES_ORDER=ordered|unordered in the environment overrules the memory (tests), as do the
 * PIGS_BUILD_POINTS_* flags of pigs_plan_build.  (The rules: csrc/build_choice.h, choose_build and OrderState; the
 * slot table behind the memory: csrc/build_memory.h.)
 * The same memory decides how pigs_plan_forward / pigs_plan_backward move the outputs / incoming gradients of
 * c = 1, orders (0, 1, 2) or (0, 1, trace) launches: directly through the points' original indices (lattices:
 * runs of consecutive indices), or -- points in no order -- through one 32-byte record per point in the plan
 * workspace and a streaming launch that deals the records out / gathers them (from 524 288 points, where it
 * starts to pay; PIGS_STAGE=0|1 overrules). */
int pigs_samples_build(void* samples_ws, size_t samples_ws_bytes, int64_t M, const void* samples, void* stream);
/* what the library currently remembers for builds of M points on the current device: 1 = coarse bins,
 * 0 = one pass, -1 = nothing yet (introspection for tools and tests) */
int pigs_samples_order_hint(int64_t M);
/* Introspection for tools and tests (additive to ABI 10: the number does not change).  Once point sets of M points have
 * been the same compact lattice on the same box for 64 verified builds and three statistic copies in a row, a build
 * with PIGS_BUILD_SAMPLES that keeps the Gaussians' order into a clean plan workspace no longer looks at the points in
 * front of its list launch (a TRUSTED build: two launches instead of four; never inside a capture).  Results do not
 * depend on it; the list launch checks every tile against the remembered box and the library goes back to looking
 * within 8 builds of points that are no such lattice.  PIGS_LATTICE_TRUST=0 / 1 in the environment, read at every
 * build: never / as soon as a row length and a stable box are remembered.  (csrc/build_choice.h: `trusted` in
 * choose_build, OrderState::trusts; tests/test_build_choice.py holds both on a CPU.)
 *   info[0] = 1 when the library's memory of M points on the current device would let the next build be trusted (the
 *             samples' side of the decision; the Gaussians' side is the build's own), else 0
 *   info[1] = trusted builds of this size so far
 *   info[2] = times the list launch's check turned this size's memory around
 *   info[3] = verified builds in the current run of agreeing statistic copies */
int pigs_samples_trust_info(int64_t M, int64_t info[4]);

/* plan workspace.  `flags`:
 *   PIGS_BUILD_SAMPLES       also (re)builds the samples workspace from `samples` in the same launches
 *                            (5 in all); without it the samples workspace must be built already, or be
 *                            being built earlier on the same stream (`samples` is not read then).
 *   PIGS_BUILD_PLAN_WS_CLEAN the plan workspace's counters are known to be zero: it was the target of
 *                            an earlier pigs_plan_build with the same (N, M, c) that has completed or
 *                            precedes this call on the same stream (every build leaves them zeroed),
 *                            or the caller zero-filled it.  Saves the zeroing launch of a build on an
 *                            existing samples workspace (4 launches instead of 5); ignored together
 *                            with PIGS_BUILD_SAMPLES, whose first launch zeroes anyway.
 * (ABI 4 called this parameter build_samples: 0 / 1 keep their meaning.)
 *   PIGS_BUILD_DEBUG_NO_LOOKBACK  test hook: the in-kernel scans never use their workgroup-to-workgroup
 *                            hand-over and take the recompute path everywhere (see pigs_*_error_offset);
 *                            results are the same, the build is slower.
 *   PIGS_BUILD_POINTS_ORDERED / PIGS_BUILD_POINTS_UNORDERED  (with PIGS_BUILD_SAMPLES) the caller knows how its
 *                            points arrive: take the one-pass / the coarse-bin samples build whatever the
 *                            library remembers (see pigs_samples_build); neither flag: the library decides. */
#define PIGS_BUILD_SAMPLES 1
#define PIGS_BUILD_PLAN_WS_CLEAN 2
#define PIGS_BUILD_DEBUG_NO_LOOKBACK 4
#define PIGS_BUILD_POINTS_ORDERED 8
#define PIGS_BUILD_POINTS_UNORDERED 16
/* ABI 7.  PIGS_BUILD_DEFER_LISTS: the build stops in front of its last launch, the tile lists; the FIRST
 * pigs_plan_forward / pigs_plan_backward / pigs_residual_* call on this plan workspace builds them -- a forward
 * (orders 0..2, orders 0, 1 + trace, order 0, the residual; c = 1, and orders 0..2 for c = 2) in the SAME launch
 * as its own evaluation: a wave builds the lists of its four tiles and samples them at once, so the latency-bound
 * list build hides behind the arithmetic of the other waves and one kernel boundary goes away (the reference's
 * pattern: preprocess, then sample_*(), model_pn.py:768-772).  The lists are written out as ever; every further
 * call reads them.  The library remembers which workspaces are waiting by their address (every build into a
 * workspace sets or clears the mark, the first sampling call clears it); the first sampling call must be stream
 * ordered behind the build, like any use of the plan.  PIGS_NO_FUSED_FIRST in the environment keeps the list
 * build in a launch of its own (A/B runs). */
#define PIGS_BUILD_DEFER_LISTS 32
/* ABI 9.  PIGS_BUILD_FORWARD_ONLY: the caller will not differentiate through this plan (grad mode off, or none of
 * means / values / conics requires grad).  The plan then serves pigs_plan_forward and pigs_residual_forward only:
 * the build sizes everything with ONE cut-off, q_max (q_max_backward is ignored), and writes the group lists the
 * forward reads but no tile lists and no wide masks.  Forward results are those of a full plan (bit for bit where
 * the Gaussians keep the caller's order, PlanParams::strips; the same sums in another order otherwise).
 * The plan records the flag in its own workspace; pigs_plan_backward / pigs_residual_backward on such a plan write
 * NaN gradients (the entry points cannot tell without waiting for the device, so they launch as ever; no list of
 * the plan is read out of bounds).  Ignored together with PIGS_BUILD_DEFER_LISTS. */
#define PIGS_BUILD_FORWARD_ONLY 64
int pigs_plan_build(void* workspace, size_t workspace_bytes, void* samples_ws, size_t samples_ws_bytes,
                    int flags, int64_t N, int64_t M, int c, float q_max, float q_max_backward,
                    const void* means, const void* conics, const void* values, const void* samples, void* stream);

int pigs_plan_forward(void* workspace, size_t workspace_bytes, const void* samples_ws, size_t samples_ws_bytes,
                      int64_t N, int64_t M, int c, float q_max,
                      int orders_mask, void* out0, void* out1, void* out2, void* out3, void* stream);

int pigs_plan_backward(void* workspace, size_t workspace_bytes, const void* samples_ws, size_t samples_ws_bytes,
                       int64_t N, int64_t M, int c, float q_max, int orders_mask,
                       const void* gout0, const void* gout1, const void* gout2, const void* gout3,
                       void* g_means, void* g_conics, void* g_values, void* stream);

/*
 * Linear residual of the sampled field in ONE launch (extension): the diffusion
 * residuals of the reference's losses (model_pn.py:612-617, 834-849; test_no_mlp.py:127-144) are
 *     r[m][c] = a0 u + a1x du/dx + a1y du/dy + aL (u_xx + u_yy) - target[m][c]
 * with constant coefficients `coeffs` = {a0, a1x, a1y, aL} (HOST doubles) and an optional `target`
 * [M][c] (device; e.g. u_prev / dt): 4 bytes per point and channel leave the kernel instead of the 28 of
 * u, grad u and the Hessian, and the loss is one elementwise + reduction on r.  The backward takes the
 * gradient gout [M][c] that arrives at r and returns the gradients wrt means, conics, values (the three
 * buffers are overwritten; d r / d target = -1 is the caller's).  plan_ws == NULL: dense (d in {1,2},
 * f32 / f64); else through a built plan (d = 2, f32; backward with the plan's wide cut-off).
 */
int pigs_residual_forward(int dtype, int d, int c, int64_t N, int64_t M,
                          const void* means, const void* conics, const void* values, const void* samples,
                          const double coeffs[4], const void* target, void* out,
                          void* plan_ws, size_t plan_ws_bytes, const void* samples_ws, size_t samples_ws_bytes, void* stream);
int pigs_residual_backward(int dtype, int d, int c, int64_t N, int64_t M,
                           const void* means, const void* conics, const void* values, const void* samples,
                           const double coeffs[4], const void* gout, void* g_means, void* g_conics, void* g_values,
                           void* plan_ws, size_t plan_ws_bytes, const void* samples_ws, size_t samples_ws_bytes, void* stream);

/*
 * General residual in ONE launch (additive to ABI 10): per-point coefficients and an advection term,
 *     w_i(m)   = sum_c' advect_by[i][c'] u_c'(x_m)
 *     r[m][ch] = a0_m u_ch + sum_i a1_{m,i} d_i u_ch + aL_m lap u_ch + adv_m sum_i w_i(m) d_i u_ch - target[m][ch]
 * -- the reference's time-blended losses (model_pn.py:794-805, IntegrationRule.TRAPEZOID; the random time weight
 * per point of test_no_mlp.py:122-144) and the Burgers term u u_x.  Each of a0, a1, aL, adv is the HOST double of
 * `terms` where its field pointer is NULL, else a DEVICE field in the call's dtype, contiguous: a0_pt [M],
 * a1_pt [M][d], aL_pt [M], adv_pt [M] (per point, shared by the channels).  advect_by is d x c host constants
 * (rows i < d, columns c' < c are read).  target [M][c] or NULL; out [M][c].
 * aux [M][1+d][c] or NULL: the forward also writes u (row 0) and d_i u (rows 1..d) of every point there; the
 * backward reads them to form the gradients that arrive at u and grad u through the advection term.  The backward
 * therefore needs the aux of THE SAME forward (same inputs, same plan) whenever advection is active (adv != 0 or
 * adv_pt), and the coefficient fields must stay unmodified between the forward and its backward.  The backward
 * returns the gradients wrt means, conics, values (overwritten); d r / d target = -1 is the caller's; there are no
 * gradients wrt the coefficient fields.  plan_ws == NULL: dense (d in {1,2}, c <= 4, f32 / f64); else through a built
 * plan (d = 2, f32, c <= 2; backward with the plan's wide cut-off; on a PIGS_BUILD_FORWARD_ONLY plan the backward
 * writes NaN gradients, as pigs_residual_backward does).
 */
typedef struct PigsResidualTerms {
    double a0, a1[2], aL, adv;                   /* used where the field pointer is NULL */
    double advect_by[2][4];                      /* B[i][c'] */
    const void *a0_pt, *a1_pt, *aL_pt, *adv_pt;  /* device fields or NULL */
} PigsResidualTerms;
int pigs_residual_terms_forward(int dtype, int d, int c, int64_t N, int64_t M,
                                const void* means, const void* conics, const void* values, const void* samples,
                                const PigsResidualTerms* terms, const void* target, void* out, void* aux,
                                void* plan_ws, size_t plan_ws_bytes, const void* samples_ws, size_t samples_ws_bytes,
                                void* stream);
int pigs_residual_terms_backward(int dtype, int d, int c, int64_t N, int64_t M,
                                 const void* means, const void* conics, const void* values, const void* samples,
                                 const PigsResidualTerms* terms, const void* gout, const void* aux,
                                 void* g_means, void* g_conics, void* g_values,
                                 void* plan_ws, size_t plan_ws_bytes, const void* samples_ws, size_t samples_ws_bytes,
                                 void* stream);

/*
 * Coupled residual in ONE launch (additive to ABI 10): the channels mixed by two constant c x c matrices under a
 * per-point weight,
 *     r[m][ch] = a0_m u_ch + aL_m lap u_ch
 *              + cw_m sum_c' ( couple0[ch][c'] u_c' + couple_lap[ch][c'] lap u_c' ) - target[m][ch]
 * -- the reference's wave system (test_no_mlp.py:127-139: res0 = u_t[0] - ub[1], res1 = u_t[1] - (10 lap ub[0] - 0.1 ub[1])
 * with ub blended by a random weight per point; model_pn.py:623-627, 843-845), which no coefficient shared by the
 * channels expresses.  Each of a0, aL, cw is the HOST double of `coupling` where its field pointer is NULL, else a
 * DEVICE field [M] in the call's dtype, contiguous.  couple0 and couple_lap are host constants, row = output channel,
 * column = input channel (rows and columns < c are read).  target [M][c] or NULL; out [M][c].  Only u and the
 * trace are accumulated (2 c sums per point).  The backward takes gout [M][c] and returns the gradients wrt means,
 * conics, values (overwritten); it is linear in the field, so it needs nothing of the forward, but the coefficient
 * fields must stay unmodified between the forward and its backward; d r / d target = -1 is the caller's; there are no
 * gradients wrt the coefficients.  c = 1 is PIGS_ERR_UNSUPPORTED (nothing to couple).  plan_ws == NULL: dense
 * (d in {1,2}, c in {2,3,4}, f32 / f64); else through a built plan (d = 2, f32, c = 2; backward with the plan's wide
 * cut-off; on a PIGS_BUILD_FORWARD_ONLY plan the backward writes NaN gradients, as pigs_residual_backward does).
 */
typedef struct PigsResidualCoupling {
    double a0, aL, cw;                      /* used where the field pointer is NULL */
    double couple0[4][4], couple_lap[4][4]; /* [ch][c'] */
    const void *a0_pt, *aL_pt, *cw_pt;      /* device fields [M] or NULL */
} PigsResidualCoupling;
int pigs_residual_coupled_forward(int dtype, int d, int c, int64_t N, int64_t M,
                                  const void* means, const void* conics, const void* values, const void* samples,
                                  const PigsResidualCoupling* coupling, const void* target, void* out,
                                  void* plan_ws, size_t plan_ws_bytes, const void* samples_ws, size_t samples_ws_bytes,
                                  void* stream);
int pigs_residual_coupled_backward(int dtype, int d, int c, int64_t N, int64_t M,
                                   const void* means, const void* conics, const void* values, const void* samples,
                                   const PigsResidualCoupling* coupling, const void* gout,
                                   void* g_means, void* g_conics, void* g_values,
                                   void* plan_ws, size_t plan_ws_bytes, const void* samples_ws, size_t samples_ws_bytes,
                                   void* stream);

/*
 * The vorticity terms of a two-channel field u = (u_x, u_y) in two dimensions in ONE launch (additive to ABI 10;
 * d = 2 and c = 2 are implied): one packed row per point,
 *     out[m][0..6] = (u_x, u_y, div u, w, w_x, w_y, lap w),   w = d_x u_y - d_y u_x,
 * -- the seven numbers the reference's Navier-Stokes problem keeps of orders 0..3 of its field: Model.forward
 * (model_pn.py:650-659) and Model.sample / compute_loss (model_pn.py:770-781, 801-805, 817-849), with
 * div = ux[:,0,0] + ux[:,1,1] (:848), w = ux[:,0,1] - ux[:,1,0] (:779), wx = uxx[...,0,1] - uxx[...,1,0] (:655, :780)
 * and lap w = wxx[:,0,0] + wxx[:,1,1] of wxx = uxxx[...,0,1] - uxxx[...,1,0] (:656, :781, :630).  Each is a sum over
 * the pairs: 7 accumulators and 28 B per point (float32) instead of the 30 and 120 B of orders 0..3.
 * means [N][2], conics [N][3], values [N][2], samples [M][2]; out and gout [M][7], contiguous.  The backward is the
 * backward of orders 0..3 with the incoming gradients formed from gout; it overwrites g_means [N][2], g_conics [N][3],
 * g_values [N][2].  plan_ws == NULL: dense (f32 / f64, the launch variants of every other mask); else through a built
 * plan (f32; the caller builds it with the cut-off it wants for third derivatives; backward with the plan's wide
 * cut-off; on a PIGS_BUILD_FORWARD_ONLY plan the backward writes NaN gradients, as pigs_residual_backward does).
 */
int pigs_vorticity_forward(int dtype, int64_t N, int64_t M,
                           const void* means, const void* conics, const void* values, const void* samples, void* out,
                           void* plan_ws, size_t plan_ws_bytes, const void* samples_ws, size_t samples_ws_bytes, void* stream);
int pigs_vorticity_backward(int dtype, int64_t N, int64_t M,
                            const void* means, const void* conics, const void* values, const void* samples, const void* gout,
                            void* g_means, void* g_conics, void* g_values,
                            void* plan_ws, size_t plan_ws_bytes, const void* samples_ws, size_t samples_ws_bytes, void* stream);

/*
 * The Navier-Stokes residual in the vorticity formulation in ONE launch (additive to ABI 10; d = 2 and c = 2 are
 * implied).  With `now` = the seven vorticity terms of the Gaussians at point m (the row of pigs_vorticity_forward),
 * prev[m][0..6] the same seven of the previous time level (device, contiguous [M][7]; NULL reads as zeros) and
 * tau = params->tau, or tau_pt[m] where tau_pt is not NULL (a DEVICE field [M] in the call's dtype):
 *     X_b       = tau X_now + (1 - tau) X_prev            for X in u_x, u_y, div, w_x, w_y, lap_w
 *     out[m][0] = div_b
 *     out[m][1] = time_term (w_now - w_prev) - dt (nu lap_w_b - (u_x_b w_x_b + u_y_b w_y_b))
 * -- compute_loss of the reference's model for Problem.NAVIER_STOKES (model_pn.py:794-818, 629-631, 830, 848-849):
 * tau per point is IntegrationRule.TRAPEZOID, tau = 1 BACKWARD, tau = 0 FORWARD; time_term = 0, dt = -1 and no prev
 * give column 1 = nu lap_w - u . grad w, the sample_pde of Model.forward (:655-659).  out and gout are [M][2].
 * aux [M][4] or NULL: the forward also writes (u_x_b, u_y_b, w_x_b, w_y_b) there; the backward reads gout, tau and the
 * aux of THE SAME forward (not prev) and needs it whenever M > 0; tau_pt must stay unmodified in between.  The backward
 * overwrites g_means [N][2], g_conics [N][3], g_values [N][2]; there are no gradients wrt prev, tau or the samples.
 * plan_ws == NULL: dense (f32 / f64); else through a built plan (f32; built with the cut-off wanted for third
 * derivatives; backward with the plan's wide cut-off; on a PIGS_BUILD_FORWARD_ONLY plan the backward writes NaN
 * gradients, as pigs_residual_backward does).
 */
typedef struct PigsVorticityResidual {
    double nu, dt, time_term, tau;          /* tau: used where tau_pt is NULL */
    const void* tau_pt;                     /* device field [M] or NULL */
} PigsVorticityResidual;
int pigs_vorticity_residual_forward(int dtype, int64_t N, int64_t M,
                                    const void* means, const void* conics, const void* values, const void* samples,
                                    const PigsVorticityResidual* params, const void* prev, void* out, void* aux,
                                    void* plan_ws, size_t plan_ws_bytes, const void* samples_ws, size_t samples_ws_bytes,
                                    void* stream);
int pigs_vorticity_residual_backward(int dtype, int64_t N, int64_t M,
                                     const void* means, const void* conics, const void* values, const void* samples,
                                     const PigsVorticityResidual* params, const void* gout, const void* aux,
                                     void* g_means, void* g_conics, void* g_values,
                                     void* plan_ws, size_t plan_ws_bytes, const void* samples_ws, size_t samples_ws_bytes,
                                     void* stream);

/*
 * The vorticity residual with a data term as a third column, from the same seven sums in the same launch (additive to
 * ABI 10; d = 2 and c = 2 are implied).  Everything of pigs_vorticity_residual_* holds, and in addition
 *     out[m][2] = data_weight (w_now[m] - data[m])
 * with w_now the vorticity of the CURRENT level (not blended) and data a DEVICE array [M] in the call's dtype -- the
 * recon_loss of the reference's Navier-Stokes loop (main_pn.py:209-210; data_weight = sqrt(5)) and, with nu = dt =
 * time_term = 0, the loss of its initialisation fit (test_initialize.py:135-136).  out and gout are [M][3].  The
 * backward differs in one line: the gradient that arrives at w is gout[m][1] time_term + gout[m][2] data_weight; it
 * reads neither prev nor data, and there is no gradient wrt data.  A NULL params or a NULL data in the forward is
 * PIGS_ERR_INVALID, as is a backward with M > 0 and no aux; through a plan float64 is PIGS_ERR_UNSUPPORTED; on a
 * PIGS_BUILD_FORWARD_ONLY plan the backward writes NaN gradients.
 */
typedef struct PigsVorticityFit {
    double nu, dt, time_term, tau, data_weight;      /* tau: used where tau_pt is NULL */
    const void* tau_pt;                              /* device field [M] or NULL */
    const void* data;                                /* device array [M]; the forward reads it */
} PigsVorticityFit;
int pigs_vorticity_fit_forward(int dtype, int64_t N, int64_t M,
                               const void* means, const void* conics, const void* values, const void* samples,
                               const PigsVorticityFit* params, const void* prev, void* out, void* aux,
                               void* plan_ws, size_t plan_ws_bytes, const void* samples_ws, size_t samples_ws_bytes,
                               void* stream);
int pigs_vorticity_fit_backward(int dtype, int64_t N, int64_t M,
                                const void* means, const void* conics, const void* values, const void* samples,
                                const PigsVorticityFit* params, const void* gout, const void* aux,
                                void* g_means, void* g_conics, void* g_values,
                                void* plan_ws, size_t plan_ws_bytes, const void* samples_ws, size_t samples_ws_bytes,
                                void* stream);

/*
 * The pixel of an image under every sample point, in one launch (additive to ABI 10): image [H][W] (dtype_image),
 * samples [M][2] (dtype_samples), out [M] (dtype_image), all on the device and contiguous.  With every operation
 * rounded once in the samples' dtype, a true division and no contraction,
 *     tx = (x - lo) / (hi - lo) * W,  ix = clamp(trunc(tx), 0, W - 1)         (ty, iy with H likewise)
 *     out[m] = image[iy][ix]
 * -- `((samples + 1) / 2 * res).to(long).clamp(0, res - 1)`, `coords[:, 1] * res + coords[:, 0]` and `torch.take` of the
 * reference (main_pn.py:206-207, 210) for lo = -1, hi = 1 and a square image, bit for bit.  A non-finite coordinate reads
 * pixel 0 of its axis.  Checked before any HIP call: a dtype other than PIGS_F32 / PIGS_F64, H or W above 2^24 or more
 * than 2^31 - 1 blocks of 256 points is PIGS_ERR_UNSUPPORTED; H or W < 1, M < 0, hi <= lo (also after rounding to the
 * samples' dtype), a non-finite box or a NULL array with M > 0 is PIGS_ERR_INVALID.  M = 0 returns PIGS_OK without a
 * launch.  Nothing allocates, frees or synchronises.
 */
int pigs_grid_lookup(int dtype_image, int dtype_samples, int64_t H, int64_t W, int64_t M, double lo, double hi,
                     const void* image, const void* samples, void* out, void* stream);

/*
 * The network inputs in ONE launch (additive to ABI 10; d = 2; forward only): the four arrays that the reference's
 * Model.forward samples at its Gaussians' means under no_grad and hands to its dynamics network
 * (model_pn.py:645-664), in the layouts of those lines,
 *     sample_u   [M][c]        u
 *     sample_ux  [M][2][c]     d_i u_ch, the memory of the order-1 output
 *     sample_uxx [M][2][c]     u_xx of every channel, then u_yy (planar: the cat of :664), not the Hessian
 *     sample_pde [M][p]        pde_rhs (:612-631) by params->kind:
 *         PIGS_NET_ZERO           zeros                                          p = c   (Problem.TEST)
 *         PIGS_NET_DIFFUSION      u_xx + u_yy                                    p = c
 *         PIGS_NET_BURGERS        nu (u_xx + u_yy) - u_ch d_x u_ch               p = c
 *         PIGS_NET_WAVE           (u_1, wave[0] (u_xx + u_yy)_0 - wave[1] u_1)   c = 2, p = 2
 *         PIGS_NET_NAVIER_STOKES  nu lap w - (u_0 w_x + u_1 w_y),                c = 2, p = 1
 *                                 w = d_x u_y - d_y u_x
 * Only the sums these need are accumulated: 5 c per point, 13 for Navier-Stokes (orders 0..3 carry 30 at c = 2).
 * All four outputs are contiguous, in the call's dtype, and required when M > 0.  d != 2, or c != 2 with the wave or
 * Navier-Stokes kind, is PIGS_ERR_UNSUPPORTED; an unknown kind is PIGS_ERR_INVALID.  There is no backward: the model
 * calls it under no_grad.  plan_ws == NULL: dense (c <= 4, f32 / f64); else through a built plan (f32, c <= 2; for
 * Navier-Stokes the caller builds it with the cut-off it wants for third derivatives).
 */
#define PIGS_NET_ZERO 0
#define PIGS_NET_DIFFUSION 1
#define PIGS_NET_BURGERS 2
#define PIGS_NET_WAVE 3
#define PIGS_NET_NAVIER_STOKES 4
typedef struct PigsNetworkInputs {
    int kind;                               /* PIGS_NET_* */
    double nu, wave[2];                     /* burgers, navier_stokes: nu; wave: its two constants */
} PigsNetworkInputs;
int pigs_network_inputs_forward(int dtype, int d, int c, int64_t N, int64_t M,
                                const void* means, const void* conics, const void* values, const void* samples,
                                const PigsNetworkInputs* params, void* sample_u, void* sample_ux, void* sample_uxx,
                                void* sample_pde,
                                void* plan_ws, size_t plan_ws_bytes, const void* samples_ws, size_t samples_ws_bytes,
                                void* stream);

/* Byte offset, inside a samples / plan workspace, of a uint32 DIAGNOSTIC that a build leaves at 0 and
 * sets to non-zero when a workgroup of its in-kernel scan did not receive a predecessor's total within
 * the bounded wait and summed that predecessor's counters itself.  The result is valid either way
 * (the counters are final before the scan starts); the flag only says that the slow path ran -- never
 * observed with the hardware's in-order dispatch, always with PIGS_BUILD_DEBUG_NO_LOOKBACK.
 * (ABI <= 5: the scan gave up instead and this word meant "workspace invalid".) */
size_t pigs_samples_error_offset(void);
size_t pigs_plan_error_offset(void);

/* ABI 7.  Byte offset, inside a samples workspace, of two uint32 {rf, rs} that a samples build leaves behind:
 * non-zero when the points were taken in INDEX-TILED order -- they arrived as an rf x rs lattice in row order
 * (rf points along the fastest axis; both multiples of 8: meshgrid(indexing="xy").reshape(-1, 2),
 * test_gaussian_sampling.py:43-46, main_pn.py:317-324), so a point's tile (an 8 x 8 index patch) and group (4 x 4)
 * are index arithmetic: the build neither keys, counts, scans, scatters NOR COPIES the points -- and {0, 0} when
 * they were sorted into cells.  The decision is the build's own, on the device (the first backward step of the
 * fastest coordinate gives rf; the largest steps between index neighbours along and across rows bound every index
 * tile, which must stay within twice its share of the bounding box) for point sets of 4 096 points and more;
 * results never depend on it; PIGS_LATTICE=0 / 1 in the environment: never / at every size.
 * When the library expects a lattice (the last completed build of this size was one) and that build and the one before it
 * had the same bounding box, pigs_plan_build with PIGS_BUILD_SAMPLES | PIGS_BUILD_PLAN_WS_CLEAN bins the Gaussians on
 * the REMEMBERED box beside its first look at the points (one launch fewer, two with Gaussians in strips, below; a grid's
 * domain steers the quality of the binning, never a result; PIGS_NO_AHEAD in the environment switches it off).
 * CONTRACT that comes with it: a samples workspace in index-tiled order holds the ADDRESS of `samples`, not the
 * points; pigs_plan_build / pigs_plan_forward / pigs_plan_backward / pigs_residual_* read the caller's array
 * through it.  `samples` must therefore stay allocated and unmodified for as long as the samples workspace is
 * used (the sorted order has no such requirement; a caller that cannot promise it sets PIGS_LATTICE=0). */
size_t pigs_samples_lattice_offset(void);

/* Byte offset, inside a PLAN workspace, of one uint32: non-zero when the build kept the Gaussians in the CALLER's
 * order (ABI 8).  Gaussians whose order in the arrays is already spatial -- the reference lays them out on a meshgrid
 * (model_pn.py:338-342) and training moves them by fractions of a spacing -- are not binned into grid cells: every
 * 16 consecutive ones are a strip with a bounding box (16 strips a super-strip), and the tile lists are built from
 * those boxes; no count, scan or scatter launch.  The library measures in every build how many times over the strips cover
 * the samples' domain and decides the next build of the same sizes from the last completed measurement (at most 64 times: strips);
 * always correct whatever the order, results never depend on it beyond the order of a list's entries;
 * PIGS_GAUSS_STRIPS=0 / 1 in the environment: never / always. */
size_t pigs_plan_strips_offset(void);

/* Introspection for tools and tests (never needed to use a plan): where the tile lists sit inside a
 * plan workspace.  info[0] = tiles, info[1] = entries per list slab, info[2] = byte offset of the
 * tile headers (8 uint32 each: [0] = count | mode << 30; mode 0 = list of `count` entries `sorted
 * Gaussian index | wide group mask << 24 | narrow group mask << 28`, mode 1 = `count` record ranges
 * {first, length}, mode 2 = group lists only; [1..4] = the lengths of the four group lists), info[3] = byte offset of the tile-list slabs (uint32[tiles][slab]),
 * info[4] = byte offset of the sorted -> caller Gaussian index table (uint32[N]), info[5] = byte
 * offset of the group-list slabs (uint32[tiles][4][slab], sorted Gaussian indices).
 * Returns PIGS_ERR_UNSUPPORTED for sizes the binned path does not take (N >= 2^24 among them). */
int pigs_plan_layout_info(int64_t N, int64_t M, int c, int64_t info[6]);

/* ... and where the Gaussians' half of a plan sits (additive to ABI 10; tools and tests): info[0] = byte offset of the
 * records in the plan's order (float4[2 N + 2]: {mux, muy, a, b}, {c, v0, v1, 0}; record N is all zero), info[1] = byte
 * offset of the strip boxes (float4[ceil(N / 16)]: {min x, min y, max x, max y}), info[2] = byte offset of the
 * super-strip boxes (float4[ceil(N / 256)]); both kinds of boxes are written by builds that keep the caller's order
 * alone (pigs_plan_strips_offset).  info[3] = 0. */
int pigs_plan_records_info(int64_t N, int64_t M, int c, int64_t info[4]);

/* The same for a samples workspace (additive to ABI 10): where the points sit in the order the sampling kernels take
 * them.  info[0] = tiles (64 consecutive sorted points each, four groups of 16), info[1] = byte offset of the sorted
 * points, info[2] = bytes per sorted point ({float x, y; uint32 m}: the coordinates and the point's index in the
 * caller's array; positions behind the last point of a ragged last tile are not written), info[3] = 0.  Meaningful
 * when the build sorted the points into cells: in index-tiled order ({rf, rs} at pigs_samples_lattice_offset non-zero)
 * the workspace holds no points, tile t is the 8 x 8 index patch the serpentine of pair-rows puts at position t and
 * group g of it the 4 x 4 patch (g & 1, g >> 1).
 * Returns PIGS_ERR_UNSUPPORTED for sizes the binned path does not take. */
int pigs_samples_layout_info(int64_t M, int64_t info[4]);

/*
 * ABI 10.  Periodic domain [lo, lo + period)^2, d = 2, f32 / f64, c in 1..4.  A periodic sampler sums, for every
 * point x, the 3 x 3 images of every Gaussian:
 *     u(x) = sum_n sum_{k in {-1,0,1}^2} v_n exp(-1/2 (x - mu'_n - k period)^T C_n (x - mu'_n - k period)),
 *     mu'_n = lo + (mu_n - lo) - period floor((mu_n - lo) / period)     (the mean wrapped into the box; d mu'/d mu = 1).
 * In floating point mu'_n lies in the CLOSED box [lo, lo + period]: a mean just below lo lands on lo + period, the same
 * point of the torus (a remainder that comes out negative -- (mu - lo) / period underflowing to -0 -- gets one period).
 * Sample points are not wrapped.  For x in the closed box this is the periodic field exactly (up to the cut-off)
 * when every Gaussian's q <= q_cut ellipse spans less than one period on each axis: q_cut Sigma_ii < period^2,
 * Sigma = C^-1, with q_cut the widest cut-off the caller samples with.
 *
 * pigs_periodic_images: means [N][2], conics [N][3], values [N][c] -> img_means [9N][2], img_conics [9N][3],
 *   img_values [9N][c], the arrays the caller then binds (pigs_sample_*, pigs_plan_build, pigs_residual_*) in place
 *   of the originals.  Image j of Gaussian n is row j*N + n.  Block j = 0 holds the wrapped originals; blocks 1..8
 *   the shifts k = (kx, ky) = (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1).  Every block keeps the
 *   caller's order, so Gaussians laid out on a lattice stay in spatial strips (pigs_plan_strips_offset) in each.
 *   A Gaussian whose ellipse reaches one period (or whose conic is not positive definite, or whose mean is not
 *   finite) sets *flag (uint32, zeroed by the caller; one atomic OR per wave at most) to non-zero; the images are
 *   written as ever.  flag may be NULL.
 * pigs_periodic_images_backward: the fold -- g_means[n] = sum_j g_img_means[j*N + n], likewise for conics and values,
 *   summed over j = 0..8 in order without atomics (bitwise reproducible).  A NULL incoming array reads as zero; the
 *   three outputs are overwritten.
 * Arguments are checked before any HIP call: a bad dtype or c is PIGS_ERR_UNSUPPORTED; a negative N, null arrays
 * with N > 0, a period that is not finite and positive, a non-finite lo or a q_cut that is not finite and positive
 * are PIGS_ERR_INVALID.
 */
int pigs_periodic_images(int dtype, int c, int64_t N, double lo, double period, double q_cut,
                         const void* means, const void* conics, const void* values,
                         void* img_means, void* img_conics, void* img_values, uint32_t* flag, void* stream);
int pigs_periodic_images_backward(int dtype, int c, int64_t N,
                                  const void* g_img_means, const void* g_img_conics, const void* g_img_values,
                                  void* g_means, void* g_conics, void* g_values, void* stream);

/*
 * preprocess_aggregate() / aggregate_neighbors() -- GaussianSampler methods of the reference
 * (model_pn.py:257-264; test_neighbor_aggregation.py:75-98).  PARITY UNPINNED: their arithmetic exists
 * only in the reference's absent CUDA source; these entry points implement this repository's own
 * definition (DESIGN.md "aggregate_neighbors"; pigs_amd/csrc/aggregate.hip), d = 2, float32 / float64:
 *   neighbours of i = { j : (mu_i - mu_j)^T C_j (mu_i - mu_j) <= q_max };  a_ij = softmax_j <queries_i, keys_j> / sqrt(K);
 *   out_i = sum_j a_ij (transform features_j + distance_transform [e_ij ; g_ij e_ij]),  e_ij = Fourier embedding
 *   of mu_j - mu_i with `frequencies` (E = 4F + 1 entries), g_ij = exp(-q_ij / 2).
 * The neighbour relation is kept as index lists -- `cap` int32 slots per Gaussian, by rows (the j of an
 * i) and by columns (the i that hold a j).
 *
 * pigs_aggregate_lists: counts [N] and lists [N][cap] by rows and by columns.  Up to N = 2048 every pair
 *   is tested (two launches, lists ascending, `workspace` and `flags` unused: cap = N can never overflow and
 *   needs no counting pass); beyond, through the sampler's multi-level Gaussian grid in `workspace`
 *   (pigs_aggregate_workspace_bytes(dtype, N) bytes, 256-byte aligned; 0 = unsupported N): `flags` & PIGS_AGGREGATE_BUILD_GRID (re)builds the grid from
 *   `means` / `conics` first (4 launches; float64 inputs are binned through float32 copies with a
 *   widened cut-off -- the grid only nominates candidates, every pair is tested in the caller's dtype),
 *   without it the workspace must hold the grid of the same Gaussians.
 *   PRECONDITION of the float64 grid build, not checked: the cut-off is widened by 5 %, which covers a displacement
 *   of sqrt(q) by 0.148 at q_max = 36; the float32 copies move a difference of centres by up to 2 sqrt(2) 2^-24
 *   max|mu|, so every Gaussian's smallest standard deviation along any axis must stay above that / 0.148
 *   ~ 1.14e-6 max|mu| (8e-4 for centres near (300, -700)).  A narrower Gaussian can lose neighbours.
 *   With row_lists == col_lists == NULL only the counts are written (the FULL list lengths: the caller sizes
 *   `cap` from their maximum, then calls again with the lists).  *overflow (int32, zeroed by the caller) is set when a list did not fit
 *   `cap` (it is then truncated).  List order is the grid's (not ascending; may differ between builds).
 * pigs_aggregate_forward: out [N][L], and for the backward lse [N] (log-sum-exp of the scaled scores)
 *   and acc [N][L + 2E] = (sum_j a_ij features_j ; sum_j a_ij [e_ij ; g_ij e_ij]).
 * pigs_aggregate_backward: the whole backward from gout [N][L] (4 launches; 5 for N > 2048): all six
 *   gradients -- g_features [N][L], g_transform [L][L], g_queries [N][K], g_keys [N][K], g_frequencies [F],
 *   g_distance_transform [L][2E].  `scratch` (pigs_aggregate_backward_scratch_bytes(dtype, N, L, F) bytes)
 *   holds dacc = gout [transform | distance_transform], D_i = <dacc_i, acc_i> and the per-row shares of the
 *   frequency gradient between the launches.  The per-Gaussian gradients are gathers (no atomics); the
 *   three sums over the Gaussians are plain sums up to N = 2048 and atomic sums of 2048-Gaussian
 *   partials beyond.
 * Sizes: L + 2E <= 128, L + K <= 128, K + F <= 128 (two components per lane), and the three sampling kernels' dynamic
 *   LDS -- sizeof(T) * 4 * region values, region = max(64 ((L + 4F) | 1), 136) in the forward, the same with
 *   (L + K) | 1 in the backward by columns, 136 + the same with (K + F) | 1 in the backward by rows -- must fit a
 *   CU's PIGS_AGGREGATE_LDS_MAX bytes.  Every float32 shape of the first rule does (at most 134 272 B); in float64
 *   the strides are limited to 79 in the forward and the backward by columns (e.g. L + K <= 79) and to 77 in the
 *   backward by rows (K + F <= 77).  pigs_aggregate_lds_bytes(dtype, L, K, F) is the largest of
 *   the three (0: a size out of range).  pigs_aggregate_forward applies all of this, the backward's kernels
 *   included -- a forward that could never be differentiated is refused -- and so does pigs_aggregate_backward:
 *   PIGS_ERR_UNSUPPORTED before any HIP call.  (pigs_aggregate_lds_bytes is additive to ABI 10.)
 * pigs_aggregate_grid_info: introspection for tests (never needed to use the lists; additive to ABI 10).  After a grid
 *   build (N > 2048) info[0] = byte offset inside `workspace` of a uint32 whose bit l is set when level l of the grid
 *   holds a Gaussian, info[1] = the grid's levels (the top one, a single cell, is level info[1] - 1).
 *   PIGS_ERR_UNSUPPORTED where pigs_aggregate_lists builds no grid.
 */
#define PIGS_AGGREGATE_BUILD_GRID 1
#define PIGS_AGGREGATE_LDS_MAX 163840
size_t pigs_aggregate_workspace_bytes(int dtype, int64_t N);
size_t pigs_aggregate_lds_bytes(int dtype, int L, int K, int F);
int pigs_aggregate_grid_info(int dtype, int64_t N, int64_t info[2]);
int pigs_aggregate_lists(int dtype, int64_t N, int64_t cap, const void* means, const void* conics, double q_max,
                         void* workspace, size_t workspace_bytes, int flags,
                         int32_t* row_counts, int32_t* row_lists, int32_t* col_counts, int32_t* col_lists,
                         int32_t* overflow, void* stream);

int pigs_aggregate_forward(int dtype, int64_t N, int64_t cap, int L, int K, int F,
                           const void* means, const void* conics, const int32_t* row_counts, const int32_t* row_lists,
                           const void* features, const void* transform, const void* queries, const void* keys,
                           const void* frequencies, const void* distance_transform,
                           void* out, void* lse, void* acc, void* stream);

size_t pigs_aggregate_backward_scratch_bytes(int dtype, int64_t N, int L, int F);
int pigs_aggregate_backward(int dtype, int64_t N, int64_t cap, int L, int K, int F,
                            const void* means, const void* conics, const int32_t* row_counts, const int32_t* row_lists,
                            const int32_t* col_counts, const int32_t* col_lists,
                            const void* features, const void* transform, const void* queries, const void* keys,
                            const void* frequencies, const void* distance_transform,
                            const void* lse, const void* acc, const void* gout, void* scratch, size_t scratch_bytes,
                            void* g_features, void* g_transform, void* g_queries, void* g_keys, void* g_frequencies,
                            void* g_distance_transform, void* stream);

/*
 * The same on the torus [lo, lo + period)^2 of pigs_periodic_images (additive to ABI 10: the number does not change).
 * The neighbours of i are the PAIRS (j, k), image k = 0..8 of Gaussian j in the block order of pigs_periodic_images
 * (k = 0: no shift), with (mu'_i - mu'_j - s_k L)^T C_j (mu'_i - mu'_j - s_k L) <= q_max, L = period: every pair is
 * a neighbour of its own (offset mu'_j + s_k L - mu'_i, its own density and softmax entry, keys and features of j),
 * i.e. the definition above applied to the 9N images, rows of block 0.  One j may appear through several images
 * (half extents between L/2 and L), so a list can be LONGER THAN N: `cap` = N is not safe here, take the counting
 * pass (lists == NULL) or check *overflow.
 * PRECONDITIONS, neither of which is checked here: (1) `means` are already wrapped into [lo, lo + period] (the closed
 * box: a centre on lo + period is admitted, the culls carry a margin for it) -- block 0
 * of pigs_periodic_images (with its conics); nothing is wrapped here.  (2) Every Gaussian's q <= q_max ellipse spans
 * less than one period on each axis, sqrt(q_max Sigma_ii) < period -- what the flag of pigs_periodic_images reports
 * for q_cut >= q_max.  The all-pairs build (N <= 2048) relies on both: it tests only the four shifts that can then
 * reach.  With unwrapped means or a wider Gaussian it drops pairs silently, while the grid build (N > 2048), which
 * tries all nine shifts, would still find them: the two builds then differ, and neither gives the periodic relation
 * (a second-neighbour image would be needed).  A list entry is j | k << 28 (row lists: (j, k); column lists: (i, k) with the k
 * of the row entry of that pair; sum of col_counts = sum of row_counts); N >= 2^28 is PIGS_ERR_UNSUPPORTED.  Lists
 * built here are read by the two _periodic sampling entries only, and those read no others.  Up to N = 2048 a
 * pair costs four tests (only the shifts towards each other can reach) and lists ascend in (j, k); beyond, the grid
 * of the wrapped centres is walked once per shift that can reach.  A period that is not finite and positive or a
 * non-finite lo is PIGS_ERR_INVALID (checked before any HIP call).  The means are constants: no gradient.
 */
int pigs_aggregate_lists_periodic(int dtype, int64_t N, int64_t cap, const void* means, const void* conics, double q_max,
                                  double lo, double period, void* workspace, size_t workspace_bytes, int flags,
                                  int32_t* row_counts, int32_t* row_lists, int32_t* col_counts, int32_t* col_lists,
                                  int32_t* overflow, void* stream);
int pigs_aggregate_forward_periodic(int dtype, int64_t N, int64_t cap, int L, int K, int F, double period,
                                    const void* means, const void* conics, const int32_t* row_counts,
                                    const int32_t* row_lists, const void* features, const void* transform,
                                    const void* queries, const void* keys, const void* frequencies,
                                    const void* distance_transform, void* out, void* lse, void* acc, void* stream);
int pigs_aggregate_backward_periodic(int dtype, int64_t N, int64_t cap, int L, int K, int F, double period,
                                     const void* means, const void* conics, const int32_t* row_counts,
                                     const int32_t* row_lists, const int32_t* col_counts, const int32_t* col_lists,
                                     const void* features, const void* transform, const void* queries, const void* keys,
                                     const void* frequencies, const void* distance_transform, const void* lse,
                                     const void* acc, const void* gout, void* scratch, size_t scratch_bytes,
                                     void* g_features, void* g_transform, void* g_queries, void* g_keys,
                                     void* g_frequencies, void* g_distance_transform, void* stream);

/*
 * All H heads of an attention layer in one launch (additive to ABI 10: the number does not change).  The heads share
 * `features`, `frequencies` and the lists; head h has transform_h, distance_transform_h and its own queries and keys:
 *   out[:, h, :] = pigs_aggregate_forward(features, transforms[h], queries[:, h], keys[:, h], frequencies,
 *                                         distance_transforms[h])          for h < H,
 * what a pair's geometry gives (list entry, q, g, the 4F sin / cos values, the features row) being computed once.
 * Layouts (row-major): features [N][L]; transforms [H][L][L]; queries, keys [N][H][K] (a Gaussian's H rows are
 *   contiguous); frequencies [F]; distance_transforms [H][L][2E].  The forward writes out [N][H][L], lse [N][H] and
 *   acc [N][H][L + 2E].  The backward takes gout [N][H][L] and writes g_features [N][L] and g_frequencies [F] (both
 *   the sums over the heads), g_transforms [H][L][L], g_queries, g_keys [N][H][K], g_distance_transforms [H][L][2E];
 *   `scratch` (pigs_aggregate_heads_backward_scratch_bytes(dtype, N, H, L, F) bytes) holds dacc [N][H][L + 2E],
 *   D [N][H] and the per-row shares of the frequency gradient [N][F].  Launches and the sums over N as in
 *   pigs_aggregate_backward.
 * `period` = 0: lists of pigs_aggregate_lists; > 0: lists of pigs_aggregate_lists_periodic on a torus of that period
 *   (its preconditions hold); anything else is PIGS_ERR_INVALID.
 * Sizes: 1 <= H <= PIGS_AGGREGATE_HEADS_MAX (else PIGS_ERR_UNSUPPORTED).  H = 1 is pigs_aggregate_forward / _backward (the same
 *   kernels; at H = 1 the rule below is theirs).  At most 128 components per kernel -- L + 2E <= 128, H K + F <= 128, H (L + K) <= 128 -- and the dynamic LDS
 *   of each kernel, sizeof(T) * 4 * region values, within PIGS_AGGREGATE_LDS_MAX: region = max(64 ((L + 4F) | 1), 136 H)
 *   in the forward, 136 H + max(64 ((H K + F) | 1), 136) in the backward by rows, max(64 ((H (L + K)) | 1), 136) in the
 *   backward by columns.  pigs_aggregate_heads_lds_bytes is the whole rule in one call: the largest of the three, or 0
 *   when an argument, H or a component count is out of range -- a shape is admitted when 0 < bytes <= PIGS_AGGREGATE_LDS_MAX.
 *   Both entries check all of it before any HIP call (PIGS_ERR_UNSUPPORTED; the forward refuses a shape whose
 *   backward could not run) and return after the check when N = 0.  H separate pigs_aggregate_forward calls remain
 *   available for a refused shape.
 */
#define PIGS_AGGREGATE_HEADS_MAX 4
size_t pigs_aggregate_heads_lds_bytes(int dtype, int H, int L, int K, int F);
size_t pigs_aggregate_heads_backward_scratch_bytes(int dtype, int64_t N, int H, int L, int F);
int pigs_aggregate_heads_forward(int dtype, int64_t N, int64_t cap, int H, int L, int K, int F, double period,
                                 const void* means, const void* conics, const int32_t* row_counts,
                                 const int32_t* row_lists, const void* features, const void* transforms,
                                 const void* queries, const void* keys, const void* frequencies,
                                 const void* distance_transforms, void* out, void* lse, void* acc, void* stream);
int pigs_aggregate_heads_backward(int dtype, int64_t N, int64_t cap, int H, int L, int K, int F, double period,
                                  const void* means, const void* conics, const int32_t* row_counts,
                                  const int32_t* row_lists, const int32_t* col_counts, const int32_t* col_lists,
                                  const void* features, const void* transforms, const void* queries, const void* keys,
                                  const void* frequencies, const void* distance_transforms, const void* lse,
                                  const void* acc, const void* gout, void* scratch, size_t scratch_bytes,
                                  void* g_features, void* g_transforms, void* g_queries, void* g_keys,
                                  void* g_frequencies, void* g_distance_transforms, void* stream);

/*
 * Refinement: prune and split (or clone) Gaussians on the device (additive to ABI 10: the number does not change).
 * d = 2, float32 / float64.  Replaces the boolean indexing, torch.linalg.eig, repeat_interleave and cat of
 * Model.forward(split=True) / Model.split (model_pn.py:703-714, :578-605; PIGS_REFINE_SPLIT) and of the
 * densification block of test_no_mlp.py:198-240 (PIGS_REFINE_CLONE).
 *
 * Inputs: means [N][2], scaling [N][2] (variances), transforms [N] (raw correlation t), values [N][c], and two masks
 *   of one byte per row, nonzero = true: keep (NULL = all rows) and split (NULL = none).  The effective split set is
 *   split & keep.  With n_k kept rows and n_s effective split rows both modes give n_k + n_s output rows:
 *   PIGS_REFINE_SPLIT  the rows with keep & ~split in input order, then for every split parent in input order its two
 *                      children (mean - e, mean + e), adjacent, values = value_scale * v, scaling and transforms copied.
 *                      e = lambda_max * v of the covariance [[s0, tau], [tau, s1]], tau = tanh(t) sqrt(s0 s1): the UNIT
 *                      eigenvector times the eigenVALUE (model_pn.py:587-589), signed so that e_x > 0, or e_x = 0 and
 *                      e_y > 0; an exactly isotropic covariance gives e = (lambda, 0).
 *   PIGS_REFINE_CLONE  all kept rows in input order, then one unchanged copy of every split parent in input order.
 *
 * pigs_refine_index classifies and ranks the rows: kept_pos [N] (int64) = the output row of a row's kept copy, child_pos
 *   [N] (int64) = the output row of its first child or of its copy, -1 where there is none; counts [2] (int64, device) =
 *   {n_k, n_s}.  The caller reads `counts` to size the outputs; that read is the path's only host wait.  Three launches:
 *   totals per workgroup of PIGS_REFINE_ROWS rows, their exclusive scan by ONE workgroup that takes
 *   PIGS_REFINE_SCAN_WIDTH totals per pass, the ranks.  `workspace`: pigs_refine_workspace_bytes(N) bytes, 8-byte
 *   aligned (16 bytes per workgroup; a pure function of N; 0 for N <= 0 and for sizes the path does not take, N >= 2^31).
 * pigs_refine_apply writes the output rows and the two maps source [rows] (int64: the input row of every output row)
 *   and child [rows] (int32: -1 kept row, 0 / 1 the -e / +e child, 0 a copy).  `rows` is the length of the output
 *   arrays: every store is guarded by position < rows, so a `rows` smaller than n_k + n_s truncates the result and
 *   nothing is written behind it.  An output may be NULL (not wanted: source and child alone are the maps for arrays
 *   the library does not know); a wanted output needs its input, out_means in PIGS_REFINE_SPLIT needs scaling and
 *   transforms as well.  One launch, one thread per input row.
 * pigs_refine_backward gathers the gradients of the inputs, one thread per input row, no atomics: a pruned row 0, a kept
 *   row its output row's, a split parent the sum of its two children's (times value_scale for values), a clone parent
 *   its kept row's plus its copy's.  e is a constant (the reference computes it under no_grad, model_pn.py:584-585).
 *   Any incoming gradient may be NULL (zero), any outgoing one NULL (not wanted).  Positions >= rows count as zero.
 * Rows of means and scaling are read and written as one 8-byte (float32) / 16-byte (float64) access: those arrays
 *   are aligned to a row.
 * Arguments are checked before any HIP call: a bad dtype or mode, or N >= 2^31, is PIGS_ERR_UNSUPPORTED; a negative N or
 *   rows, c < 1, a null required array or a misaligned one with N > 0 is PIGS_ERR_INVALID; a short workspace is
 *   PIGS_ERR_WORKSPACE.  N = 0 (and rows = 0 in apply) returns PIGS_OK without a launch -- pigs_refine_index then leaves
 *   `counts` unwritten: both totals are 0.  Nothing allocates, frees or synchronises.
 */
#define PIGS_REFINE_SPLIT 0
#define PIGS_REFINE_CLONE 1
#define PIGS_REFINE_ROWS 1024
#define PIGS_REFINE_SCAN_WIDTH 256
size_t pigs_refine_workspace_bytes(int64_t N);
int pigs_refine_index(int mode, int64_t N, const uint8_t* keep, const uint8_t* split, void* workspace,
                      size_t workspace_bytes, int64_t* kept_pos, int64_t* child_pos, int64_t* counts, void* stream);
int pigs_refine_apply(int dtype, int mode, int c, int64_t N, int64_t rows, double value_scale, const int64_t* kept_pos,
                      const int64_t* child_pos, const void* means, const void* scaling, const void* transforms,
                      const void* values, void* out_means, void* out_scaling, void* out_transforms, void* out_values,
                      int64_t* source, int32_t* child, void* stream);
int pigs_refine_backward(int dtype, int mode, int c, int64_t N, int64_t rows, double value_scale, const int64_t* kept_pos,
                         const int64_t* child_pos, const void* g_out_means, const void* g_out_scaling,
                         const void* g_out_transforms, const void* g_out_values, void* g_means, void* g_scaling,
                         void* g_transforms, void* g_values, void* stream);

/*
 * The split criteria: which Gaussians to refine, as a byte mask on the device (additive to ABI 10: the number does not
 * change).  float32 / float64.  Replaces the element-wise chain, the reductions and the full sort of torch.quantile in
 * Model.forward(split=True) (model_pn.py:733-754; the three sampling passes of :719-737 stay the sampler's) and the
 * threshold of the densification block (test_no_mlp.py:203-205).  The mask goes straight into pigs_refine_index.
 *
 * pigs_criterion_quantile_mask.  Inputs, row-major: sample_u [n][c] (the current field at the current means),
 *   prev_sample_u [n][c] (the previous field there), density [n] (a field of ones there), boundary_mask [n] (one byte
 *   per row, nonzero = true; NULL = all).  In the inputs' dtype, each step one IEEE operation, no contraction:
 *     w[i]   = 1 - (D[i] - min D) / max D
 *     m[i,k] = ((u[i,k] - u_prev[i,k]) * (u[i,k] - u_prev[i,k])) * w[i]
 *     L = n c,  pos = q (L - 1) in double,  lo = floor(pos),  hi = min(lo + 1, L - 1),  x = sort(m)
 *     quantile = x[lo] + (x[hi] - x[lo]) (pos - lo)        in double, rounded once: torch.quantile's linear rule
 *     mask[i] = any_k(m[i,k] > quantile) and boundary_mask[i]        (0 / 1)
 *   x[lo] and x[hi] are selected elements, bit for bit: a most-significant-digit-first radix select (8-bit digits) on
 *   the order-preserving unsigned image of the float bits, so -0.0, negatives, denormals and +inf sort as IEEE
 *   compares them.  A NaN in m (or in D: min and max propagate it) is found by a flag of its own: quantile, x_lo and
 *   x_hi are then NaN and the mask is all 0.  L = 1: quantile = x[0], mask all 0 (the compare is strict).
 *   metric [n][c] (m; or NULL) and stats (4 values of the dtype: quantile, x_lo, x_hi, 1 if a NaN was seen else 0; or
 *   NULL) are optional outputs.
 * pigs_criterion_meanstd_mask.  threshold = mean(score) + k std(score), std unbiased (n - 1) as torch.std; mean and the
 *   sum of squared deviations in double, two passes, mean first, the threshold rounded once; mask[i] = score[i] >
 *   threshold and keep[i] (NULL = all).  n = 1 (std NaN) and a NaN score give an all-0 mask.  stats (or NULL):
 *   threshold, mean, std.
 * variant: PIGS_CRITERION_AUTO; PIGS_CRITERION_ONE_WORKGROUP, ONE launch of one workgroup with the keys in LDS, for
 *   n c <= PIGS_CRITERION_LDS_VALUES (pigs_criterion_lds_values() returns the library's; PIGS_ERR_UNSUPPORTED above);
 *   PIGS_CRITERION_MANY_WORKGROUPS for any n c <= 2^24: quantile 6 launches in float32, 10 in float64 (min / max
 *   partials; metric + first digit; one per remaining digit; finish), mean/std 3.  AUTO takes the first where it
 *   fits.  The variants agree bit for bit in the quantile rule.  Cross-workgroup sums are per-workgroup partials or
 *   integer adds on histogram bins: every output is a pure function of the inputs.
 * workspace: pigs_criterion_workspace_bytes(dtype, n, c) bytes (c = 1 for mean/std), 8-byte aligned; read and written by
 *   the many-workgroup variant only (the one-workgroup variant takes NULL).  A pure function, monotone in n c; 0 for
 *   n <= 0, c < 1, a bad dtype and n c > 2^24.
 * Arguments are checked before any HIP call: a bad dtype or variant, or n c > 2^24 (torch.quantile refuses the same),
 *   is PIGS_ERR_UNSUPPORTED; a negative n, c < 1, q outside [0, 1] or NaN (k NaN), or a null required array with n > 0
 *   is PIGS_ERR_INVALID; a short workspace is PIGS_ERR_WORKSPACE.  n = 0 returns PIGS_OK without a launch.  Nothing
 *   allocates, frees, synchronises or waits for another workgroup: both entries can be captured into a graph.
 */
#define PIGS_CRITERION_AUTO 0
#define PIGS_CRITERION_ONE_WORKGROUP 1
#define PIGS_CRITERION_MANY_WORKGROUPS 2
#define PIGS_CRITERION_LDS_VALUES 16384      /* float64 keys: 128 KiB of the 160 KiB of LDS of a CU */
int pigs_criterion_lds_values(void);
size_t pigs_criterion_workspace_bytes(int dtype, int64_t n, int c);
int pigs_criterion_quantile_mask(int dtype, int variant, int c, int64_t n, double q, const void* sample_u,
                                 const void* prev_sample_u, const void* density, const uint8_t* boundary_mask,
                                 void* workspace, size_t workspace_bytes, void* metric, void* stats, uint8_t* mask,
                                 void* stream);
int pigs_criterion_meanstd_mask(int dtype, int variant, int64_t n, double k, const void* score, const uint8_t* keep,
                                void* workspace, size_t workspace_bytes, void* stats, uint8_t* mask, void* stream);

/*
 * The optimiser of the MLP-free loops: the Gaussians' parameterisation, its chain rule and Adam in one launch
 * (additive to ABI 10: the number does not change).  d = 2, c = 1..4, float32 / float64.  Replaces, per training step,
 * tanh(raw_means) * scale and exp(raw_scaling) (test_no_mlp.py:99-104, test_initialize.py:100-104), build_covariances
 * (gaussians.py:163-193), the autograd backward of each, torch.optim.Adam over four tensors with zero_grad
 * (test_no_mlp.py:146, 185-186, test_initialize.py:80-85, 151, 172-173) and the periodic wrap of the means
 * (test_initialize.py:175-180, model_pn.py:689-693).
 *
 * Parameters: raw_means [N][2], values [N][c], raw_scaling [N][2], transform [N].  The Gaussians they stand for:
 *   means        PIGS_OPTIM_MEANS_TANH: tanh(raw_means) * scale;  PIGS_OPTIM_MEANS_IDENTITY: raw_means
 *   s = exp(raw_scaling), h = tanh(transform), covariances (s0, h sqrt(s0 s1), s1), conics their inverses, flat
 *   (xx, xy, yy); 1 / (1 - h^2) and sech^2 are formed from exp(-2 |x|), never from a cancelling subtraction.
 *
 * pigs_optim_materialize writes means [N][2], covariances [N][3] and conics [N][3] from the parameters: one launch.
 * pigs_optim_step, one launch of one thread per Gaussian (two with a device state, see below):
 *   1. the chain rule from g_means [N][2], g_covariances [N][3], g_conics [N][3] (gradients with respect to the arrays
 *      pigs_optim_materialize wrote) to the raw parameters; g_values [N][c] passes through;
 *   2. Adam as torch.optim.Adam defines it, per group g in (means, values, scaling, transform):
 *        m <- beta1 m + (1 - beta1) g,  v <- beta2 v + (1 - beta2) g^2,
 *        p <- p - lr[g] / (1 - beta1_pow[g]) * m / (sqrt(v) / sqrt(1 - beta2_pow[g]) + eps),
 *      in place on the parameters, exp_avg and exp_avg_sq (arrays of the parameters' shapes);
 *   3. with hyper->wrap, a coordinate of raw_means > wrap_hi is lowered by wrap_hi - wrap_lo and one < wrap_lo raised by
 *      it: one shift, strict inequalities;
 *   4. means, covariances and conics of the UPDATED parameters, as pigs_optim_materialize would write them, bit for bit.
 *   A null gradient leaves its group untouched: g_means the means, g_values the values, g_covariances and g_conics
 *   BOTH null the scaling and the transform (one of them null counts as zero).  The outputs are always written.
 *   beta1_pow[g] / beta2_pow[g] are beta1^t / beta2^t of the step being taken, kept by the caller as running products
 *   in double.  With hyper->device_state (12 doubles on the device: beta1_pow[4], beta2_pow[4], steps[4]; initially
 *   1, 1, 0) the entry ignores the two host arrays and first launches ONE thread that multiplies the products of the
 *   groups that have a gradient by beta1 / beta2 and adds 1 to their step counts; the update reads them from there.
 *   With hyper->device_lr (4 doubles on the device) the rates are read from there.  Nothing in the update waits for
 *   another workgroup.  Both ways the bias corrections are formed on the device by the same double operations.
 * Arguments are checked before any HIP call: a bad dtype or means_map, or c outside 1..4, is PIGS_ERR_UNSUPPORTED;
 *   N <= 0, a null hyper, parameter, moment or output array, all four gradients null, or a raw_means / raw_scaling
 *   array (or its moments, g_means, means) not aligned to a row is PIGS_ERR_INVALID.  Nothing allocates, frees or
 *   synchronises.
 */
#define PIGS_OPTIM_MEANS_TANH 0
#define PIGS_OPTIM_MEANS_IDENTITY 1
typedef struct PigsAdamStep {
    double lr[4];                     /* means, values, scaling, transform */
    double beta1, beta2, eps;
    double beta1_pow[4], beta2_pow[4];
    double scale;                     /* PIGS_OPTIM_MEANS_TANH */
    double wrap_lo, wrap_hi;
    int means_map, wrap;
    const double* device_lr;          /* [4] on the device, or NULL */
    double* device_state;             /* [12] on the device, or NULL */
} PigsAdamStep;
int pigs_optim_materialize(int dtype, int means_map, int64_t N, double scale, const void* raw_means,
                           const void* raw_scaling, const void* transform, void* means, void* covariances, void* conics,
                           void* stream);
int pigs_optim_step(int dtype, int c, int64_t N, const PigsAdamStep* hyper, void* raw_means, void* values,
                    void* raw_scaling, void* transform, void* exp_avg_means, void* exp_avg_values, void* exp_avg_scaling,
                    void* exp_avg_transform, void* exp_avg_sq_means, void* exp_avg_sq_values, void* exp_avg_sq_scaling,
                    void* exp_avg_sq_transform, const void* g_means, const void* g_values, const void* g_covariances,
                    const void* g_conics, void* means, void* covariances, void* conics, void* stream);

/*
 * The optimiser's gradient statistics and its d = 1 form (additive to ABI 10: the number does not change; PigsAdamStep,
 * pigs_optim_materialize and pigs_optim_step are as they were).
 *
 * Statistics.  The densification of the MLP-free loops thresholds sums of the RAW parameters' gradients, which with
 * pigs_optim_step exist only in the kernel's registers.  With G_m = dL/d raw_means and G_s = dL/d raw_scaling after the
 * chain rule, exactly as Adam consumes them, a step with a PigsGradStats does, per Gaussian and for a group whose
 * gradient is present (means: g_means; scaling: g_covariances or g_conics):
 *      last_mean_grad  = G_m,  mean_grad  += G_m,  mean_grad_norm  += || mean_grad ||_2     (the sum AFTER adding)
 *      last_scale_grad = G_s,  scale_grad += G_s,  scale_grad_norm += || scale_grad ||_2
 *   in the same launch; this replaces test_no_mlp.py:149-155 and test_no_mlp_1d.py:156-162 (mean_grad += raw_means.grad,
 *   mean_grad_norm += torch.norm(mean_grad, dim=-1), the same pair for the scaling) and the reads of raw_means.grad /
 *   scaling.grad in test_initialize.py:156-158 and test_initialize_1d.py:68-71.  The arrays have the parameters' dtype:
 *   mean_grad, scale_grad, last_* [N][d], the two norms [N] (d = 1: the norm is |x|).  An absent group's arrays are not
 *   touched.  Parameters, moments and outputs are bit for bit those of a step without statistics.
 *   device_counts: NULL, or 2 doubles on the device (steps counted for means, scaling; the counter of :155 / :162); it
 *   needs hyper->device_state, and the ONE-thread launch that advances the products adds 1 to the count of each present
 *   group.  Without a device state the caller counts.
 * pigs_optim_step_stats: pigs_optim_step's arguments, then the statistics (not NULL).  One launch, two with a device state.
 *
 * d = 1 (test_no_mlp_1d.py:109-111, 189-190; test_initialize_1d.py:54-56, 75-76): parameters raw_means [N], values [N][c],
 *   raw_scaling [N]; three groups in slots 0..2 of PigsAdamStep's arrays and of the device state (slot 3 is not used).
 *   means = tanh(raw_means) * scale or raw_means (with the wrap), s = exp(raw_scaling), covariances = s, conics = 1 / s.
 *   Chain rule: d raw_means = g_means * scale * sech^2(raw_means); d raw_scaling = g_covariances * s - g_conics / s (one of
 *   the two NULL counts as zero, both NULL skip the group).  Adam, the wrap, the null-gradient rule, the running products
 *   and the outputs of the UPDATED parameters as for d = 2.
 * pigs_optim1d_materialize writes means, covariances, conics [N] each: one launch.
 * pigs_optim1d_step: one launch (two with a device state); stats is NULL or as above.
 *
 * Refusals, before any HIP call, as for pigs_optim_step; in addition a NULL statistics array, device_counts without
 * hyper->device_state or off 8 bytes, a NULL stats for pigs_optim_step_stats, or (d = 2) a mean_grad / scale_grad /
 * last_* array not aligned to a row is PIGS_ERR_INVALID.
 */
typedef struct PigsGradStats {
    void *mean_grad, *mean_grad_norm, *scale_grad, *scale_grad_norm, *last_mean_grad, *last_scale_grad;
    double* device_counts;            /* [2] on the device (means, scaling), or NULL */
} PigsGradStats;
int pigs_optim_step_stats(int dtype, int c, int64_t N, const PigsAdamStep* hyper, void* raw_means, void* values,
                          void* raw_scaling, void* transform, void* exp_avg_means, void* exp_avg_values,
                          void* exp_avg_scaling, void* exp_avg_transform, void* exp_avg_sq_means, void* exp_avg_sq_values,
                          void* exp_avg_sq_scaling, void* exp_avg_sq_transform, const void* g_means, const void* g_values,
                          const void* g_covariances, const void* g_conics, void* means, void* covariances, void* conics,
                          const PigsGradStats* stats, void* stream);
int pigs_optim1d_materialize(int dtype, int means_map, int64_t N, double scale, const void* raw_means,
                             const void* raw_scaling, void* means, void* covariances, void* conics, void* stream);
int pigs_optim1d_step(int dtype, int c, int64_t N, const PigsAdamStep* hyper, void* raw_means, void* values,
                      void* raw_scaling, void* exp_avg_means, void* exp_avg_values, void* exp_avg_scaling,
                      void* exp_avg_sq_means, void* exp_avg_sq_values, void* exp_avg_sq_scaling, const void* g_means,
                      const void* g_values, const void* g_covariances, const void* g_conics, void* means, void* covariances,
                      void* conics, const PigsGradStats* stats, void* stream);

/*
 * The optimiser of the loop with the network: Adam over up to 128 small tensors in two launches, and the loss-weighted
 * rate of that loop on the device (additive to ABI 10: the number does not change).  float32 / float64, all tensors
 * alike.  Replaces, per time step of main_pn.py:171-232, torch.optim.Adam(model.parameters()).step() (:59, :222; the
 * reference's DynamicsNetwork is 90 trainable tensors of some 30 000 elements), the rate g["lr"] = g["prev_lr"] *
 * loss_weight (:217-218) and loss_weight *= exp(-epsilon * current_loss.item()) (:225), whose device read it removes
 * together with those of total_loss (:227) and all_sufficient (:228).
 *
 * The state, pigs_network_adam_state_doubles(S) = 4 + 5 S doubles on the device, aligned to 8 bytes:
 *   [0] rate_scale (initially 1)   [1] loss_sum   [2] loss_max   [3] loss_count        (initially 0)
 *   then five arrays of S: steps (0), beta1_pow (1), beta2_pow (1), step_size, bc2_sqrt (the last two are written before
 *   they are read).
 * The moments, exp_avg and exp_avg_sq: ONE flat array each, in the parameters' dtype, aligned to 16 bytes.  Tensor s
 * owns counts[s] elements from offset seg[s], seg[0] = 0, seg[s + 1] = seg[s] + counts[s] rounded up to a multiple of 4
 * (the padding is never read or written); the arrays hold seg[S] elements.
 *
 * pigs_network_adam_step, two launches on `stream`; a tensor takes part when grads[s] is not NULL:
 *   1. one wave, lanes over the tensors.  Per present tensor, in double:
 *        steps[s] += 1,  beta1_pow[s] *= beta1,  beta2_pow[s] *= beta2,
 *        step_size[s] = rate / (1 - beta1_pow[s]),  bc2_sqrt[s] = sqrt(1 - beta2_pow[s]),
 *      rate = lr * rate_scale, lr = *dev_lr when dev_lr is not NULL.  Then, when `loss` is not NULL (one float32 or
 *      float64 on the device, loss_dtype PIGS_F32 / PIGS_F64), one lane does, in double,
 *        rate_scale *= exp(-decay * loss),  loss_sum += loss,  loss_max = loss if loss > loss_max or loss is NaN,
 *        loss_count += 1:
 *      the step uses the rate from BEFORE the decay, the order of main_pn.py:217-225.  A non-finite loss has no special
 *      case: IEEE arithmetic gives what the reference's line gives (a NaN loss makes rate_scale, loss_sum and loss_max
 *      NaN, and they stay so until they are reset).
 *   2. workgroups of 256 threads over chunks of 1 024 elements of the present tensors (an absent tensor has none):
 *        m <- beta1 m + (1 - beta1) g,  v <- beta2 v + (1 - beta2) g^2,  p <- p - step_size m / (sqrt(v) / bc2_sqrt + eps)
 *      with the multiply-adds as explicit fma, in place on params[s] and the two flat arrays.  A tensor whose parameter and
 *      gradient are both aligned to 16 bytes is read and written 16 bytes at a time with a scalar tail, any other one
 *      element at a time; both ways give the same bits, and the bits do not depend on where the chunks fall.
 *   An absent tensor keeps its parameter, its moments, its step count and its running products, as torch.optim.Adam
 *   leaves a parameter whose .grad is None.  Nothing waits for another workgroup, allocates, frees or synchronises; the
 *   pointers travel in the launch's arguments, so a captured call replays with the addresses it was recorded with.
 * Refusals, before any HIP call.  PIGS_ERR_UNSUPPORTED: a dtype (or, with a loss, a loss_dtype) other than PIGS_F32 /
 *   PIGS_F64.  PIGS_ERR_INVALID: a NULL block; tensors < 1 or > PIGS_NETWORK_ADAM_MAX_TENSORS; a NULL parameter; a count
 *   <= 0; 2^31 elements or more in all (counted with the padding); every gradient NULL; a parameter or gradient not
 *   aligned to its element; a NULL state or one off 8 bytes; a NULL moment array or one off 16 bytes; a dev_lr off 8
 *   bytes; a loss not aligned to its type.  pigs_network_adam_state_doubles returns 0 for a count outside 1..128.
 */
#define PIGS_NETWORK_ADAM_MAX_TENSORS 128
typedef struct PigsNetworkAdam {
    int tensors;                                            /* S */
    int64_t counts[PIGS_NETWORK_ADAM_MAX_TENSORS];          /* elements per tensor */
    void* params[PIGS_NETWORK_ADAM_MAX_TENSORS];
    const void* grads[PIGS_NETWORK_ADAM_MAX_TENSORS];       /* NULL: the tensor sits this step out */
    double lr, beta1, beta2, eps;
    double decay;                                           /* read with a loss only */
    const double* dev_lr;                                   /* one double on the device, or NULL */
} PigsNetworkAdam;
int pigs_network_adam_state_doubles(int tensors);
int pigs_network_adam_step(int dtype, const PigsNetworkAdam* block, double* state, void* exp_avg, void* exp_avg_sq,
                           const void* loss, int loss_dtype, void* stream);

/*
 * The model's state update: the dynamics network's deltas applied to the Gaussians, the next covariances and the
 * conservation penalty (additive to ABI 10: the number does not change).  d = 2, c = 1..4, float32 / float64.
 * Replaces, per time step of the loop with the network (main_pn.py:171-232 driving model_pn.Model):
 *   model_pn.py:270-273  the four strided column slices of the network's output (and, in the backward, a zero tensor and
 *                        an add per slice);
 *   :677-682             six detach().clone() of the previous state: the inputs are never written, they ARE prev_*;
 *   :684-687             means + dmeans m, scaling exp(dscaling m), transforms + dtransforms m, u + du m;
 *   :689-693             the periodic wrap of the means, two boolean-index writes with a host wait each;
 *   :695-698             build_full_covariances and flatten_covariances;
 *   :878-882             mean(x[mask]^2) of the four delta blocks, a boolean indexing with a host wait each.
 *
 * Arrays, row-major: means [N][2], u [N][c], scaling [N][2], transforms [N], deltas [N][5 + c] in the network's own column
 * order (dmeans 0:2, dscaling 2:4, dtransforms 4:5, du 5:5+c), boundary_mask [N] (one byte per row, nonzero = a FREE
 * Gaussian, m = 1, as the reference uses it; zero = a boundary Gaussian, m = 0).
 *
 * pigs_advance_forward, two launches.  The first, one thread per Gaussian in workgroups of 256:
 *   means' = means + dmeans m,  scaling' = scaling exp(dscaling m),  transforms' = transforms + dtransforms m,
 *   u' = u + du m;  with `wrap`, a coordinate of means' > wrap_hi is lowered by wrap_hi - wrap_lo and one < wrap_lo
 *   raised by it: one shift, strict inequalities.  A boundary row copies its inputs bit for bit; its deltas take part in
 *   no arithmetic (they may be NaN or Inf).
 *   covariances [N][3], conics [N][3] of (scaling', transforms') with the expressions of pigs_build_covariances, bit for
 *   bit what it writes from out_scaling and out_transforms; full_covariances [N][2][2], full_conics [N][2][2] the same
 *   values, the xy entry stored twice.
 *   Each thread squares its row's deltas in double; a workgroup adds the four sums and the free-row count across each
 *   wave, then across its waves through LDS, and writes one record of PIGS_ADVANCE_RECORD doubles to `scratch`.
 * The second, one workgroup, adds the records in a fixed order and writes
 *   penalty[k] = sum over the free rows of the squares of block k / (n_free width_k),  widths 2, 2, 1, c,
 *   k = dmeans, dscaling, dtransforms, du, rounded once to the dtype; no free row gives NaN (0 / 0), as torch.mean of an
 *   empty tensor.  No float atomics: the penalty is a pure function of the inputs.  n_free stays in `scratch`.
 * pigs_advance_backward, one launch of one thread per Gaussian.  From gradients with respect to any subset of the nine
 *   outputs (a NULL one counts as zero) to g_means [N][2], g_u [N][c], g_scaling [N][2], g_transforms [N] and ONE packed
 *   g_deltas [N][5 + c] (a NULL one is not written).  It reads out_scaling, out_transforms, deltas, boundary_mask and the
 *   scratch of the forward.  The covariance terms are recomputed from (scaling', transforms') with the arithmetic of
 *   pigs_build_covariances_backward; a full-matrix gradient folds into the flat one, the xy entry receiving both
 *   off-diagonals.  The wrap passes its gradient through.  The penalty's share of g_deltas is
 *   2 x m g_penalty[k] / (n_free width_k).  A boundary row's g_deltas is exactly zero.
 * scratch: pigs_advance_scratch_bytes(N) bytes, 8-byte aligned (0 for N <= 0): record 0 the totals, record 1 + b the
 *   record of workgroup b.  The forward writes all of it; the backward reads it only with a g_penalty.
 * Rows of means, scaling, out_means, out_scaling, g_out_means, g_out_scaling, g_means and g_scaling are one 8-byte
 *   (float32) / 16-byte (float64) access: those arrays are aligned to a row.
 * Arguments are checked before any HIP call: a bad dtype or c outside 1..4 is PIGS_ERR_UNSUPPORTED; N <= 0, wrap with
 *   wrap_lo >= wrap_hi, a null required array (forward: every input, output and the scratch; backward: the four saved
 *   arrays, the scratch with a g_penalty, and all five gradients null) or a misaligned one is PIGS_ERR_INVALID; a short
 *   scratch is PIGS_ERR_WORKSPACE.  Nothing allocates, frees, synchronises or waits for another workgroup.
 */
#define PIGS_ADVANCE_RECORD 5
size_t pigs_advance_scratch_bytes(int64_t N);
int pigs_advance_forward(int dtype, int c, int64_t N, int wrap, double wrap_lo, double wrap_hi, const void* means,
                         const void* u, const void* scaling, const void* transforms, const void* deltas,
                         const uint8_t* boundary_mask, void* scratch, size_t scratch_bytes, void* out_means, void* out_u,
                         void* out_scaling, void* out_transforms, void* covariances, void* conics, void* full_covariances,
                         void* full_conics, void* penalty, void* stream);
int pigs_advance_backward(int dtype, int c, int64_t N, const void* out_scaling, const void* out_transforms,
                          const void* deltas, const uint8_t* boundary_mask, const void* scratch, const void* g_out_means,
                          const void* g_out_u, const void* g_out_scaling, const void* g_out_transforms,
                          const void* g_covariances, const void* g_conics, const void* g_full_covariances,
                          const void* g_full_conics, const void* g_penalty, void* g_means, void* g_u, void* g_scaling,
                          void* g_transforms, void* g_deltas, void* stream);

/*
 * The TEST problem's state terms (additive to ABI 10: the number does not change).  The eight
 * unweighted terms of Problem.TEST's pde_loss (model_pn.py:851-852), bc_loss (:854-861) and conservation_loss
 * (:866-876), which read the Gaussians' NEW state and the network's deltas and no sample: three `if torch.any(...)` and
 * about seventeen boolean indexings there, each with a host wait.  d = 2, c = 1..4, float32 / float64.
 *
 * Arrays, row-major: means [N][2] and u [N][c] of the new state (out_means, out_u of pigs_advance_forward), deltas
 * [N][5 + c] in the network's column order, boundary_mask [N] (one byte per row, nonzero = a FREE Gaussian).
 * Over the free rows, with F their count, y = means[.][1], dx, dy = deltas[.][0], deltas[.][1], du = deltas[.][5 .. 5 + c),
 * u0 = u[.][0], and LOW = {y < -wall}, HIGH = {y > wall}, MID = {|y| < wall}, strict compares in the dtype against wall
 * rounded to it (a row at +-wall or with a NaN height is in no set):
 *   terms[0]  sum (dy - u0 / drift)^2 / F                  u0 / drift divided in the dtype, drift rounded to it
 *   terms[1]  sum_LOW sum_c (u - 1)^2 / (|LOW| c)           0 when LOW is empty
 *   terms[2]  sum_HIGH sum_c (u + 1)^2 / (|HIGH| c)         0 when HIGH is empty
 *   terms[3]  sum dx^2 / F
 *   terms[4]  sum [(dx - mean dx)^2 + (dy - mean dy)^2] / (2 F)
 *   terms[5]  sum (y - mean y)^2 / F
 *   terms[6]  sum_MID (|u0| - 1)^2 / |MID|                  0 when MID is empty
 *   terms[7]  sum_MID sum_c du^2 / (|MID| c)                0 when MID is empty
 * each rounded once to the dtype; with F = 0 the entries 0, 3, 4, 5 are NaN (0 / 0, torch.mean of nothing).  A boundary
 * row is branched around: its state and deltas (NaN, Inf) reach neither a term nor a gradient.
 *
 * pigs_state_loss_forward.  Up to PIGS_STATE_LOSS_ONE_LAUNCH_ROWS rows: ONE launch of one workgroup (256 threads up to
 *   256 rows, else 1 024 threads of up to four rows each) that makes both passes: it adds F and the sums of dx, dy, y,
 *   takes K = sum / F as the centre and adds sum (x - K) and sum (x - K)^2 over the rows it kept in registers; the
 *   spread is sum (x - K)^2 - (sum (x - K))^2 / F, whose second part is a second-order correction.  Above the bound TWO
 *   launches: workgroups of 256 rows do the same about their own centres and write one record of
 *   PIGS_STATE_LOSS_RECORD doubles each; one workgroup then moves the records to one common centre and adds them in
 *   record order.  Accumulators are double, sums go across a wave by shuffles, across waves through LDS in wave order.
 *   No float atomics: the same inputs give the same bits.
 * pigs_state_loss_backward, one launch of one thread per Gaussian, from g_terms [8] on the device to g_means [N][2],
 *   g_u [N][c] and ONE packed g_deltas [N][5 + c] (a NULL one is not written).  The sets, their counts and the means are
 *   constants: it reads them from the statistics record.  A boundary row's gradients are exact zeros.
 * scratch: pigs_state_loss_scratch_bytes(N) bytes, 8-byte aligned (0 for N <= 0): PIGS_STATE_LOSS_STATS doubles
 *   F, |LOW|, |HIGH|, |MID|, mean dx, mean dy, mean y, 0; above the bound also ceil(N / 256) records.
 * Arguments are checked before any HIP call: a bad dtype or c outside 1..4 is PIGS_ERR_UNSUPPORTED; N <= 0, a wall that
 *   is negative or not finite, a drift that is zero or not finite, a null array (the backward: all three gradients
 *   null) or a scratch off 8 bytes is PIGS_ERR_INVALID; a short scratch is PIGS_ERR_WORKSPACE.  Nothing allocates, frees,
 *   synchronises or waits for another workgroup.
 */
#define PIGS_STATE_LOSS_ONE_LAUNCH_ROWS 4096
#define PIGS_STATE_LOSS_STATS 8
#define PIGS_STATE_LOSS_RECORD 20
size_t pigs_state_loss_scratch_bytes(int64_t N);
int pigs_state_loss_forward(int dtype, int c, int64_t N, double wall, double drift, const void* means, const void* u,
                            const void* deltas, const uint8_t* boundary_mask, void* scratch, size_t scratch_bytes,
                            void* terms, void* stream);
int pigs_state_loss_backward(int dtype, int c, int64_t N, double wall, double drift, const void* means, const void* u,
                             const void* deltas, const uint8_t* boundary_mask, const void* scratch, const void* g_terms,
                             void* g_means, void* g_u, void* g_deltas, void* stream);

/* ---- One per-Gaussian tanh network per launch (additive to ABI 10) ----------------------------
 * The three per-Gaussian nets of the dynamics network (model_pn.py:154-174 delta_net, :187-198 input_projection,
 * :203-226 the query / key transforms; nn.Tanh, :425-426): nn.Linear layers with tanh between them and none after the last,
 * applied row by row.  One net per call:
 *   a_0 = x [N][w_0];  a_{l+1} = tanh(a_l W_l^T + b_l) for l < L - 1;  y = a_{L-1} W_{L-1}^T + b_{L-1}  [N][w_L]
 * `widths` is a host array of L + 1 ints (w_0 .. w_L); `weights` and `biases` are host arrays of L device pointers, W_l
 * [w_{l+1}][w_l] and b_l [w_{l+1}] row-major in nn.Linear's layout.  1 <= L <= PIGS_MLP_MAX_LAYERS, every width in
 * 1..PIGS_MLP_MAX_WIDTH, float32 only.  The host arrays are read during the call and not kept.
 *
 * pigs_mlp_forward, one launch.  A wave takes 16 rows at a time and keeps the activations in the accumulator registers of
 *   v_mfma_f32_16x16x4_f32 from x to y; the weights are staged once per workgroup in LDS, padded with zeros to multiples
 *   of 16.  Each output is a float32 fmaf chain over the layer's inputs, started from the bias, in a fixed order.
 * pigs_mlp_backward, one launch, and a second one when any weight or bias gradient is wanted.  From g_y [N][w_L] to g_x
 *   [N][w_0], g_weights[l] and g_biases[l] (shapes of W_l, b_l); a NULL g_x, a NULL array or a NULL entry is not
 *   written.  The activations are recomputed from x: the forward saves nothing.  At most PIGS_MLP_MAX_RECORDS waves walk
 *   the row tiles in a fixed order, each adds its weight and bias gradients in registers and writes one record to
 *   `scratch`; the second launch adds the records in a fixed order (four interleaved partial sums per parameter, then
 *   (p0 + p1) + (p2 + p3)).  No float atomics: every output is a pure function of the inputs, bit for bit.
 * scratch: pigs_mlp_scratch_bytes(N, L, widths) bytes = min(ceil(N / 16), PIGS_MLP_MAX_RECORDS) records of
 *   sum_l w_{l+1} (w_l + 1) floats, 4-byte aligned; 0 for N <= 0 or an unsupported net.  Not read by the caller.
 * Arguments are checked before any HIP call: a dtype other than PIGS_F32, L or a width out of range is
 *   PIGS_ERR_UNSUPPORTED; N <= 0, a null required array (widths, x, weights, biases and their entries, y or g_y; the
 *   backward with no gradient wanted), or a null, misaligned or short scratch with a weight or bias gradient wanted is
 *   PIGS_ERR_INVALID.  Nothing allocates, frees, synchronises or waits for another workgroup.
 */
#define PIGS_MLP_MAX_LAYERS 6
#define PIGS_MLP_MAX_WIDTH 48
#define PIGS_MLP_MAX_RECORDS 256
size_t pigs_mlp_scratch_bytes(int64_t N, int L, const int* widths);
int pigs_mlp_forward(int dtype, int64_t N, int L, const int* widths, const void* x, const void* const* weights,
                     const void* const* biases, void* y, void* stream);
int pigs_mlp_backward(int dtype, int64_t N, int L, const int* widths, const void* x, const void* const* weights,
                      const void* const* biases, const void* g_y, void* scratch, size_t scratch_bytes, void* g_x,
                      void* const* g_weights, void* const* g_biases, void* stream);

/* ---- A bank of tanh networks of one shape over one input, per launch (additive to ABI 10) ------
 * The query_transform / key_transform nets of all attention heads (model_pn.py:203-226, used at :259-261) have one shape
 * and read the same features.  A bank is B such nets, 1 <= B <= PIGS_MLP_BANK_MAX_NETS, each a net of the pigs_mlp_*
 * block in every respect (the same L, the same widths w_0 .. w_L, float32), all applied to the same x [N][w_0].  With a
 * group count G that divides B,
 *   y [G][N][B / G][w_L]:   y[b / (B / G)][row][b % (B / G)][:] = net_b(x[row])
 * G = 1 gives [1][N][B][w_L]; B = 4, G = 2 with the nets in the order (q0, q1, k0, k1) gives y[0] = queries [N][H][K]
 * and y[1] = keys [N][H][K] of pigs_aggregate_heads_forward, contiguous, without a stack or a copy.
 * `widths` is a host array of L + 1 ints, the same for every net; `weights`, `biases`, `g_weights`, `g_biases` are host
 * arrays of B L device pointers, net b's layer l at index b L + l.  The host arrays are read during the call and not kept.
 *
 * pigs_mlp_bank_forward, one launch.  A workgroup belongs to one net: it stages that net's weights in LDS (the LDS need
 *   is that of one net: every net pigs_mlp_forward takes is taken for every B) and runs pigs_mlp_forward's chain; only
 *   the store differs.  y of net b has the bits of pigs_mlp_forward(x, net b).
 * pigs_mlp_bank_backward, at most two launches.  From g_y (the layout of y) to g_x [N][w_0] = sum_b g_x^(b), added in the
 *   order b = 0, 1, .., B - 1, and every g_weights / g_biases entry; a NULL g_x, a NULL array or a NULL entry is not
 *   written.  Launch 1 is pigs_mlp_backward's first launch per net, at most PIGS_MLP_MAX_RECORDS waves and records PER
 *   NET; net 0 writes its part of g_x into g_x, net b > 0 into the scratch.  Launch 2 adds every net's records in the order
 *   of pigs_mlp_backward and adds the parts into g_x element by element; it is left out when B = 1 and only g_x is wanted.
 *   A net with no gradient wanted is not run when g_x is not wanted either.  No float atomics: every output is a pure
 *   function of the inputs, bit for bit.
 * scratch: pigs_mlp_bank_scratch_bytes(N, B, L, widths) bytes = B pigs_mlp_scratch_bytes(N, L, widths) for the records,
 *   then (B - 1) N w_0 floats for the parts of g_x; 4-byte aligned; 0 for N <= 0 or an unsupported bank.  Needed with a
 *   weight or bias gradient wanted, and with g_x wanted when B > 1.  Not read by the caller.
 * Arguments are checked before any HIP call: a dtype other than PIGS_F32, L or a width out of range, or B outside
 *   1..PIGS_MLP_BANK_MAX_NETS is PIGS_ERR_UNSUPPORTED; G < 1 or G not dividing B, N <= 0, a null required array (widths,
 *   x, weights, biases and their entries, y or g_y; the backward with no gradient wanted), or a null, misaligned or short
 *   scratch when it is needed is PIGS_ERR_INVALID.  Nothing allocates, frees, synchronises or waits for another workgroup.
 */
#define PIGS_MLP_BANK_MAX_NETS 8
size_t pigs_mlp_bank_scratch_bytes(int64_t N, int B, int L, const int* widths);
int pigs_mlp_bank_forward(int dtype, int64_t N, int B, int G, int L, const int* widths, const void* x,
                          const void* const* weights, const void* const* biases, void* y, void* stream);
int pigs_mlp_bank_backward(int dtype, int64_t N, int B, int G, int L, const int* widths, const void* x,
                           const void* const* weights, const void* const* biases, const void* g_y, void* scratch,
                           size_t scratch_bytes, void* g_x, void* const* g_weights, void* const* g_biases, void* stream);

/* ---- A tanh network over a row that lies in several arrays, with block means (additive to ABI 10) -
 * delta_net reads the features and the heads' neighbour features side by side (model_pn.py:265-268, a cat), and
 * magnitude_loss (:892-901) is the mean square of each head's block of that joined row.  Here the net of the pigs_mlp_*
 * block in every respect (L, widths, weights, biases, float32) takes its input row as P arrays, 1 <= P <=
 * PIGS_MLP_JOINED_MAX_PARTS:
 *   x[row] = (parts[0][row], .., parts[P-1][row]),  parts[p] [N][part_widths[p]] row-major,  sum_p part_widths[p] = widths[0]
 *   y [N][w_L] = the net of x, with the bits of pigs_mlp_forward on the joined array.
 * `blocks` is NULL (no block means) or a host array of P ints: blocks[p] = 0 takes none of part p, blocks[p] >= 1 must
 * divide part_widths[p] and cuts part p's columns into blocks[p] equal blocks; sum_p blocks[p] <=
 * PIGS_MLP_JOINED_MAX_BLOCKS.  With a block wanted,
 *   m [sum_p blocks[p]] (float32), in the order of the parts:  m[j] = mean over the N rows and block j's columns of x^2.
 * `part_widths`, `parts`, `blocks`, `g_parts` are host arrays, read during the call and not kept.
 *
 * pigs_mlp_joined_forward.  Without block means: one launch, no scratch, `m` not touched.  With them: the same launch,
 *   in which every wave also writes one record of column sums of x^2 to `scratch`, and a one-workgroup launch that adds
 *   the records in double in a fixed order, divides by N part_widths[p] / blocks[p] (formed in double) and rounds once.
 * pigs_mlp_joined_backward, the launches of pigs_mlp_backward (one, and a second one when any weight or bias gradient is
 *   wanted).  From g_y [N][w_L] and g_m [sum_p blocks[p]], either of which may be NULL (= zero) but not both, to
 *   g_parts[p] [N][part_widths[p]], g_weights[l] and g_biases[l]; a NULL array or a NULL entry is not written.
 *     g_parts[p][row][k] = dA_0[row][K_p + k] + (g_m[block of k] * 2 / (N part_widths[p] / blocks[p])) x[row][k]
 *   (K_p = part p's first column; the second term only for a part with blocks, and only with g_m).  The factor 2 / (N ..)
 *   is formed in double and rounded once.  Every g_weights / g_biases has the bits of pigs_mlp_backward on the joined
 *   array; without g_m every g_parts[p] has the bits of its columns of pigs_mlp_backward's g_x.  No float atomics.
 * scratch: pigs_mlp_joined_scratch_bytes(N, L, widths, P, blocks, backward) bytes, 4-byte aligned.  backward = 0: the
 *   forward's, min(ceil(N / 16), 2048) records of widths[0] floats with a block wanted, else 0.  backward != 0:
 *   pigs_mlp_scratch_bytes(N, L, widths), needed only with a weight or bias gradient wanted.  0 for N <= 0 or an
 *   unsupported net.  Not read by the caller.
 * Arguments are checked before any HIP call and before any pointer is dereferenced: a dtype other than PIGS_F32, L, P, a
 *   width or a part's width out of range, or more than PIGS_MLP_JOINED_MAX_BLOCKS blocks is PIGS_ERR_UNSUPPORTED; N <= 0,
 *   part widths that do not add up to widths[0], a negative blocks[p] or one that does not divide part_widths[p], a null
 *   required array or entry (widths, part_widths, parts, weights, biases and their entries, y; m with a block wanted; g_y
 *   and g_m both; g_m without a block), a backward with no gradient wanted, or a null, misaligned or short scratch when it
 *   is needed is PIGS_ERR_INVALID.  Nothing allocates, frees, synchronises or waits for another workgroup.
 */
#define PIGS_MLP_JOINED_MAX_PARTS 4
#define PIGS_MLP_JOINED_MAX_BLOCKS 8
size_t pigs_mlp_joined_scratch_bytes(int64_t N, int L, const int* widths, int P, const int* blocks, int backward);
int pigs_mlp_joined_forward(int dtype, int64_t N, int L, const int* widths, int P, const int* part_widths,
                            const void* const* parts, const int* blocks, const void* const* weights,
                            const void* const* biases, void* scratch, size_t scratch_bytes, void* y, void* m, void* stream);
int pigs_mlp_joined_backward(int dtype, int64_t N, int L, const int* widths, int P, const int* part_widths,
                             const void* const* parts, const int* blocks, const void* const* weights,
                             const void* const* biases, const void* g_y, const void* g_m, void* scratch,
                             size_t scratch_bytes, void* const* g_parts, void* const* g_weights, void* const* g_biases,
                             void* stream);

/* ---- The dynamics network's input transform (additive to ABI 10) -------------------------------
 * InputTransform (model_pn.py:51-152) as DynamicsNetwork.forward uses it (:237-249): t_params, the input of
 * input_projection.  d = 2, c = 1..4 channels, p = pde_size = 1..4, float32 only.  Row-major device arrays:
 *   means [N][2], full_covariances [N][4], u [N][c], boundaries [N], sample_u [N][c], sample_ux [N][2c],
 *   sample_uxx [N][2c], sample_pde [N][p];
 *   params: a host array of 36 device pointers, net * 6 + (W1, b1, W2, b2, W3, b3); net 0 is latent_net (the Conv1d
 *     weights [out][in][1] read as [out][in]: (7 + 6c + p) -> 16 -> 32 -> 16, tanh after every layer), nets 1..5 are
 *     transform_net, transform_u_net, transform_ux_net, transform_uxx_net, transform_pde_net (16 -> 48 -> 32 -> k^2, tanh
 *     between the layers, k = 2, c, 2c, 2c, p);
 *   latent [16]; matrices [4 + 9 c^2 + p^2]: T [2][2], T_u [c][c], T_ux [2c][2c], T_uxx [2c][2c], T_pde [p][p], each
 *     I + the net's output; t_params [N][5 + 6c + p].
 *
 * pigs_input_transform_matrices_forward, two launches (model_pn.py:104-119): the latent net over the concatenated row
 *   (gathered from the eight arrays, no copy), one record of 16 sums per wave of live rows (at most 2 048 waves); then
 *   one workgroup adds the records in a fixed order, divides by N, writes `latent` and runs the five nets.
 * pigs_input_transform_apply_forward, one launch (model_pn.py:121-135, :137-152 and the cat of :241-249, :288-295):
 *   t_params_n = (T Sigma_n, T_u u_n, boundaries_n, T_u sample_u_n, T_ux ux_n, T_uxx uxx_n, T_pde pde_n).  T means_n
 *   is never used by the reference and is not computed.  boundaries may be NULL: zeros (:282).
 * pigs_input_transform_apply_backward, one launch, two with g_matrices: from g_t_params to g_full_covariances [N][4] =
 *   T^T g, g_u [N][c] = T_u^T g and g_matrices = sum_n g_n x_n^T (one record per wave, added in a fixed order).  A
 *   NULL output is not written.
 * pigs_input_transform_matrices_backward, one launch for the nets (recomputed from `latent`; their 30 gradients and
 *   g_latent), and two more when a gradient through the latent net is wanted: g_means, g_full_covariances, g_u (the part
 *   through the mean alone) and the six gradients of the latent net.  g_params is NULL or a host array of 36 device
 *   pointers in the order of params; a NULL entry is not written.
 * scratch: pigs_input_transform_scratch_bytes(N, c, p) bytes, 4-byte aligned; 0 for N < 1 or c, p outside 1..4.  It is
 *   16 floats and min(ceil(N / 16), PIGS_MLP_MAX_RECORDS) records of the latent net's parameter count.  Not read by
 *   the caller.
 * Arguments are checked before any HIP call: a dtype other than PIGS_F32 or c, p outside 1..4 is PIGS_ERR_UNSUPPORTED;
 *   N < 1, a null required array or entry, no gradient wanted, or a null, misaligned or short scratch where one is used
 *   (always but in apply_forward and in apply_backward without g_matrices) is PIGS_ERR_INVALID.  No float atomics: every
 *   output is a pure function of the inputs, bit for bit.  Nothing allocates, frees, synchronises or waits for another
 *   workgroup.
 */
size_t pigs_input_transform_scratch_bytes(int64_t N, int c, int p);
int pigs_input_transform_matrices_forward(int dtype, int64_t N, int c, int p, const void* means,
                                          const void* full_covariances, const void* u, const void* boundaries,
                                          const void* sample_u, const void* sample_ux, const void* sample_uxx,
                                          const void* sample_pde, const void* const* params, void* scratch,
                                          size_t scratch_bytes, void* latent, void* matrices, void* stream);
int pigs_input_transform_matrices_backward(int dtype, int64_t N, int c, int p, const void* means,
                                           const void* full_covariances, const void* u, const void* boundaries,
                                           const void* sample_u, const void* sample_ux, const void* sample_uxx,
                                           const void* sample_pde, const void* const* params, const void* latent,
                                           const void* g_matrices, void* scratch, size_t scratch_bytes, void* g_means,
                                           void* g_full_covariances, void* g_u, void* const* g_params, void* stream);
int pigs_input_transform_apply_forward(int dtype, int64_t N, int c, int p, const void* matrices,
                                       const void* full_covariances, const void* u, const void* boundaries,
                                       const void* sample_u, const void* sample_ux, const void* sample_uxx,
                                       const void* sample_pde, void* t_params, void* stream);
int pigs_input_transform_apply_backward(int dtype, int64_t N, int c, int p, const void* matrices,
                                        const void* full_covariances, const void* u, const void* sample_u,
                                        const void* sample_ux, const void* sample_uxx, const void* sample_pde,
                                        const void* g_t_params, void* scratch, size_t scratch_bytes,
                                        void* g_full_covariances, void* g_u, void* g_matrices, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PIGS_AMD_H */
