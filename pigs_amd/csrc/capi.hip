// extern "C" entry points declared in include/pigs_amd.h: argument checks + dispatch.
#include <cmath>

#include "launch.h"

using namespace pigs;

namespace pigs {
thread_local hipError_t g_last_hip_error = hipSuccess;
}

static int check_common(int dtype, int d, int c, int mask, int64_t N, int64_t M, const void* means,
                        const void* conics, const void* values, const void* samples) {
    if (dtype != PIGS_F32 && dtype != PIGS_F64) return PIGS_ERR_UNSUPPORTED;
    if (d < 1 || c < 1 || N < 0 || M < 0 || !mask_valid(mask)) return PIGS_ERR_INVALID;
    if (d > 2 || c > 4) return PIGS_ERR_UNSUPPORTED;
    if (N > 0 && (!means || !conics || !values)) return PIGS_ERR_INVALID;
    if (M > 0 && !samples) return PIGS_ERR_INVALID;
    return PIGS_OK;
}

extern "C" {

int pigs_abi_version(void) { return PIGS_ABI_VERSION; }

const char* pigs_last_hip_error(void) { return hipGetErrorString(g_last_hip_error); }

const char* pigs_status_string(int status) {
    switch (status) {
        case PIGS_OK: return "ok";
        case PIGS_ERR_INVALID: return "invalid argument";
        case PIGS_ERR_UNSUPPORTED: return "unsupported d/c/dtype/orders combination";
        case PIGS_ERR_LAUNCH: return "HIP launch error";
        case PIGS_ERR_WORKSPACE: return "workspace too small";
        default: return "unknown status";
    }
}

int pigs_sample_forward(int dtype, int d, int c, int orders_mask, int64_t N, int64_t M, const void* means,
                        const void* conics, const void* values, const void* samples, void* out0, void* out1,
                        void* out2, void* out3, void* stream) {
    int rc = check_common(dtype, d, c, orders_mask, N, M, means, conics, values, samples);
    if (rc != PIGS_OK) return rc;
    void* outs[4] = {out0, out1, out2, out3};
    for (int k = 0; k < 4; ++k)
        if (mask_uses_slot(orders_mask, k) && M > 0 && !outs[k]) return PIGS_ERR_INVALID;
    SampleArgs a{};
    a.dtype = dtype; a.d = d; a.c = c; a.orders_mask = orders_mask; a.N = N; a.M = M;
    a.means = means; a.conics = conics; a.values = values; a.samples = samples;
    for (int k = 0; k < 4; ++k) a.out[k] = mask_uses_slot(orders_mask, k) ? outs[k] : nullptr;
    return dense_dispatch(false, a, (hipStream_t)stream);
}

int pigs_sample_backward(int dtype, int d, int c, int orders_mask, int64_t N, int64_t M, const void* means,
                         const void* conics, const void* values, const void* samples, const void* gout0,
                         const void* gout1, const void* gout2, const void* gout3, void* g_means, void* g_conics,
                         void* g_values, void* stream) {
    int rc = check_common(dtype, d, c, orders_mask, N, M, means, conics, values, samples);
    if (rc != PIGS_OK) return rc;
    const void* gs[4] = {gout0, gout1, gout2, gout3};
    for (int k = 0; k < 4; ++k)
        if (mask_uses_slot(orders_mask, k) && M > 0 && !gs[k]) return PIGS_ERR_INVALID;
    if (N > 0 && (!g_means || !g_conics || !g_values)) return PIGS_ERR_INVALID;
    SampleArgs a{};
    a.dtype = dtype; a.d = d; a.c = c; a.orders_mask = orders_mask; a.N = N; a.M = M;
    a.means = means; a.conics = conics; a.values = values; a.samples = samples;
    for (int k = 0; k < 4; ++k) a.gout[k] = mask_uses_slot(orders_mask, k) ? gs[k] : nullptr;
    a.g_means = g_means; a.g_conics = g_conics; a.g_values = g_values;
    return dense_dispatch(true, a, (hipStream_t)stream);
}

int pigs_build_covariances(int dtype, int64_t N, const void* scaling, const void* transform, void* covariances,
                           void* conics, void* stream) {
    if (N < 0) return PIGS_ERR_INVALID;
    if (N > 0 && (!scaling || !transform || (!covariances && !conics))) return PIGS_ERR_INVALID;
    return covariances_dispatch(false, dtype, N, scaling, transform, nullptr, nullptr, covariances, conics,
                                (hipStream_t)stream);
}

int pigs_build_covariances_backward(int dtype, int64_t N, const void* scaling, const void* transform,
                                    const void* g_covariances, const void* g_conics, void* g_scaling,
                                    void* g_transform, void* stream) {
    if (N < 0) return PIGS_ERR_INVALID;
    if (N > 0 && (!scaling || !transform || !g_scaling || !g_transform)) return PIGS_ERR_INVALID;
    return covariances_dispatch(true, dtype, N, scaling, transform, g_covariances, g_conics, g_scaling, g_transform,
                                (hipStream_t)stream);
}

size_t pigs_samples_workspace_bytes(int64_t M) { return samples_workspace_bytes(M); }
size_t pigs_plan_workspace_bytes(int64_t N, int64_t M, int c) { return plan_workspace_bytes(N, M, c); }
size_t pigs_samples_error_offset(void) { return samples_error_offset(); }
size_t pigs_plan_error_offset(void) { return plan_error_offset(); }
size_t pigs_samples_lattice_offset(void) { return samples_lattice_offset(); }
size_t pigs_plan_strips_offset(void) { return plan_strips_offset(); }

int pigs_plan_layout_info(int64_t N, int64_t M, int c, int64_t info[6]) {
    if (!info) return PIGS_ERR_INVALID;
    return plan_layout_info(N, M, c, info);
}

int pigs_plan_records_info(int64_t N, int64_t M, int c, int64_t info[4]) {
    if (!info) return PIGS_ERR_INVALID;
    return plan_records_info(N, M, c, info);
}

int pigs_samples_layout_info(int64_t M, int64_t info[4]) {
    if (!info) return PIGS_ERR_INVALID;
    return samples_layout_info(M, info);
}

int pigs_samples_build(void* samples_ws, size_t samples_ws_bytes, int64_t M, const void* samples, void* stream) {
    if (M < 0 || !samples) return PIGS_ERR_INVALID;
    return samples_build(samples_ws, samples_ws_bytes, M, samples, (hipStream_t)stream);
}

int pigs_samples_order_hint(int64_t M) { return samples_order_hint(M); }
int pigs_samples_trust_info(int64_t M, int64_t info[4]) {
    if (!info) return PIGS_ERR_INVALID;
    return samples_trust_info(M, info);
}

int pigs_plan_build(void* workspace, size_t workspace_bytes, void* samples_ws, size_t samples_ws_bytes,
                    int flags, int64_t N, int64_t M, int c, float q_max, float q_max_backward, const void* means,
                    const void* conics, const void* values, const void* samples, void* stream) {
    if (N < 0 || M < 0 || c < 1) return PIGS_ERR_INVALID;
    if (!means || !conics || !values || ((flags & PIGS_BUILD_SAMPLES) && !samples)) return PIGS_ERR_INVALID;
    return plan_build(workspace, workspace_bytes, samples_ws, samples_ws_bytes, flags, N, M, c, q_max, q_max_backward, means,
                      conics, values, samples, (hipStream_t)stream);
}

int pigs_plan_forward(void* workspace, size_t workspace_bytes, const void* samples_ws, size_t samples_ws_bytes,
                      int64_t N, int64_t M, int c, float q_max, int orders_mask, void* out0, void* out1, void* out2,
                      void* out3, void* stream) {
    if (!mask_valid(orders_mask)) return PIGS_ERR_INVALID;
    void* outs[4] = {out0, out1, out2, out3};
    for (int k = 0; k < 4; ++k)
        if (mask_uses_slot(orders_mask, k) && !outs[k]) return PIGS_ERR_INVALID;
    SampleArgs a{};
    a.dtype = PIGS_F32; a.d = 2; a.c = c; a.orders_mask = orders_mask; a.N = N; a.M = M;
    for (int k = 0; k < 4; ++k) a.out[k] = outs[k];
    return plan_forward(workspace, workspace_bytes, samples_ws, samples_ws_bytes, q_max, a, (hipStream_t)stream);
}

int pigs_plan_backward(void* workspace, size_t workspace_bytes, const void* samples_ws, size_t samples_ws_bytes,
                       int64_t N, int64_t M, int c, float q_max, int orders_mask, const void* gout0,
                       const void* gout1, const void* gout2, const void* gout3, void* g_means, void* g_conics,
                       void* g_values, void* stream) {
    if (!mask_valid(orders_mask)) return PIGS_ERR_INVALID;
    const void* gs[4] = {gout0, gout1, gout2, gout3};
    for (int k = 0; k < 4; ++k)
        if (mask_uses_slot(orders_mask, k) && !gs[k]) return PIGS_ERR_INVALID;
    if (!g_means || !g_conics || !g_values) return PIGS_ERR_INVALID;
    SampleArgs a{};
    a.dtype = PIGS_F32; a.d = 2; a.c = c; a.orders_mask = orders_mask; a.N = N; a.M = M;
    for (int k = 0; k < 4; ++k) a.gout[k] = gs[k];
    a.g_means = g_means; a.g_conics = g_conics; a.g_values = g_values;
    return plan_backward(workspace, workspace_bytes, samples_ws, samples_ws_bytes, q_max, a, (hipStream_t)stream);
}

// ---- the fused outputs (launch.h MASK_*): dense when plan_ws is null, else through the plan.  An entry point does its
// own null checks, fills a SampleArgs and leaves the rest to fused_launch.
static SampleArgs fused_args(int mask, int dtype, int d, int c, int64_t N, int64_t M, const void* means, const void* conics,
                             const void* values, const void* samples) {
    SampleArgs a{};
    a.dtype = dtype; a.d = d; a.c = c; a.orders_mask = mask; a.N = N; a.M = M;
    a.means = means; a.conics = conics; a.values = values; a.samples = samples;
    return a;
}

static void fused_gradients(SampleArgs& a, const void* gout, void* g_means, void* g_conics, void* g_values) {
    a.gout[0] = gout;
    a.g_means = g_means; a.g_conics = g_conics; a.g_values = g_values;
}

static int fused_launch(bool backward, const SampleArgs& a, void* plan_ws, size_t plan_ws_bytes, const void* samples_ws,
                        size_t samples_ws_bytes, void* stream) {
    if (plan_ws) {
        // the binned kernels: float32 in two dimensions; the coupled residual for two channels only
        if (a.dtype != PIGS_F32 || a.d != 2 || (a.orders_mask == MASK_COUPLED && a.c != 2)) return PIGS_ERR_UNSUPPORTED;
        return backward ? plan_backward(plan_ws, plan_ws_bytes, samples_ws, samples_ws_bytes, 0.f, a, (hipStream_t)stream)
                        : plan_forward(plan_ws, plan_ws_bytes, samples_ws, samples_ws_bytes, 0.f, a, (hipStream_t)stream);
    }
    const int rc = check_common(a.dtype, a.d, a.c, 1, a.N, a.M, a.means, a.conics, a.values, a.samples);
    if (rc != PIGS_OK) return rc;
    return dense_dispatch(backward, a, (hipStream_t)stream);
}

// linear residual (pair_math.h ORDR)
int pigs_residual_forward(int dtype, int d, int c, int64_t N, int64_t M, const void* means, const void* conics,
                          const void* values, const void* samples, const double* coeffs, const void* target, void* out,
                          void* plan_ws, size_t plan_ws_bytes, const void* samples_ws, size_t samples_ws_bytes, void* stream) {
    if (!coeffs || (M > 0 && !out)) return PIGS_ERR_INVALID;
    SampleArgs a = fused_args(MASK_RESIDUAL, dtype, d, c, N, M, means, conics, values, samples);
    for (int k = 0; k < 4; ++k) a.resid[k] = coeffs[k];
    a.target = target;
    a.out[0] = out;
    return fused_launch(false, a, plan_ws, plan_ws_bytes, samples_ws, samples_ws_bytes, stream);
}

int pigs_residual_backward(int dtype, int d, int c, int64_t N, int64_t M, const void* means, const void* conics,
                           const void* values, const void* samples, const double* coeffs, const void* gout, void* g_means,
                           void* g_conics, void* g_values, void* plan_ws, size_t plan_ws_bytes, const void* samples_ws,
                           size_t samples_ws_bytes, void* stream) {
    if (!coeffs || (M > 0 && !gout) || (N > 0 && (!g_means || !g_conics || !g_values))) return PIGS_ERR_INVALID;
    SampleArgs a = fused_args(MASK_RESIDUAL, dtype, d, c, N, M, means, conics, values, samples);
    for (int k = 0; k < 4; ++k) a.resid[k] = coeffs[k];
    fused_gradients(a, gout, g_means, g_conics, g_values);
    return fused_launch(true, a, plan_ws, plan_ws_bytes, samples_ws, samples_ws_bytes, stream);
}

// general residual (pair_math.h ORDG): per-point coefficients and an advection term
static bool terms_advect(const PigsResidualTerms* t) { return t->adv != 0.0 || t->adv_pt != nullptr; }

int pigs_residual_terms_forward(int dtype, int d, int c, int64_t N, int64_t M, const void* means, const void* conics,
                                const void* values, const void* samples, const PigsResidualTerms* terms, const void* target,
                                void* out, void* aux, void* plan_ws, size_t plan_ws_bytes, const void* samples_ws,
                                size_t samples_ws_bytes, void* stream) {
    if (!terms || (M > 0 && !out)) return PIGS_ERR_INVALID;
    SampleArgs a = fused_args(MASK_TERMS, dtype, d, c, N, M, means, conics, values, samples);
    a.terms = terms;
    a.target = target;
    a.out[0] = out;
    a.aux = aux;
    return fused_launch(false, a, plan_ws, plan_ws_bytes, samples_ws, samples_ws_bytes, stream);
}

int pigs_residual_terms_backward(int dtype, int d, int c, int64_t N, int64_t M, const void* means, const void* conics,
                                 const void* values, const void* samples, const PigsResidualTerms* terms, const void* gout,
                                 const void* aux, void* g_means, void* g_conics, void* g_values, void* plan_ws,
                                 size_t plan_ws_bytes, const void* samples_ws, size_t samples_ws_bytes, void* stream) {
    if (!terms || (M > 0 && !gout) || (N > 0 && (!g_means || !g_conics || !g_values))) return PIGS_ERR_INVALID;
    if (terms_advect(terms) && !aux) return PIGS_ERR_INVALID;
    SampleArgs a = fused_args(MASK_TERMS, dtype, d, c, N, M, means, conics, values, samples);
    a.terms = terms;
    a.aux = terms_advect(terms) ? const_cast<void*>(aux) : nullptr;      // without advection nothing of it is needed
    fused_gradients(a, gout, g_means, g_conics, g_values);
    return fused_launch(true, a, plan_ws, plan_ws_bytes, samples_ws, samples_ws_bytes, stream);
}

// coupled residual (pair_math.h ORDC): the channels mixed by two constant matrices under a per-point weight
int pigs_residual_coupled_forward(int dtype, int d, int c, int64_t N, int64_t M, const void* means, const void* conics,
                                  const void* values, const void* samples, const PigsResidualCoupling* coupling,
                                  const void* target, void* out, void* plan_ws, size_t plan_ws_bytes, const void* samples_ws,
                                  size_t samples_ws_bytes, void* stream) {
    if (!coupling || (M > 0 && !out)) return PIGS_ERR_INVALID;
    if (c == 1) return PIGS_ERR_UNSUPPORTED;      // nothing to couple: pigs_residual_* / pigs_residual_terms_*
    SampleArgs a = fused_args(MASK_COUPLED, dtype, d, c, N, M, means, conics, values, samples);
    a.coupling = coupling;
    a.target = target;
    a.out[0] = out;
    return fused_launch(false, a, plan_ws, plan_ws_bytes, samples_ws, samples_ws_bytes, stream);
}

int pigs_residual_coupled_backward(int dtype, int d, int c, int64_t N, int64_t M, const void* means, const void* conics,
                                   const void* values, const void* samples, const PigsResidualCoupling* coupling,
                                   const void* gout, void* g_means, void* g_conics, void* g_values, void* plan_ws,
                                   size_t plan_ws_bytes, const void* samples_ws, size_t samples_ws_bytes, void* stream) {
    if (!coupling || (M > 0 && !gout) || (N > 0 && (!g_means || !g_conics || !g_values))) return PIGS_ERR_INVALID;
    if (c == 1) return PIGS_ERR_UNSUPPORTED;
    SampleArgs a = fused_args(MASK_COUPLED, dtype, d, c, N, M, means, conics, values, samples);
    a.coupling = coupling;
    fused_gradients(a, gout, g_means, g_conics, g_values);
    return fused_launch(true, a, plan_ws, plan_ws_bytes, samples_ws, samples_ws_bytes, stream);
}

// vorticity terms (pair_math.h ORDV): (u_x, u_y, div, w, w_x, w_y, lap w) of a two-channel field, d = 2
int pigs_vorticity_forward(int dtype, int64_t N, int64_t M, const void* means, const void* conics, const void* values,
                           const void* samples, void* out, void* plan_ws, size_t plan_ws_bytes, const void* samples_ws,
                           size_t samples_ws_bytes, void* stream) {
    if (M > 0 && !out) return PIGS_ERR_INVALID;
    SampleArgs a = fused_args(MASK_VORTICITY, dtype, 2, 2, N, M, means, conics, values, samples);
    a.out[0] = out;
    return fused_launch(false, a, plan_ws, plan_ws_bytes, samples_ws, samples_ws_bytes, stream);
}

int pigs_vorticity_backward(int dtype, int64_t N, int64_t M, const void* means, const void* conics, const void* values,
                            const void* samples, const void* gout, void* g_means, void* g_conics, void* g_values,
                            void* plan_ws, size_t plan_ws_bytes, const void* samples_ws, size_t samples_ws_bytes, void* stream) {
    if ((M > 0 && !gout) || (N > 0 && (!g_means || !g_conics || !g_values))) return PIGS_ERR_INVALID;
    SampleArgs a = fused_args(MASK_VORTICITY, dtype, 2, 2, N, M, means, conics, values, samples);
    fused_gradients(a, gout, g_means, g_conics, g_values);
    return fused_launch(true, a, plan_ws, plan_ws_bytes, samples_ws, samples_ws_bytes, stream);
}

// vorticity residual (pair_math.h ORDN): (div_b, the time-blended vorticity equation's residual), d = 2, c = 2
int pigs_vorticity_residual_forward(int dtype, int64_t N, int64_t M, const void* means, const void* conics, const void* values,
                                    const void* samples, const PigsVorticityResidual* params, const void* prev, void* out,
                                    void* aux, void* plan_ws, size_t plan_ws_bytes, const void* samples_ws,
                                    size_t samples_ws_bytes, void* stream) {
    if (!params || (M > 0 && !out)) return PIGS_ERR_INVALID;
    SampleArgs a = fused_args(MASK_VORT_RESIDUAL, dtype, 2, 2, N, M, means, conics, values, samples);
    a.vort = params;
    a.target = prev;
    a.out[0] = out;
    a.aux = aux;
    return fused_launch(false, a, plan_ws, plan_ws_bytes, samples_ws, samples_ws_bytes, stream);
}

int pigs_vorticity_residual_backward(int dtype, int64_t N, int64_t M, const void* means, const void* conics, const void* values,
                                     const void* samples, const PigsVorticityResidual* params, const void* gout, const void* aux,
                                     void* g_means, void* g_conics, void* g_values, void* plan_ws, size_t plan_ws_bytes,
                                     const void* samples_ws, size_t samples_ws_bytes, void* stream) {
    if (!params || (M > 0 && (!gout || !aux)) || (N > 0 && (!g_means || !g_conics || !g_values))) return PIGS_ERR_INVALID;
    SampleArgs a = fused_args(MASK_VORT_RESIDUAL, dtype, 2, 2, N, M, means, conics, values, samples);
    a.vort = params;
    a.aux = const_cast<void*>(aux);
    fused_gradients(a, gout, g_means, g_conics, g_values);
    return fused_launch(true, a, plan_ws, plan_ws_bytes, samples_ws, samples_ws_bytes, stream);
}

// vorticity fit (pair_math.h ORDF): the vorticity residual's two columns and data_weight (w - data), d = 2, c = 2
int pigs_vorticity_fit_forward(int dtype, int64_t N, int64_t M, const void* means, const void* conics, const void* values,
                               const void* samples, const PigsVorticityFit* params, const void* prev, void* out, void* aux,
                               void* plan_ws, size_t plan_ws_bytes, const void* samples_ws, size_t samples_ws_bytes, void* stream) {
    if (!params || !params->data || (M > 0 && !out)) return PIGS_ERR_INVALID;
    SampleArgs a = fused_args(MASK_VORT_FIT, dtype, 2, 2, N, M, means, conics, values, samples);
    a.fit = params;
    a.target = prev;
    a.out[0] = out;
    a.aux = aux;
    return fused_launch(false, a, plan_ws, plan_ws_bytes, samples_ws, samples_ws_bytes, stream);
}

int pigs_vorticity_fit_backward(int dtype, int64_t N, int64_t M, const void* means, const void* conics, const void* values,
                                const void* samples, const PigsVorticityFit* params, const void* gout, const void* aux,
                                void* g_means, void* g_conics, void* g_values, void* plan_ws, size_t plan_ws_bytes,
                                const void* samples_ws, size_t samples_ws_bytes, void* stream) {
    if (!params || (M > 0 && (!gout || !aux)) || (N > 0 && (!g_means || !g_conics || !g_values))) return PIGS_ERR_INVALID;
    SampleArgs a = fused_args(MASK_VORT_FIT, dtype, 2, 2, N, M, means, conics, values, samples);
    a.fit = params;
    a.aux = const_cast<void*>(aux);
    fused_gradients(a, gout, g_means, g_conics, g_values);
    return fused_launch(true, a, plan_ws, plan_ws_bytes, samples_ws, samples_ws_bytes, stream);
}

// network inputs (pair_math.h ORDI, ORDJ): sample_u, sample_ux, sample_uxx, sample_pde of Model.forward; d = 2, forward only
int pigs_network_inputs_forward(int dtype, int d, int c, int64_t N, int64_t M, const void* means, const void* conics,
                                const void* values, const void* samples, const PigsNetworkInputs* params, void* sample_u,
                                void* sample_ux, void* sample_uxx, void* sample_pde, void* plan_ws, size_t plan_ws_bytes,
                                const void* samples_ws, size_t samples_ws_bytes, void* stream) {
    if (!params || (M > 0 && (!sample_u || !sample_ux || !sample_uxx || !sample_pde))) return PIGS_ERR_INVALID;
    if (params->kind < PIGS_NET_ZERO || params->kind > PIGS_NET_NAVIER_STOKES) return PIGS_ERR_INVALID;
    if (d == 1) return PIGS_ERR_UNSUPPORTED;      // the model is two-dimensional
    const bool ns = params->kind == PIGS_NET_NAVIER_STOKES;
    if ((ns || params->kind == PIGS_NET_WAVE) && c >= 1 && c <= 4 && c != 2) return PIGS_ERR_UNSUPPORTED;
    SampleArgs a = fused_args(ns ? MASK_NET_INPUTS_NS : MASK_NET_INPUTS, dtype, d, c, N, M, means, conics, values, samples);
    a.net = params;
    a.out[0] = sample_u; a.out[1] = sample_ux; a.out[2] = sample_uxx; a.out[3] = sample_pde;
    return fused_launch(false, a, plan_ws, plan_ws_bytes, samples_ws, samples_ws_bytes, stream);
}

// ---- periodic domain (ABI 10): the 3 x 3 images of every Gaussian and the fold of their gradients (periodic.hip)
int pigs_periodic_images(int dtype, int c, int64_t N, double lo, double period, double q_cut, const void* means,
                         const void* conics, const void* values, void* img_means, void* img_conics, void* img_values,
                         uint32_t* flag, void* stream) {
    if (dtype != PIGS_F32 && dtype != PIGS_F64) return PIGS_ERR_UNSUPPORTED;
    if (c < 1 || c > 4) return PIGS_ERR_UNSUPPORTED;
    if (N < 0 || !std::isfinite(lo) || !std::isfinite(period) || !(period > 0) || !std::isfinite(lo + period) ||
        !(q_cut > 0) || !std::isfinite(q_cut))
        return PIGS_ERR_INVALID;
    if (N > 0 && (!means || !conics || !values || !img_means || !img_conics || !img_values)) return PIGS_ERR_INVALID;
    return periodic_dispatch(false, dtype, c, N, lo, period, q_cut, means, conics, values, img_means, img_conics,
                             img_values, flag, (hipStream_t)stream);
}

int pigs_periodic_images_backward(int dtype, int c, int64_t N, const void* g_img_means, const void* g_img_conics,
                                  const void* g_img_values, void* g_means, void* g_conics, void* g_values, void* stream) {
    if (dtype != PIGS_F32 && dtype != PIGS_F64) return PIGS_ERR_UNSUPPORTED;
    if (c < 1 || c > 4) return PIGS_ERR_UNSUPPORTED;
    if (N < 0) return PIGS_ERR_INVALID;
    if (N > 0 && (!g_means || !g_conics || !g_values)) return PIGS_ERR_INVALID;
    return periodic_dispatch(true, dtype, c, N, 0.0, 1.0, 1.0, g_img_means, g_img_conics, g_img_values, g_means,
                             g_conics, g_values, nullptr, (hipStream_t)stream);
}

// the periodic entry points: argument checks before any HIP call (a list entry is j | k << 28)
static int periodic_box_ok(int dtype, int64_t N, double lo, double period) {
    if (dtype != PIGS_F32 && dtype != PIGS_F64) return PIGS_ERR_UNSUPPORTED;
    if (!std::isfinite(lo) || !std::isfinite(period) || !(period > 0) || !std::isfinite(lo + period)) return PIGS_ERR_INVALID;
    if (N >= (1LL << 28)) return PIGS_ERR_UNSUPPORTED;
    return PIGS_OK;
}

// THE argument rule of the sampling entry points (pigs_aggregate_*: H = 1, period = 0 or, checked by the entry, > 0)
static int aggregate_sizes_ok(int dtype, int64_t N, int64_t cap, int H, int L, int K, int F, double period) {
    if (dtype != PIGS_F32 && dtype != PIGS_F64) return PIGS_ERR_UNSUPPORTED;
    if (H < 1 || H > PIGS_AGGREGATE_HEADS_MAX) return PIGS_ERR_UNSUPPORTED;
    if (N < 0 || cap < 1 || L < 1 || K < 1 || F < 0) return PIGS_ERR_INVALID;
    if (L > 128 || K > 128 || F > 128 || N > 0x7fffffffLL) return PIGS_ERR_UNSUPPORTED;
    // two components per lane; the forward, too, refuses a shape whose backward could not run: all three kernels' LDS must fit a CU
    if (!aggregate_admitted(dtype, H, L, K, F)) return PIGS_ERR_UNSUPPORTED;
    if (period != 0.0) return periodic_box_ok(dtype, N, 0.0, period);
    return PIGS_OK;
}

size_t pigs_aggregate_lds_bytes(int dtype, int L, int K, int F) {
    if ((dtype != PIGS_F32 && dtype != PIGS_F64) || L < 1 || K < 1 || F < 0 || L > 128 || K > 128 || F > 128) return 0;
    return aggregate_lds_bytes(dtype, 1, L, K, F);
}

int pigs_aggregate_grid_info(int dtype, int64_t N, int64_t info[2]) {
    if (dtype != PIGS_F32 && dtype != PIGS_F64) return PIGS_ERR_UNSUPPORTED;
    if (N < 0 || !info) return PIGS_ERR_INVALID;
    return aggregate_grid_info(dtype, N, info);
}

size_t pigs_aggregate_workspace_bytes(int dtype, int64_t N) {
    if ((dtype != PIGS_F32 && dtype != PIGS_F64) || N < 0) return 0;
    return aggregate_workspace_bytes(dtype, N);
}

static int aggregate_lists_checked(int dtype, int64_t N, int64_t cap, const void* means, const void* conics, double q_max,
                                   double lo, double period, void* workspace, size_t workspace_bytes, int flags,
                                   int32_t* row_counts, int32_t* row_lists, int32_t* col_counts, int32_t* col_lists,
                                   int32_t* overflow, void* stream) {
    if (dtype != PIGS_F32 && dtype != PIGS_F64) return PIGS_ERR_UNSUPPORTED;
    if (N < 0 || cap < 1 || !(q_max > 0)) return PIGS_ERR_INVALID;
    if ((row_lists == nullptr) != (col_lists == nullptr)) return PIGS_ERR_INVALID;
    if (N > 0 && (!means || !conics || !row_counts || !col_counts || (row_lists && !overflow))) return PIGS_ERR_INVALID;
    return aggregate_lists(dtype, N, cap, means, conics, q_max, workspace, workspace_bytes, flags, row_counts, row_lists,
                           col_counts, col_lists, overflow, (hipStream_t)stream, lo, period);
}

int pigs_aggregate_lists(int dtype, int64_t N, int64_t cap, const void* means, const void* conics, double q_max,
                         void* workspace, size_t workspace_bytes, int flags, int32_t* row_counts, int32_t* row_lists,
                         int32_t* col_counts, int32_t* col_lists, int32_t* overflow, void* stream) {
    return aggregate_lists_checked(dtype, N, cap, means, conics, q_max, 0.0, 0.0, workspace, workspace_bytes, flags, row_counts,
                                   row_lists, col_counts, col_lists, overflow, stream);
}

int pigs_aggregate_lists_periodic(int dtype, int64_t N, int64_t cap, const void* means, const void* conics, double q_max,
                                  double lo, double period, void* workspace, size_t workspace_bytes, int flags,
                                  int32_t* row_counts, int32_t* row_lists, int32_t* col_counts, int32_t* col_lists,
                                  int32_t* overflow, void* stream) {
    const int rc = periodic_box_ok(dtype, N, lo, period);
    if (rc != PIGS_OK) return rc;
    return aggregate_lists_checked(dtype, N, cap, means, conics, q_max, lo, period, workspace, workspace_bytes, flags, row_counts,
                                   row_lists, col_counts, col_lists, overflow, stream);
}

// ---- all heads of a layer in one launch; pigs_aggregate_{forward,backward}[_periodic] are H = 1 of it.
// period = 0: plain lists; > 0: the torus's
int pigs_aggregate_heads_forward(int dtype, int64_t N, int64_t cap, int H, int L, int K, int F, double period, const void* means,
                                 const void* conics, const int32_t* row_counts, const int32_t* row_lists, const void* features,
                                 const void* transforms, const void* queries, const void* keys, const void* frequencies,
                                 const void* distance_transforms, void* out, void* lse, void* acc, void* stream) {
    const int rc = aggregate_sizes_ok(dtype, N, cap, H, L, K, F, period);
    if (rc != PIGS_OK) return rc;
    if (N > 0 && (!means || !conics || !row_counts || !row_lists || !features || !transforms || !queries || !keys ||
                  (F > 0 && !frequencies) || !distance_transforms || !out || !lse || !acc))
        return PIGS_ERR_INVALID;
    AggregateArgs a{};
    a.dtype = dtype; a.N = N; a.cap = cap; a.H = H; a.L = L; a.K = K; a.F = F; a.period = period;
    a.means = means; a.conics = conics; a.row_counts = row_counts; a.row_lists = row_lists;
    a.features = features; a.transform = transforms; a.queries = queries; a.keys = keys; a.frequencies = frequencies;
    a.distance_transform = distance_transforms; a.out = out; a.lse = lse; a.acc = acc;
    return aggregate_forward(a, (hipStream_t)stream);
}

int pigs_aggregate_forward(int dtype, int64_t N, int64_t cap, int L, int K, int F, const void* means, const void* conics,
                           const int32_t* row_counts, const int32_t* row_lists, const void* features,
                           const void* transform, const void* queries, const void* keys, const void* frequencies,
                           const void* distance_transform, void* out, void* lse, void* acc, void* stream) {
    return pigs_aggregate_heads_forward(dtype, N, cap, 1, L, K, F, 0.0, means, conics, row_counts, row_lists, features, transform,
                                        queries, keys, frequencies, distance_transform, out, lse, acc, stream);
}

int pigs_aggregate_forward_periodic(int dtype, int64_t N, int64_t cap, int L, int K, int F, double period, const void* means,
                                    const void* conics, const int32_t* row_counts, const int32_t* row_lists,
                                    const void* features, const void* transform, const void* queries, const void* keys,
                                    const void* frequencies, const void* distance_transform, void* out, void* lse, void* acc,
                                    void* stream) {
    const int rc = periodic_box_ok(dtype, N, 0.0, period);
    if (rc != PIGS_OK) return rc;
    return pigs_aggregate_heads_forward(dtype, N, cap, 1, L, K, F, period, means, conics, row_counts, row_lists, features, transform,
                                        queries, keys, frequencies, distance_transform, out, lse, acc, stream);
}

size_t pigs_aggregate_heads_lds_bytes(int dtype, int H, int L, int K, int F) {
    if ((dtype != PIGS_F32 && dtype != PIGS_F64) || L < 1 || K < 1 || F < 0 || L > 128 || K > 128 || F > 128) return 0;
    return aggregate_heads_lds_bytes(dtype, H, L, K, F);         // 0: H or a component count out of range
}

size_t pigs_aggregate_heads_backward_scratch_bytes(int dtype, int64_t N, int H, int L, int F) {
    if ((dtype != PIGS_F32 && dtype != PIGS_F64) || N < 0 || H < 1 || H > PIGS_AGGREGATE_HEADS_MAX || L < 1 || F < 0) return 0;
    return aggregate_backward_scratch_bytes(dtype, N, H, L, F);
}

size_t pigs_aggregate_backward_scratch_bytes(int dtype, int64_t N, int L, int F) {
    return pigs_aggregate_heads_backward_scratch_bytes(dtype, N, 1, L, F);
}

int pigs_aggregate_heads_backward(int dtype, int64_t N, int64_t cap, int H, int L, int K, int F, double period, const void* means,
                                  const void* conics, const int32_t* row_counts, const int32_t* row_lists,
                                  const int32_t* col_counts, const int32_t* col_lists, const void* features,
                                  const void* transforms, const void* queries, const void* keys, const void* frequencies,
                                  const void* distance_transforms, const void* lse, const void* acc, const void* gout,
                                  void* scratch, size_t scratch_bytes, void* g_features, void* g_transforms, void* g_queries,
                                  void* g_keys, void* g_frequencies, void* g_distance_transforms, void* stream) {
    const int rc = aggregate_sizes_ok(dtype, N, cap, H, L, K, F, period);
    if (rc != PIGS_OK) return rc;
    if (N > 0 && (!means || !conics || !row_counts || !row_lists || !col_counts || !col_lists || !features || !transforms ||
                  !queries || !keys || (F > 0 && !frequencies) || !distance_transforms || !lse || !acc || !gout || !scratch ||
                  !g_features || !g_transforms || !g_queries || !g_keys || (F > 0 && !g_frequencies) || !g_distance_transforms))
        return PIGS_ERR_INVALID;
    if (N > 0 && scratch_bytes < aggregate_backward_scratch_bytes(dtype, N, H, L, F)) return PIGS_ERR_WORKSPACE;
    AggregateArgs a{};
    a.dtype = dtype; a.N = N; a.cap = cap; a.H = H; a.L = L; a.K = K; a.F = F; a.period = period;
    a.means = means; a.conics = conics; a.row_counts = row_counts; a.row_lists = row_lists;
    a.col_counts = col_counts; a.col_lists = col_lists;
    a.features = features; a.transform = transforms; a.queries = queries; a.keys = keys; a.frequencies = frequencies;
    a.distance_transform = distance_transforms;
    a.lse = const_cast<void*>(lse); a.acc = const_cast<void*>(acc); a.gout = gout; a.scratch = scratch;
    a.g_features = g_features; a.g_transform = g_transforms; a.g_queries = g_queries; a.g_keys = g_keys;
    a.g_frequencies = g_frequencies; a.g_distance_transform = g_distance_transforms;
    return aggregate_backward(a, (hipStream_t)stream);
}

int pigs_aggregate_backward(int dtype, int64_t N, int64_t cap, int L, int K, int F, const void* means,
                            const void* conics, const int32_t* row_counts, const int32_t* row_lists,
                            const int32_t* col_counts, const int32_t* col_lists, const void* features,
                            const void* transform, const void* queries, const void* keys, const void* frequencies,
                            const void* distance_transform, const void* lse, const void* acc, const void* gout,
                            void* scratch, size_t scratch_bytes, void* g_features, void* g_transform, void* g_queries,
                            void* g_keys, void* g_frequencies, void* g_distance_transform, void* stream) {
    return pigs_aggregate_heads_backward(dtype, N, cap, 1, L, K, F, 0.0, means, conics, row_counts, row_lists, col_counts, col_lists,
                                         features, transform, queries, keys, frequencies, distance_transform, lse, acc, gout, scratch,
                                         scratch_bytes, g_features, g_transform, g_queries, g_keys, g_frequencies,
                                         g_distance_transform, stream);
}

int pigs_aggregate_backward_periodic(int dtype, int64_t N, int64_t cap, int L, int K, int F, double period, const void* means,
                                     const void* conics, const int32_t* row_counts, const int32_t* row_lists,
                                     const int32_t* col_counts, const int32_t* col_lists, const void* features,
                                     const void* transform, const void* queries, const void* keys, const void* frequencies,
                                     const void* distance_transform, const void* lse, const void* acc, const void* gout,
                                     void* scratch, size_t scratch_bytes, void* g_features, void* g_transform,
                                     void* g_queries, void* g_keys, void* g_frequencies, void* g_distance_transform,
                                     void* stream) {
    const int rc = periodic_box_ok(dtype, N, 0.0, period);
    if (rc != PIGS_OK) return rc;
    return pigs_aggregate_heads_backward(dtype, N, cap, 1, L, K, F, period, means, conics, row_counts, row_lists, col_counts, col_lists,
                                         features, transform, queries, keys, frequencies, distance_transform, lse, acc, gout, scratch,
                                         scratch_bytes, g_features, g_transform, g_queries, g_keys, g_frequencies,
                                         g_distance_transform, stream);
}

size_t pigs_refine_workspace_bytes(int64_t N) { return refine_workspace_bytes(N); }

static int refine_sizes_ok(int dtype, int mode, int c, int64_t N, int64_t rows) {
    if (dtype != PIGS_F32 && dtype != PIGS_F64) return PIGS_ERR_UNSUPPORTED;
    if (mode != PIGS_REFINE_SPLIT && mode != PIGS_REFINE_CLONE) return PIGS_ERR_UNSUPPORTED;
    if (N < 0 || rows < 0 || c < 1) return PIGS_ERR_INVALID;
    if (N > REFINE_MAX_N) return PIGS_ERR_UNSUPPORTED;
    return PIGS_OK;
}
static bool refine_misaligned(const void* p, int dtype) {      // a row of two values is one access
    return ((uintptr_t)p & (dtype == PIGS_F64 ? 15u : 7u)) != 0;
}

int pigs_refine_index(int mode, int64_t N, const uint8_t* keep, const uint8_t* split, void* workspace,
                      size_t workspace_bytes, int64_t* kept_pos, int64_t* child_pos, int64_t* counts, void* stream) {
    const int rc = refine_sizes_ok(PIGS_F32, mode, 1, N, 0);
    if (rc != PIGS_OK) return rc;
    if (N == 0) return PIGS_OK;
    if (!workspace || !kept_pos || !child_pos || !counts || ((uintptr_t)workspace & 7u)) return PIGS_ERR_INVALID;
    if (workspace_bytes < refine_workspace_bytes(N)) return PIGS_ERR_WORKSPACE;
    return refine_index(mode, N, keep, split, workspace, kept_pos, child_pos, counts, (hipStream_t)stream);
}

int pigs_refine_apply(int dtype, int mode, int c, int64_t N, int64_t rows, double value_scale, const int64_t* kept_pos,
                      const int64_t* child_pos, const void* means, const void* scaling, const void* transforms,
                      const void* values, void* out_means, void* out_scaling, void* out_transforms, void* out_values,
                      int64_t* source, int32_t* child, void* stream) {
    const int rc = refine_sizes_ok(dtype, mode, c, N, rows);
    if (rc != PIGS_OK) return rc;
    if (N == 0 || rows == 0) return PIGS_OK;
    if (!kept_pos || !child_pos) return PIGS_ERR_INVALID;
    if ((out_means && !means) || (out_scaling && !scaling) || (out_transforms && !transforms) || (out_values && !values))
        return PIGS_ERR_INVALID;
    if (out_means && mode == PIGS_REFINE_SPLIT && (!scaling || !transforms)) return PIGS_ERR_INVALID;
    if (!out_means && !out_scaling && !out_transforms && !out_values && !source && !child) return PIGS_ERR_INVALID;
    if ((out_means && (refine_misaligned(means, dtype) || refine_misaligned(out_means, dtype))) ||
        ((out_scaling || out_means) && refine_misaligned(scaling, dtype)) || refine_misaligned(out_scaling, dtype))
        return PIGS_ERR_INVALID;
    RefineRows r{};
    r.dtype = dtype; r.mode = mode; r.c = c; r.N = N; r.rows = rows; r.value_scale = value_scale;
    r.kept_pos = kept_pos; r.child_pos = child_pos;
    r.in[0] = means; r.in[1] = scaling; r.in[2] = transforms; r.in[3] = values;
    r.out[0] = out_means; r.out[1] = out_scaling; r.out[2] = out_transforms; r.out[3] = out_values;
    r.source = source; r.child = child;
    return refine_rows(false, r, (hipStream_t)stream);
}

int pigs_refine_backward(int dtype, int mode, int c, int64_t N, int64_t rows, double value_scale, const int64_t* kept_pos,
                         const int64_t* child_pos, const void* g_out_means, const void* g_out_scaling,
                         const void* g_out_transforms, const void* g_out_values, void* g_means, void* g_scaling,
                         void* g_transforms, void* g_values, void* stream) {
    const int rc = refine_sizes_ok(dtype, mode, c, N, rows);
    if (rc != PIGS_OK) return rc;
    if (N == 0) return PIGS_OK;
    if (!kept_pos || !child_pos || (!g_means && !g_scaling && !g_transforms && !g_values)) return PIGS_ERR_INVALID;
    RefineRows r{};
    r.dtype = dtype; r.mode = mode; r.c = c; r.N = N; r.rows = rows; r.value_scale = value_scale;
    r.kept_pos = kept_pos; r.child_pos = child_pos;
    r.in[0] = g_out_means; r.in[1] = g_out_scaling; r.in[2] = g_out_transforms; r.in[3] = g_out_values;
    r.out[0] = g_means; r.out[1] = g_scaling; r.out[2] = g_transforms; r.out[3] = g_values;
    return refine_rows(true, r, (hipStream_t)stream);
}

int pigs_criterion_lds_values(void) { return CRITERION_LDS_VALUES; }

size_t pigs_criterion_workspace_bytes(int dtype, int64_t n, int c) { return criterion_workspace_bytes(dtype, n, c); }

// the checks the two criteria share; *one = the variant that runs
static int criterion_sizes_ok(int dtype, int variant, int c, int64_t n, bool* one) {
    if (dtype != PIGS_F32 && dtype != PIGS_F64) return PIGS_ERR_UNSUPPORTED;
    if (variant != PIGS_CRITERION_AUTO && variant != PIGS_CRITERION_ONE_WORKGROUP && variant != PIGS_CRITERION_MANY_WORKGROUPS)
        return PIGS_ERR_UNSUPPORTED;
    if (n < 0 || c < 1) return PIGS_ERR_INVALID;
    if (n > CRITERION_MAX_VALUES / c) return PIGS_ERR_UNSUPPORTED;
    const bool fits = n * c <= CRITERION_LDS_VALUES;
    if (variant == PIGS_CRITERION_ONE_WORKGROUP && !fits) return PIGS_ERR_UNSUPPORTED;
    *one = variant == PIGS_CRITERION_AUTO ? fits : variant == PIGS_CRITERION_ONE_WORKGROUP;
    return PIGS_OK;
}

int pigs_criterion_quantile_mask(int dtype, int variant, int c, int64_t n, double q, const void* sample_u,
                                 const void* prev_sample_u, const void* density, const uint8_t* boundary_mask,
                                 void* workspace, size_t workspace_bytes, void* metric, void* stats, uint8_t* mask,
                                 void* stream) {
    CriterionQuantile a{};
    const int rc = criterion_sizes_ok(dtype, variant, c, n, &a.one_workgroup);
    if (rc != PIGS_OK) return rc;
    if (!(q >= 0.0 && q <= 1.0)) return PIGS_ERR_INVALID;            // NaN fails both compares
    if (n == 0) return PIGS_OK;
    if (!sample_u || !prev_sample_u || !density || !mask) return PIGS_ERR_INVALID;
    if (!a.one_workgroup) {
        if (!workspace || ((uintptr_t)workspace & 7u)) return PIGS_ERR_INVALID;
        if (workspace_bytes < criterion_workspace_bytes(dtype, n, c)) return PIGS_ERR_WORKSPACE;
    }
    a.dtype = dtype; a.c = c; a.n = n; a.q = q;
    a.sample_u = sample_u; a.prev_sample_u = prev_sample_u; a.density = density; a.boundary = boundary_mask;
    a.workspace = workspace; a.metric = metric; a.stats = stats; a.mask = mask;
    return criterion_quantile(a, (hipStream_t)stream);
}

int pigs_criterion_meanstd_mask(int dtype, int variant, int64_t n, double k, const void* score, const uint8_t* keep,
                                void* workspace, size_t workspace_bytes, void* stats, uint8_t* mask, void* stream) {
    CriterionMeanStd a{};
    const int rc = criterion_sizes_ok(dtype, variant, 1, n, &a.one_workgroup);
    if (rc != PIGS_OK) return rc;
    if (k != k) return PIGS_ERR_INVALID;
    if (n == 0) return PIGS_OK;
    if (!score || !mask) return PIGS_ERR_INVALID;
    if (!a.one_workgroup) {
        if (!workspace || ((uintptr_t)workspace & 7u)) return PIGS_ERR_INVALID;
        if (workspace_bytes < criterion_workspace_bytes(dtype, n, 1)) return PIGS_ERR_WORKSPACE;
    }
    a.dtype = dtype; a.n = n; a.k = k; a.score = score; a.keep = keep;
    a.workspace = workspace; a.stats = stats; a.mask = mask;
    return criterion_meanstd(a, (hipStream_t)stream);
}

static int optim_sizes_ok(int dtype, int means_map, int c, int64_t N) {
    if (dtype != PIGS_F32 && dtype != PIGS_F64) return PIGS_ERR_UNSUPPORTED;
    if (means_map != PIGS_OPTIM_MEANS_TANH && means_map != PIGS_OPTIM_MEANS_IDENTITY) return PIGS_ERR_UNSUPPORTED;
    if (c < 1 || c > 4) return PIGS_ERR_UNSUPPORTED;
    if (N <= 0) return PIGS_ERR_INVALID;
    return PIGS_OK;
}

int pigs_optim_materialize(int dtype, int means_map, int64_t N, double scale, const void* raw_means,
                           const void* raw_scaling, const void* transform, void* means, void* covariances, void* conics,
                           void* stream) {
    const int rc = optim_sizes_ok(dtype, means_map, 1, N);
    if (rc != PIGS_OK) return rc;
    if (!raw_means || !raw_scaling || !transform || !means || !covariances || !conics) return PIGS_ERR_INVALID;
    if (refine_misaligned(raw_means, dtype) || refine_misaligned(raw_scaling, dtype) || refine_misaligned(means, dtype))
        return PIGS_ERR_INVALID;
    return optim_materialize(dtype, N, means_map == PIGS_OPTIM_MEANS_TANH, scale, raw_means, raw_scaling, transform, means,
                             covariances, conics, (hipStream_t)stream);
}

// the statistics' arrays: all six, the [N][2] ones aligned to a row when d = 2; device counts only with a device state
static int optim_stats_ok(const PigsGradStats* s, const PigsAdamStep* hyper, int dtype, bool rows_of_two) {
    if (!s->mean_grad || !s->mean_grad_norm || !s->scale_grad || !s->scale_grad_norm || !s->last_mean_grad ||
        !s->last_scale_grad)
        return PIGS_ERR_INVALID;
    if (s->device_counts && !hyper->device_state) return PIGS_ERR_INVALID;
    if (((uintptr_t)s->device_counts & 7u) != 0) return PIGS_ERR_INVALID;
    if (rows_of_two && (refine_misaligned(s->mean_grad, dtype) || refine_misaligned(s->scale_grad, dtype) ||
                        refine_misaligned(s->last_mean_grad, dtype) || refine_misaligned(s->last_scale_grad, dtype)))
        return PIGS_ERR_INVALID;
    return PIGS_OK;
}

static int optim_step_checked(int dtype, int c, int64_t N, const PigsAdamStep* hyper, void* raw_means, void* values,
                              void* raw_scaling, void* transform, void* exp_avg_means, void* exp_avg_values,
                              void* exp_avg_scaling, void* exp_avg_transform, void* exp_avg_sq_means, void* exp_avg_sq_values,
                              void* exp_avg_sq_scaling, void* exp_avg_sq_transform, const void* g_means, const void* g_values,
                              const void* g_covariances, const void* g_conics, void* means, void* covariances, void* conics,
                              const PigsGradStats* stats, void* stream) {
    if (!hyper) return PIGS_ERR_INVALID;
    const int rc = optim_sizes_ok(dtype, hyper->means_map, c, N);
    if (rc != PIGS_OK) return rc;
    OptimStep o{};
    o.dtype = dtype; o.c = c; o.N = N; o.hyper = hyper; o.stats = stats;
    o.params[0] = raw_means; o.params[1] = values; o.params[2] = raw_scaling; o.params[3] = transform;
    o.exp_avg[0] = exp_avg_means; o.exp_avg[1] = exp_avg_values; o.exp_avg[2] = exp_avg_scaling;
    o.exp_avg[3] = exp_avg_transform;
    o.exp_avg_sq[0] = exp_avg_sq_means; o.exp_avg_sq[1] = exp_avg_sq_values; o.exp_avg_sq[2] = exp_avg_sq_scaling;
    o.exp_avg_sq[3] = exp_avg_sq_transform;
    o.grads[0] = g_means; o.grads[1] = g_values; o.grads[2] = g_covariances; o.grads[3] = g_conics;
    o.out[0] = means; o.out[1] = covariances; o.out[2] = conics;
    for (int g = 0; g < 4; ++g)
        if (!o.params[g] || !o.exp_avg[g] || !o.exp_avg_sq[g]) return PIGS_ERR_INVALID;
    if (!means || !covariances || !conics) return PIGS_ERR_INVALID;
    if (!g_means && !g_values && !g_covariances && !g_conics) return PIGS_ERR_INVALID;
    for (int g = 0; g < 4; g += 2)      // the rows of two values: one access each
        if (refine_misaligned(o.params[g], dtype) || refine_misaligned(o.exp_avg[g], dtype) ||
            refine_misaligned(o.exp_avg_sq[g], dtype))
            return PIGS_ERR_INVALID;
    if (refine_misaligned(g_means, dtype) || refine_misaligned(means, dtype)) return PIGS_ERR_INVALID;
    if (stats) {
        const int ok = optim_stats_ok(stats, hyper, dtype, true);
        if (ok != PIGS_OK) return ok;
    }
    return optim_step(o, (hipStream_t)stream);
}

int pigs_optim_step(int dtype, int c, int64_t N, const PigsAdamStep* hyper, void* raw_means, void* values,
                    void* raw_scaling, void* transform, void* exp_avg_means, void* exp_avg_values, void* exp_avg_scaling,
                    void* exp_avg_transform, void* exp_avg_sq_means, void* exp_avg_sq_values, void* exp_avg_sq_scaling,
                    void* exp_avg_sq_transform, const void* g_means, const void* g_values, const void* g_covariances,
                    const void* g_conics, void* means, void* covariances, void* conics, void* stream) {
    return optim_step_checked(dtype, c, N, hyper, raw_means, values, raw_scaling, transform, exp_avg_means, exp_avg_values,
                              exp_avg_scaling, exp_avg_transform, exp_avg_sq_means, exp_avg_sq_values, exp_avg_sq_scaling,
                              exp_avg_sq_transform, g_means, g_values, g_covariances, g_conics, means, covariances, conics,
                              nullptr, stream);
}

int pigs_optim_step_stats(int dtype, int c, int64_t N, const PigsAdamStep* hyper, void* raw_means, void* values,
                          void* raw_scaling, void* transform, void* exp_avg_means, void* exp_avg_values,
                          void* exp_avg_scaling, void* exp_avg_transform, void* exp_avg_sq_means, void* exp_avg_sq_values,
                          void* exp_avg_sq_scaling, void* exp_avg_sq_transform, const void* g_means, const void* g_values,
                          const void* g_covariances, const void* g_conics, void* means, void* covariances, void* conics,
                          const PigsGradStats* stats, void* stream) {
    if (!stats) return PIGS_ERR_INVALID;
    return optim_step_checked(dtype, c, N, hyper, raw_means, values, raw_scaling, transform, exp_avg_means, exp_avg_values,
                              exp_avg_scaling, exp_avg_transform, exp_avg_sq_means, exp_avg_sq_values, exp_avg_sq_scaling,
                              exp_avg_sq_transform, g_means, g_values, g_covariances, g_conics, means, covariances, conics,
                              stats, stream);
}

int pigs_optim1d_materialize(int dtype, int means_map, int64_t N, double scale, const void* raw_means,
                             const void* raw_scaling, void* means, void* covariances, void* conics, void* stream) {
    const int rc = optim_sizes_ok(dtype, means_map, 1, N);
    if (rc != PIGS_OK) return rc;
    if (!raw_means || !raw_scaling || !means || !covariances || !conics) return PIGS_ERR_INVALID;
    return optim1d_materialize(dtype, N, means_map == PIGS_OPTIM_MEANS_TANH, scale, raw_means, raw_scaling, means,
                               covariances, conics, (hipStream_t)stream);
}

int pigs_optim1d_step(int dtype, int c, int64_t N, const PigsAdamStep* hyper, void* raw_means, void* values,
                      void* raw_scaling, void* exp_avg_means, void* exp_avg_values, void* exp_avg_scaling,
                      void* exp_avg_sq_means, void* exp_avg_sq_values, void* exp_avg_sq_scaling, const void* g_means,
                      const void* g_values, const void* g_covariances, const void* g_conics, void* means, void* covariances,
                      void* conics, const PigsGradStats* stats, void* stream) {
    if (!hyper) return PIGS_ERR_INVALID;
    const int rc = optim_sizes_ok(dtype, hyper->means_map, c, N);
    if (rc != PIGS_OK) return rc;
    OptimStep o{};
    o.dtype = dtype; o.c = c; o.N = N; o.hyper = hyper; o.stats = stats;
    o.params[0] = raw_means; o.params[1] = values; o.params[2] = raw_scaling;
    o.exp_avg[0] = exp_avg_means; o.exp_avg[1] = exp_avg_values; o.exp_avg[2] = exp_avg_scaling;
    o.exp_avg_sq[0] = exp_avg_sq_means; o.exp_avg_sq[1] = exp_avg_sq_values; o.exp_avg_sq[2] = exp_avg_sq_scaling;
    o.grads[0] = g_means; o.grads[1] = g_values; o.grads[2] = g_covariances; o.grads[3] = g_conics;
    o.out[0] = means; o.out[1] = covariances; o.out[2] = conics;
    for (int g = 0; g < 3; ++g)
        if (!o.params[g] || !o.exp_avg[g] || !o.exp_avg_sq[g]) return PIGS_ERR_INVALID;
    if (!means || !covariances || !conics) return PIGS_ERR_INVALID;
    if (!g_means && !g_values && !g_covariances && !g_conics) return PIGS_ERR_INVALID;
    if (stats) {
        const int ok = optim_stats_ok(stats, hyper, dtype, false);
        if (ok != PIGS_OK) return ok;
    }
    return optim1d_step(o, (hipStream_t)stream);
}

int pigs_network_adam_state_doubles(int tensors) {
    return tensors >= 1 && tensors <= NETWORK_ADAM_MAX ? network_adam_state_doubles(tensors) : 0;
}

int pigs_network_adam_step(int dtype, const PigsNetworkAdam* block, double* state, void* exp_avg, void* exp_avg_sq,
                           const void* loss, int loss_dtype, void* stream) {
    if (dtype != PIGS_F32 && dtype != PIGS_F64) return PIGS_ERR_UNSUPPORTED;
    if (loss && loss_dtype != PIGS_F32 && loss_dtype != PIGS_F64) return PIGS_ERR_UNSUPPORTED;
    if (!block || block->tensors < 1 || block->tensors > NETWORK_ADAM_MAX) return PIGS_ERR_INVALID;
    const uintptr_t element = dtype == PIGS_F32 ? 3u : 7u;
    int64_t end = 0;                                  // the moments' elements, every segment starting at a multiple of 4
    bool any = false;
    for (int s = 0; s < block->tensors; ++s) {
        if (!block->params[s] || block->counts[s] <= 0) return PIGS_ERR_INVALID;
        if (block->counts[s] > 0x7fffffffLL) return PIGS_ERR_INVALID;
        end = ((end + 3) & ~(int64_t)3) + block->counts[s];
        if (end > 0x7fffffffLL) return PIGS_ERR_INVALID;
        if (((uintptr_t)block->params[s] & element) || ((uintptr_t)block->grads[s] & element)) return PIGS_ERR_INVALID;
        any = any || block->grads[s];
    }
    if (!any) return PIGS_ERR_INVALID;
    if (!state || ((uintptr_t)state & 7u) || ((uintptr_t)block->dev_lr & 7u)) return PIGS_ERR_INVALID;
    if (!exp_avg || !exp_avg_sq || ((uintptr_t)exp_avg & 15u) || ((uintptr_t)exp_avg_sq & 15u)) return PIGS_ERR_INVALID;
    if (loss && ((uintptr_t)loss & (loss_dtype == PIGS_F32 ? 3u : 7u))) return PIGS_ERR_INVALID;
    NetworkAdamStep o{};
    o.dtype = dtype; o.loss_dtype = loss_dtype; o.block = block; o.state = state;
    o.exp_avg = exp_avg; o.exp_avg_sq = exp_avg_sq; o.loss = loss;
    return network_adam_step(o, (hipStream_t)stream);
}

size_t pigs_advance_scratch_bytes(int64_t N) { return advance_scratch_bytes(N); }

static int advance_sizes_ok(int dtype, int c, int64_t N) {
    if (dtype != PIGS_F32 && dtype != PIGS_F64) return PIGS_ERR_UNSUPPORTED;
    if (c < 1 || c > 4) return PIGS_ERR_UNSUPPORTED;
    if (N <= 0) return PIGS_ERR_INVALID;
    return PIGS_OK;
}

int pigs_advance_forward(int dtype, int c, int64_t N, int wrap, double wrap_lo, double wrap_hi, const void* means,
                         const void* u, const void* scaling, const void* transforms, const void* deltas,
                         const uint8_t* boundary_mask, void* scratch, size_t scratch_bytes, void* out_means, void* out_u,
                         void* out_scaling, void* out_transforms, void* covariances, void* conics, void* full_covariances,
                         void* full_conics, void* penalty, void* stream) {
    const int rc = advance_sizes_ok(dtype, c, N);
    if (rc != PIGS_OK) return rc;
    if (wrap && !(wrap_lo < wrap_hi)) return PIGS_ERR_INVALID;            // NaN fails the compare
    AdvanceStep s{};
    s.dtype = dtype; s.c = c; s.N = N; s.wrap = wrap != 0; s.lo = wrap_lo; s.hi = wrap_hi;
    s.in[0] = means; s.in[1] = u; s.in[2] = scaling; s.in[3] = transforms;
    s.deltas = deltas; s.mask = boundary_mask; s.scratch = scratch;
    s.out[0] = out_means; s.out[1] = out_u; s.out[2] = out_scaling; s.out[3] = out_transforms;
    s.out[4] = covariances; s.out[5] = conics; s.out[6] = full_covariances; s.out[7] = full_conics; s.out[8] = penalty;
    for (int k = 0; k < 4; ++k)
        if (!s.in[k]) return PIGS_ERR_INVALID;
    for (int k = 0; k < 9; ++k)
        if (!s.out[k]) return PIGS_ERR_INVALID;
    if (!deltas || !boundary_mask || !scratch || ((uintptr_t)scratch & 7u)) return PIGS_ERR_INVALID;
    if (refine_misaligned(means, dtype) || refine_misaligned(scaling, dtype) || refine_misaligned(out_means, dtype) ||
        refine_misaligned(out_scaling, dtype))
        return PIGS_ERR_INVALID;
    if (scratch_bytes < advance_scratch_bytes(N)) return PIGS_ERR_WORKSPACE;
    return advance_forward(s, (hipStream_t)stream);
}

int pigs_advance_backward(int dtype, int c, int64_t N, const void* out_scaling, const void* out_transforms,
                          const void* deltas, const uint8_t* boundary_mask, const void* scratch, const void* g_out_means,
                          const void* g_out_u, const void* g_out_scaling, const void* g_out_transforms,
                          const void* g_covariances, const void* g_conics, const void* g_full_covariances,
                          const void* g_full_conics, const void* g_penalty, void* g_means, void* g_u, void* g_scaling,
                          void* g_transforms, void* g_deltas, void* stream) {
    const int rc = advance_sizes_ok(dtype, c, N);
    if (rc != PIGS_OK) return rc;
    AdvanceStep s{};
    s.dtype = dtype; s.c = c; s.N = N;
    s.in[2] = out_scaling; s.in[3] = out_transforms;
    s.deltas = deltas; s.mask = boundary_mask; s.scratch = const_cast<void*>(scratch);
    s.gout[0] = g_out_means; s.gout[1] = g_out_u; s.gout[2] = g_out_scaling; s.gout[3] = g_out_transforms;
    s.gout[4] = g_covariances; s.gout[5] = g_conics; s.gout[6] = g_full_covariances; s.gout[7] = g_full_conics;
    s.gout[8] = g_penalty;
    s.out[0] = g_means; s.out[1] = g_u; s.out[2] = g_scaling; s.out[3] = g_transforms; s.out[4] = g_deltas;
    if (!out_scaling || !out_transforms || !deltas || !boundary_mask) return PIGS_ERR_INVALID;
    if (g_penalty && (!scratch || ((uintptr_t)scratch & 7u))) return PIGS_ERR_INVALID;
    if (!g_means && !g_u && !g_scaling && !g_transforms && !g_deltas) return PIGS_ERR_INVALID;
    if (refine_misaligned(out_scaling, dtype) || refine_misaligned(g_out_means, dtype) ||
        refine_misaligned(g_out_scaling, dtype) || refine_misaligned(g_means, dtype) || refine_misaligned(g_scaling, dtype))
        return PIGS_ERR_INVALID;
    return advance_backward(s, (hipStream_t)stream);
}

size_t pigs_state_loss_scratch_bytes(int64_t N) { return state_loss_scratch_bytes(N); }

static int state_loss_sizes_ok(int dtype, int c, int64_t N, double wall, double drift) {
    const int rc = advance_sizes_ok(dtype, c, N);
    if (rc != PIGS_OK) return rc;
    if (!(wall >= 0.0) || !(wall < 1e300)) return PIGS_ERR_INVALID;            // NaN fails the compare
    if (!(drift * drift > 0.0) || !(drift * drift < 1e300)) return PIGS_ERR_INVALID;
    return PIGS_OK;
}

int pigs_state_loss_forward(int dtype, int c, int64_t N, double wall, double drift, const void* means, const void* u,
                            const void* deltas, const uint8_t* boundary_mask, void* scratch, size_t scratch_bytes,
                            void* terms, void* stream) {
    const int rc = state_loss_sizes_ok(dtype, c, N, wall, drift);
    if (rc != PIGS_OK) return rc;
    if (!means || !u || !deltas || !boundary_mask || !terms) return PIGS_ERR_INVALID;
    if (!scratch || ((uintptr_t)scratch & 7u)) return PIGS_ERR_INVALID;
    if (scratch_bytes < state_loss_scratch_bytes(N)) return PIGS_ERR_WORKSPACE;
    StateLossStep s{};
    s.dtype = dtype; s.c = c; s.N = N; s.wall = wall; s.drift = drift;
    s.means = means; s.u = u; s.deltas = deltas; s.mask = boundary_mask; s.scratch = scratch; s.terms = terms;
    return state_loss_forward(s, (hipStream_t)stream);
}

int pigs_state_loss_backward(int dtype, int c, int64_t N, double wall, double drift, const void* means, const void* u,
                             const void* deltas, const uint8_t* boundary_mask, const void* scratch, const void* g_terms,
                             void* g_means, void* g_u, void* g_deltas, void* stream) {
    const int rc = state_loss_sizes_ok(dtype, c, N, wall, drift);
    if (rc != PIGS_OK) return rc;
    if (!means || !u || !deltas || !boundary_mask || !g_terms) return PIGS_ERR_INVALID;
    if (!scratch || ((uintptr_t)scratch & 7u)) return PIGS_ERR_INVALID;
    if (!g_means && !g_u && !g_deltas) return PIGS_ERR_INVALID;
    StateLossStep s{};
    s.dtype = dtype; s.c = c; s.N = N; s.wall = wall; s.drift = drift;
    s.means = means; s.u = u; s.deltas = deltas; s.mask = boundary_mask; s.scratch = const_cast<void*>(scratch);
    s.g_terms = g_terms; s.g_means = g_means; s.g_u = g_u; s.g_deltas = g_deltas;
    return state_loss_backward(s, (hipStream_t)stream);
}

size_t pigs_mlp_scratch_bytes(int64_t N, int L, const int* widths) { return mlp_scratch_bytes(N, L, widths); }

static int mlp_sizes_ok(int dtype, int64_t N, int L, const int* widths) {
    if (dtype != PIGS_F32) return PIGS_ERR_UNSUPPORTED;
    if (L < 1 || L > PIGS_MLP_MAX_LAYERS) return PIGS_ERR_UNSUPPORTED;
    if (!widths) return PIGS_ERR_INVALID;
    for (int l = 0; l <= L; ++l)
        if (widths[l] < 1 || widths[l] > PIGS_MLP_MAX_WIDTH) return PIGS_ERR_UNSUPPORTED;
    if (N <= 0) return PIGS_ERR_INVALID;
    return PIGS_OK;
}

static bool mlp_net_missing(int L, const void* x, const void* const* weights, const void* const* biases) {
    if (!x || !weights || !biases) return true;
    for (int l = 0; l < L; ++l)
        if (!weights[l] || !biases[l]) return true;
    return false;
}

int pigs_mlp_forward(int dtype, int64_t N, int L, const int* widths, const void* x, const void* const* weights,
                     const void* const* biases, void* y, void* stream) {
    const int rc = mlp_sizes_ok(dtype, N, L, widths);
    if (rc != PIGS_OK) return rc;
    if (mlp_net_missing(L, x, weights, biases) || !y) return PIGS_ERR_INVALID;
    MlpStep s{};
    s.N = N; s.L = L; s.widths = widths; s.x = x; s.weights = weights; s.biases = biases; s.y = y;
    return mlp_forward(s, (hipStream_t)stream);
}

int pigs_mlp_backward(int dtype, int64_t N, int L, const int* widths, const void* x, const void* const* weights,
                      const void* const* biases, const void* g_y, void* scratch, size_t scratch_bytes, void* g_x,
                      void* const* g_weights, void* const* g_biases, void* stream) {
    const int rc = mlp_sizes_ok(dtype, N, L, widths);
    if (rc != PIGS_OK) return rc;
    if (mlp_net_missing(L, x, weights, biases) || !g_y) return PIGS_ERR_INVALID;
    bool params = false;
    for (int l = 0; l < L; ++l) params = params || (g_weights && g_weights[l]) || (g_biases && g_biases[l]);
    if (!g_x && !params) return PIGS_ERR_INVALID;
    if (params && (!scratch || ((uintptr_t)scratch & 3u) || scratch_bytes < mlp_scratch_bytes(N, L, widths)))
        return PIGS_ERR_INVALID;
    MlpStep s{};
    s.N = N; s.L = L; s.widths = widths; s.x = x; s.weights = weights; s.biases = biases; s.g_y = g_y;
    s.scratch = scratch; s.g_x = g_x; s.g_weights = g_weights; s.g_biases = g_biases;
    return mlp_backward(s, (hipStream_t)stream);
}

size_t pigs_mlp_bank_scratch_bytes(int64_t N, int B, int L, const int* widths) {
    return mlp_bank_scratch_bytes(N, B, L, widths);
}

static int mlp_bank_sizes_ok(int dtype, int64_t N, int B, int G, int L, const int* widths) {
    if (dtype != PIGS_F32) return PIGS_ERR_UNSUPPORTED;
    if (B < 1 || B > PIGS_MLP_BANK_MAX_NETS) return PIGS_ERR_UNSUPPORTED;
    const int rc = mlp_sizes_ok(dtype, N, L, widths);
    if (rc != PIGS_OK) return rc;
    return G < 1 || B % G ? PIGS_ERR_INVALID : PIGS_OK;
}

int pigs_mlp_bank_forward(int dtype, int64_t N, int B, int G, int L, const int* widths, const void* x,
                          const void* const* weights, const void* const* biases, void* y, void* stream) {
    const int rc = mlp_bank_sizes_ok(dtype, N, B, G, L, widths);
    if (rc != PIGS_OK) return rc;
    if (mlp_net_missing(B * L, x, weights, biases) || !y) return PIGS_ERR_INVALID;
    MlpBankStep s{};
    s.N = N; s.B = B; s.G = G; s.L = L; s.widths = widths; s.x = x; s.weights = weights; s.biases = biases; s.y = y;
    return mlp_bank_forward(s, (hipStream_t)stream);
}

int pigs_mlp_bank_backward(int dtype, int64_t N, int B, int G, int L, const int* widths, const void* x,
                           const void* const* weights, const void* const* biases, const void* g_y, void* scratch,
                           size_t scratch_bytes, void* g_x, void* const* g_weights, void* const* g_biases, void* stream) {
    const int rc = mlp_bank_sizes_ok(dtype, N, B, G, L, widths);
    if (rc != PIGS_OK) return rc;
    if (mlp_net_missing(B * L, x, weights, biases) || !g_y) return PIGS_ERR_INVALID;
    bool params = false;
    for (int k = 0; k < B * L; ++k) params = params || (g_weights && g_weights[k]) || (g_biases && g_biases[k]);
    if (!g_x && !params) return PIGS_ERR_INVALID;
    if ((params || (g_x && B > 1)) &&
        (!scratch || ((uintptr_t)scratch & 3u) || scratch_bytes < mlp_bank_scratch_bytes(N, B, L, widths)))
        return PIGS_ERR_INVALID;
    MlpBankStep s{};
    s.N = N; s.B = B; s.G = G; s.L = L; s.widths = widths; s.x = x; s.weights = weights; s.biases = biases; s.g_y = g_y;
    s.scratch = scratch; s.g_x = g_x; s.g_weights = g_weights; s.g_biases = g_biases;
    return mlp_bank_backward(s, (hipStream_t)stream);
}

size_t pigs_mlp_joined_scratch_bytes(int64_t N, int L, const int* widths, int P, const int* blocks, int backward) {
    if (P < 1 || P > PIGS_MLP_JOINED_MAX_PARTS) return 0;
    return mlp_joined_scratch_bytes(N, L, widths, P, blocks, backward);
}

// the sizes of a joined call; *block_count: the sum of blocks
static int mlp_joined_sizes_ok(int dtype, int64_t N, int L, const int* widths, int P, const int* part_widths,
                               const int* blocks, int* block_count) {
    if (dtype != PIGS_F32) return PIGS_ERR_UNSUPPORTED;
    if (P < 1 || P > PIGS_MLP_JOINED_MAX_PARTS) return PIGS_ERR_UNSUPPORTED;
    if (L < 1 || L > PIGS_MLP_MAX_LAYERS) return PIGS_ERR_UNSUPPORTED;
    if (!widths || !part_widths) return PIGS_ERR_INVALID;
    for (int l = 0; l <= L; ++l)
        if (widths[l] < 1 || widths[l] > PIGS_MLP_MAX_WIDTH) return PIGS_ERR_UNSUPPORTED;
    int sum = 0, count = 0;
    for (int p = 0; p < P; ++p) {
        if (part_widths[p] < 1 || part_widths[p] > PIGS_MLP_MAX_WIDTH) return PIGS_ERR_UNSUPPORTED;
        sum += part_widths[p];
    }
    for (int p = 0; blocks && p < P; ++p) {
        if (blocks[p] < 0) return PIGS_ERR_INVALID;
        if (blocks[p] > PIGS_MLP_JOINED_MAX_BLOCKS - count) return PIGS_ERR_UNSUPPORTED;
        count += blocks[p];
    }
    if (N <= 0 || sum != widths[0]) return PIGS_ERR_INVALID;
    for (int p = 0; blocks && p < P; ++p)
        if (blocks[p] && part_widths[p] % blocks[p]) return PIGS_ERR_INVALID;
    *block_count = count;
    return PIGS_OK;
}

static bool mlp_joined_missing(int L, int P, const void* const* parts, const void* const* weights,
                               const void* const* biases) {
    if (!parts) return true;
    for (int p = 0; p < P; ++p)
        if (!parts[p]) return true;
    return mlp_net_missing(L, parts, weights, biases);
}

static bool mlp_scratch_short(const void* scratch, size_t have, size_t need) {
    return need && (!scratch || ((uintptr_t)scratch & 3u) || have < need);
}

int pigs_mlp_joined_forward(int dtype, int64_t N, int L, const int* widths, int P, const int* part_widths,
                            const void* const* parts, const int* blocks, const void* const* weights,
                            const void* const* biases, void* scratch, size_t scratch_bytes, void* y, void* m, void* stream) {
    int count = 0;
    const int rc = mlp_joined_sizes_ok(dtype, N, L, widths, P, part_widths, blocks, &count);
    if (rc != PIGS_OK) return rc;
    if (mlp_joined_missing(L, P, parts, weights, biases) || !y || (count && !m)) return PIGS_ERR_INVALID;
    if (mlp_scratch_short(scratch, scratch_bytes, mlp_joined_scratch_bytes(N, L, widths, P, blocks, 0))) return PIGS_ERR_INVALID;
    MlpJoinedStep s{};
    s.N = N; s.L = L; s.P = P; s.widths = widths; s.part_widths = part_widths; s.parts = parts;
    s.blocks = count ? blocks : nullptr; s.weights = weights; s.biases = biases; s.y = y; s.m = m; s.scratch = scratch;
    return mlp_joined_forward(s, (hipStream_t)stream);
}

int pigs_mlp_joined_backward(int dtype, int64_t N, int L, const int* widths, int P, const int* part_widths,
                             const void* const* parts, const int* blocks, const void* const* weights,
                             const void* const* biases, const void* g_y, const void* g_m, void* scratch,
                             size_t scratch_bytes, void* const* g_parts, void* const* g_weights, void* const* g_biases,
                             void* stream) {
    int count = 0;
    const int rc = mlp_joined_sizes_ok(dtype, N, L, widths, P, part_widths, blocks, &count);
    if (rc != PIGS_OK) return rc;
    if (mlp_joined_missing(L, P, parts, weights, biases)) return PIGS_ERR_INVALID;
    if ((!g_y && !g_m) || (g_m && !count)) return PIGS_ERR_INVALID;
    bool params = false, wanted = false;
    for (int l = 0; l < L; ++l) params = params || (g_weights && g_weights[l]) || (g_biases && g_biases[l]);
    for (int p = 0; p < P; ++p) wanted = wanted || (g_parts && g_parts[p]);
    if (!wanted && !params) return PIGS_ERR_INVALID;
    if (params && mlp_scratch_short(scratch, scratch_bytes, mlp_joined_scratch_bytes(N, L, widths, P, blocks, 1)))
        return PIGS_ERR_INVALID;
    MlpJoinedStep s{};
    s.N = N; s.L = L; s.P = P; s.widths = widths; s.part_widths = part_widths; s.parts = parts;
    s.blocks = count ? blocks : nullptr; s.weights = weights; s.biases = biases; s.g_y = g_y; s.g_m = g_m;
    s.scratch = scratch; s.g_parts = g_parts; s.g_weights = g_weights; s.g_biases = g_biases;
    return mlp_joined_backward(s, (hipStream_t)stream);
}

}  // extern "C"
