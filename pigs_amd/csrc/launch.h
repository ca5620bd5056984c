// Host-side argument block shared by the launchers behind the C ABI (include/pigs_amd.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pigs_amd.h"
#include "aggregate_choice.h"
#include "instances.h"      // the order masks, covering_mask_of, the compiled instantiations

namespace pigs {

struct SampleArgs {
    int dtype, d, c, orders_mask;
    int64_t N, M;
    const void *means, *conics, *values, *samples;
    void* out[4];          // forward outputs (orders 0..3)
    const void* gout[4];   // backward: incoming gradients
    void *g_means, *g_conics, *g_values;
    // the fused outputs (MASK_* below), the only way their coefficient blocks reach a launcher:
    double resid[4];       // MASK_RESIDUAL: a0, a1x, a1y, aL
    const void* target;    //   and its target [M][c] (or null)
    const PigsResidualTerms* terms;      // MASK_TERMS: coefficients, fields, advect_by
    void* aux;                           //   and aux [M][1+d][c] (the forward writes it, the backward reads it; or null)
    const PigsResidualCoupling* coupling;      // MASK_COUPLED: coefficients, fields, the two matrices
    const PigsVorticityResidual* vort;         // MASK_VORT_RESIDUAL: coefficients, tau field; `target` = prev [M][7] or null,
                                               //   `aux` = [M][4] (the forward writes it, the backward reads it)
    const PigsVorticityFit* fit;               // MASK_VORT_FIT: the same, and the data [M] with its weight
    const PigsNetworkInputs* net;              // MASK_NET_INPUTS, MASK_NET_INPUTS_NS: the right-hand side's kind and constants;
                                               //   the four arrays leave through out[0..3]
};

int dense_dispatch(bool backward, const SampleArgs& a, hipStream_t stream);

// covariances.hip
int covariances_dispatch(bool backward, int dtype, int64_t N, const void* scaling, const void* transform,
                         const void* a, const void* b, void* o0, void* o1, hipStream_t stream);

// refine.hip
constexpr int REFINE_ROWS = PIGS_REFINE_ROWS;                // rows per workgroup of the index kernels
constexpr int REFINE_SCAN_WIDTH = PIGS_REFINE_SCAN_WIDTH;    // block totals per pass of the one-workgroup scan
constexpr int64_t REFINE_MAX_N = 0x7fffffffLL;
struct RefineRows {        // apply: in = inputs, out = outputs; backward: in = incoming gradients, out = gradients
    int dtype, mode, c;
    int64_t N, rows;
    double value_scale;
    const int64_t *kept_pos, *child_pos;
    const void* in[4];     // means, scaling, transforms, values
    void* out[4];
    int64_t* source;       // apply only
    int32_t* child;
};
size_t refine_workspace_bytes(int64_t N);
int refine_index(int mode, int64_t N, const uint8_t* keep, const uint8_t* split, void* workspace, int64_t* kept_pos,
                 int64_t* child_pos, int64_t* counts, hipStream_t stream);
int refine_rows(bool backward, const RefineRows& r, hipStream_t stream);

// criterion.hip
constexpr int CRITERION_LDS_VALUES = PIGS_CRITERION_LDS_VALUES;      // most values the one-workgroup variant takes
constexpr int64_t CRITERION_MAX_VALUES = 1LL << 24;                  // n * c, as torch.quantile
struct CriterionQuantile {
    int dtype, c;
    bool one_workgroup;
    int64_t n;
    double q;
    const void *sample_u, *prev_sample_u, *density;
    const uint8_t* boundary;
    void* workspace;       // many workgroups only
    void *metric, *stats;  // or null
    uint8_t* mask;
};
struct CriterionMeanStd {
    int dtype;
    bool one_workgroup;
    int64_t n;
    double k;
    const void* score;
    const uint8_t* keep;
    void* workspace;       // many workgroups only
    void* stats;           // or null
    uint8_t* mask;
};
size_t criterion_workspace_bytes(int dtype, int64_t n, int c);
int criterion_quantile(const CriterionQuantile& q, hipStream_t stream);
int criterion_meanstd(const CriterionMeanStd& m, hipStream_t stream);

// optim.hip
struct OptimStep {
    int dtype, c;
    int64_t N;
    const PigsAdamStep* hyper;
    void *params[4], *exp_avg[4], *exp_avg_sq[4];      // raw_means, values, raw_scaling, transform
    const void* grads[4];                              // d means, d values, d covariances, d conics (null = none)
    void* out[3];                                      // the next step's means, covariances, conics
    const PigsGradStats* stats;                        // or null: no gradient statistics
};
int optim_materialize(int dtype, int64_t N, bool tanh_map, double scale, const void* raw_means, const void* raw_scaling,
                      const void* transform, void* o_means, void* o_cov, void* o_conic, hipStream_t stream);
int optim_step(const OptimStep& o, hipStream_t stream);
// d = 1: slots 0..2 of the arrays are raw_means, values, raw_scaling; slot 3 is not read
int optim1d_materialize(int dtype, int64_t N, bool tanh_map, double scale, const void* raw_means, const void* raw_scaling,
                        void* o_means, void* o_cov, void* o_conic, hipStream_t stream);
int optim1d_step(const OptimStep& o, hipStream_t stream);

// network_adam.hip
constexpr int NETWORK_ADAM_MAX = PIGS_NETWORK_ADAM_MAX_TENSORS;
constexpr int NETWORK_ADAM_HEAD = 4;                   // rate_scale, loss_sum, loss_max, loss_count in front of the arrays
struct NetworkAdamStep {
    int dtype, loss_dtype;
    const PigsNetworkAdam* block;
    double* state;                                     // [4 + 5 S]
    void *exp_avg, *exp_avg_sq;                        // the flat moments
    const void* loss;                                  // or null
};
inline int network_adam_state_doubles(int tensors) { return NETWORK_ADAM_HEAD + 5 * tensors; }
int network_adam_step(const NetworkAdamStep& o, hipStream_t stream);

// advance.hip
struct AdvanceStep {
    int dtype, c, wrap;
    int64_t N;
    double lo, hi;
    const void* in[4];       // forward: means, u, scaling, transforms; backward: [2], [3] = the forward's scaling', transforms'
    const void* deltas;      // [N][5 + c]
    const uint8_t* mask;
    void* scratch;           // the forward writes it, the backward reads n_free from its record 0
    const void* gout[9];     // backward: incoming gradients in the order of the forward's outputs (null = none)
    void* out[9];            // forward: means', u', scaling', transforms', covariances, conics, the two full forms, penalty;
                             // backward: gradients of means, u, scaling, transforms, deltas (null = not wanted)
};
size_t advance_scratch_bytes(int64_t N);
int advance_forward(const AdvanceStep& s, hipStream_t stream);
int advance_backward(const AdvanceStep& s, hipStream_t stream);

// state_loss.hip
constexpr int64_t STATE_LOSS_ONE_LAUNCH_ROWS = PIGS_STATE_LOSS_ONE_LAUNCH_ROWS;      // up to here one workgroup, one launch
struct StateLossStep {
    int dtype, c;
    int64_t N;
    double wall, drift;
    const void *means, *u, *deltas;      // the NEW state's means [N][2], u [N][c]; deltas [N][5 + c]
    const uint8_t* mask;
    void* scratch;                       // the forward writes it, the backward reads its statistics record
    void* terms;                         // forward: [8]
    const void* g_terms;                 // backward: the incoming gradient [8]
    void *g_means, *g_u, *g_deltas;      // backward: null = not wanted
};
size_t state_loss_scratch_bytes(int64_t N);
int state_loss_forward(const StateLossStep& s, hipStream_t stream);
int state_loss_backward(const StateLossStep& s, hipStream_t stream);

// mlp.hip
struct MlpStep {
    int64_t N;
    int L;
    const int* widths;                  // [L + 1], host
    const void* x;                      // [N][widths[0]]
    const void* const* weights;         // [L] device pointers, host array: W_l [widths[l + 1]][widths[l]]
    const void* const* biases;          // [L]: b_l [widths[l + 1]]
    void* y;                            // forward: [N][widths[L]]
    const void* g_y;                    // backward: the incoming gradient
    void* scratch;                      // backward: the waves' records (only with a weight or bias gradient)
    void* g_x;                          // backward: null = not wanted
    void* const* g_weights;             // backward: null, or [L] with null entries = not wanted
    void* const* g_biases;
};
size_t mlp_scratch_bytes(int64_t N, int L, const int* widths);
int mlp_forward(const MlpStep& s, hipStream_t stream);
int mlp_backward(const MlpStep& s, hipStream_t stream);

// mlp_bank.hip: B nets of one shape over one x; y and g_y are [G][N][B / G][widths[L]]
struct MlpBankStep {
    int64_t N;
    int B, G, L;
    const int* widths;                  // [L + 1], host: the same for every net
    const void* x;                      // [N][widths[0]]
    const void* const* weights;         // [B * L] device pointers, host array, net b's layer l at b * L + l
    const void* const* biases;
    void* y;                            // forward
    const void* g_y;                    // backward: the incoming gradient
    void* scratch;                      // backward: the waves' records of every net, then the nets' parts of g_x
    void* g_x;                          // backward: null = not wanted
    void* const* g_weights;             // backward: null, or [B * L] with null entries = not wanted
    void* const* g_biases;
};
size_t mlp_bank_scratch_bytes(int64_t N, int B, int L, const int* widths);
int mlp_bank_forward(const MlpBankStep& s, hipStream_t stream);
int mlp_bank_backward(const MlpBankStep& s, hipStream_t stream);

// mlp_joined.hip: one net whose input row is P arrays side by side; optionally the block means of squares of the parts
struct MlpJoinedStep {
    int64_t N;
    int L, P;
    const int* widths;                  // [L + 1], host; widths[0] = the sum of part_widths
    const int* part_widths;             // [P], host
    const void* const* parts;           // [P] device pointers, host array: part p [N][part_widths[p]]
    const int* blocks;                  // null = no block means, or [P]: part p's columns in blocks[p] equal blocks
    const void* const* weights;         // [L]
    const void* const* biases;
    void* y;                            // forward: [N][widths[L]]
    void* m;                            // forward: [sum of blocks], with block means only
    const void* g_y;                    // backward: null = zero
    const void* g_m;                    // backward: null = zero
    void* scratch;                      // forward: the waves' column sums; backward: the waves' records
    void* const* g_parts;               // backward: null, or [P] with null entries = not wanted
    void* const* g_weights;
    void* const* g_biases;
};
size_t mlp_joined_scratch_bytes(int64_t N, int L, const int* widths, int P, const int* blocks, int backward);
int mlp_joined_forward(const MlpJoinedStep& s, hipStream_t stream);
int mlp_joined_backward(const MlpJoinedStep& s, hipStream_t stream);

// periodic.hip: images (fold = false; a = means, conics, values; o = image arrays) or the fold of their gradients
// (fold = true; a = image gradients, null = zero; o = gradients)
int periodic_dispatch(bool fold, int dtype, int c, int64_t N, double lo, double period, double q_cut, const void* a0,
                      const void* a1, const void* a2, void* o0, void* o1, void* o2, uint32_t* flag, hipStream_t stream);

// aggregate.hip
struct AggregateArgs {
    int dtype;
    int64_t N, cap;
    int H, L, K, F;                                // H heads (pigs_aggregate_*: 1; [N][1][K] is [N][K])
    double period;                                 // > 0: periodic lists (entries j | k << 28), means wrapped; 0: plain
    const void *means, *conics;
    const int32_t *row_counts, *row_lists, *col_counts, *col_lists;
    // transform [H][L][L], queries / keys [N][H][K], distance_transform [H][L][2E]
    const void *features, *transform, *queries, *keys, *frequencies, *distance_transform;
    void *out, *lse, *acc;                         // forward outputs [N][H][L], [N][H], [N][H][W] (the backward reads lse and acc)
    const void* gout;                              // backward: incoming gradient [N][H][L]
    void* scratch;                                 // backward: dacc [N][H][W], D [N][H], per-row d frequencies [N][F]
    void *g_features, *g_transform, *g_queries, *g_keys, *g_frequencies, *g_distance_transform;
};
size_t aggregate_workspace_bytes(int dtype, int64_t N);
// (the size rules -- AGG_LDS_MAX, aggregate_lds_bytes, aggregate_admitted, ... -- are aggregate_choice.h's inline functions)
int aggregate_lists(int dtype, int64_t N, int64_t cap, const void* means, const void* conics, double q_max, void* workspace,
                    size_t workspace_bytes, int flags, int32_t* row_counts, int32_t* row_lists, int32_t* col_counts,
                    int32_t* col_lists, int32_t* overflow, hipStream_t stream, double lo = 0.0, double period = 0.0);
int aggregate_forward(const AggregateArgs& a, hipStream_t stream);
int aggregate_backward(const AggregateArgs& a, hipStream_t stream);

// plan.hip
size_t samples_workspace_bytes(int64_t M);
size_t plan_workspace_bytes(int64_t N, int64_t M, int c);
int samples_build(void* sws, size_t sws_bytes, int64_t M, const void* samples, hipStream_t stream);
int samples_order_hint(int64_t M);
int samples_trust_info(int64_t M, int64_t* info);
int plan_build(void* ws, size_t ws_bytes, void* sws, size_t sws_bytes, int flags, int64_t N, int64_t M, int c,
               float q_max, float q_max_backward, const void* means, const void* conics, const void* values, const void* samples,
               hipStream_t stream);
// the fused outputs' coefficient blocks travel in `a` (also N, M, c, orders_mask, out / gout and the gradients)
int plan_forward(void* ws, size_t ws_bytes, const void* sws, size_t sws_bytes, float q_max, const SampleArgs& a,
                 hipStream_t stream);
int plan_backward(void* ws, size_t ws_bytes, const void* sws, size_t sws_bytes, float q_max, const SampleArgs& a,
                  hipStream_t stream);
int plan_layout_info(int64_t N, int64_t M, int c, int64_t* info);
int plan_records_info(int64_t N, int64_t M, int c, int64_t* info);
int samples_layout_info(int64_t M, int64_t* info);
// the Gaussian grid alone (aggregate.hip): plan.hip
size_t aggregate_grid_bytes(int64_t N);
void aggregate_grid_levels(int64_t N, int64_t* info);
int aggregate_grid_info(int dtype, int64_t N, int64_t* info);
int aggregate_grid_build(void* ws, size_t ws_bytes, int64_t N, float q_grid, const float* means, const float* conics,
                         hipStream_t stream);
size_t samples_error_offset();
size_t samples_lattice_offset();
size_t plan_strips_offset();
size_t plan_error_offset();

// The HIP "last error" is sticky per thread and the host process (PyTorch) makes its own HIP
// calls: clear it before a launch, read it after.
extern thread_local hipError_t g_last_hip_error;      // capi.hip; reported by pigs_last_hip_error()
inline void clear_hip_error() { (void)hipGetLastError(); }
inline int launch_status() {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return PIGS_OK;
    g_last_hip_error = e;
    return PIGS_ERR_LAUNCH;
}

}  // namespace pigs
