// One per-Gaussian tanh network (model_pn.py:154-174 delta_net, :187-198 input_projection, :203-226 the query / key
// transforms; nn.Tanh at :425-426) in ONE launch forward and at most TWO backward, on the f32 MFMA.
//
//   a_0 = x [N][w_0];  a_{l+1} = tanh(a_l W_l^T + b_l) for l < L - 1;  y = a_{L-1} W_{L-1}^T + b_{L-1}
//   W_l [w_{l+1}][w_l] and b_l [w_{l+1}] in nn.Linear's layout, 1 <= L <= 6, every width in 1..48, float32.
//
// The register-resident chain.  A wave owns a tile of 16 rows and computes Y^T = W X^T with v_mfma_f32_16x16x4_f32
// (D[i][j] = sum_k A[i][k] B[k][j]; lane l = 16 g + r supplies A[i = r][k = g] and B[k = g][j = r] and receives
// D[i = 4 g + reg][j = r]):
//   A = W:   lane (r, g) holds W[out = 16 to + r][k]        B = X^T: lane (r, g) holds X[row r][k]
//   D:       lane (r, g) holds Y[row r][out = 16 to + 4 g + reg]
// so the four registers of output tile `t` ARE the B operands of the next layer's k-steps s = 0..3 of input tile t,
// provided the weight operand of that step is read at the same permuted index  k = 16 t + 4 g + s  -- one 16-byte LDS
// read per (out tile, in tile).  Bias (the accumulator's initial value) and tanh are element-wise on the registers:
// nothing moves between lanes and nothing passes through LDS between layers.  x is loaded from memory at that same k.
//
// Widths are padded to multiples of 16 (1..3 tiles); pad weights and biases are zeros in the LDS image and
// tanh(0) = 0 keeps pad features zero.  Rows past N in the last tile are loaded as zeros and never stored.
//
// Backward (recomputes every activation from x; nothing else is saved).  Per tile: the forward sweep leaves a_l, l <
// L, in this wave's LDS region as [row][feature]; then from dZ_{L-1} = g_y downwards
//   dA_l^T = W_l^T dZ_l^T: A = W^T, lane (r, g) holds W[out = 16 to + 4 g + s][in = 16 ti + r] (the same LDS image, read
//            down a column), B = the registers of dZ_l as above, D = dA_l in the layout of a_l;  dZ_{l-1} = dA_l (1 - a_l^2)
//            with a_l read back by the lane that wrote it.  The chain stays in registers here too.
//   dW_l[o][i] = sum_rows dZ_l[row][o] a_l[row][i] contracts over the row, which sits on the lane in both operands: dZ_l
//            goes through LDS once, and A = dZ^T, lane (r, g) holds dZ[row 4 s + g][o = 16 to + r], B lane (r, g) holds
//            a_l[row 4 s + g][i = 16 ti + r], D lane (r, g) holds dW[o = 16 to + 4 g + reg][i = 16 ti + r].
//   db_l   = the column sums of dZ_l: added per lane, the 16 row lanes folded once at the end.
// A wave walks its tiles in a fixed order (tile = wave index, + the number of waves, ...; at most PIGS_MLP_MAX_RECORDS
// waves), accumulates every dW / db in registers and writes ONE record; the finishing launch adds the records in a fixed
// order.  No float atomics: the gradients are a pure function of the inputs.  Masked rows hold g_y = 0, hence dZ = 0 in
// every layer.
//
// The net's description, the staging, the forward helpers (mlp_stage, mlp_layer, mlp_tanh, ...), the backward's layer
// (mlp_backward_layer, mlp_record_layer) and the bodies of the forward and the finishing kernel live in mlp_chain.h:
// input_transform.hip runs the same chain over gathered rows, mlp_bank.hip the same bodies for several nets of one shape
// in one launch.  The backward kernel's body is the text of mlp_backward_body.h, included here, in mlp_chain.h
// (mlp_backward_tiles<T>, for the bank) and in mlp_joined.hip: called as a function it no longer fits this kernel's
// registers.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "mlp_chain.h"

namespace pigs {

// waves of the forward: it writes no records, so its cap only bounds how often the weights are staged (two workgroups
// per CU of 256; measured at N = 65 536, input_projection in a graph replay: 94 us with 256 waves, 31 us with 2 048)
constexpr int MLP_FORWARD_WAVES = 2048;

__global__ __launch_bounds__(64 * MLP_WAVES) void mlp_forward_kernel(int64_t N, int64_t tiles, MlpNet n,
                                                                     const float* __restrict__ x, float* __restrict__ y) {
    extern __shared__ float mlp_lds[];
    mlp_stage(n, mlp_lds);
    mlp_forward_tiles(N, tiles, n, mlp_lds, x, y, n.w[n.L]);
}

__global__ __launch_bounds__(64 * MLP_WAVES) void mlp_backward_kernel(int64_t N, int64_t tiles, MlpNet n, MlpGrads out,
                                                                      const float* __restrict__ x,
                                                                      const float* __restrict__ g_y,
                                                                      float* __restrict__ scratch) {
    extern __shared__ float mlp_lds[];
    mlp_stage(n, mlp_lds);
#define MLP_BODY_T MLP_TILES
#define MLP_BODY_LDS mlp_lds
#define MLP_BODY_LOAD_X(a, row, live, g) mlp_load_rows(a, x, row, live, n.w[0], n.w[0], g)
#define MLP_BODY_LOAD_GY(d, row, live, g) mlp_load_rows(d, g_y, row, live, n.w[n.L], n.w[n.L], g)
#define MLP_BODY_WANT_DA0 out.g_x
#define MLP_BODY_STORE_DA0(d, row, live, g) mlp_store_rows(out.g_x, d, row, live, n.w[0], n.w[0], g)
#define MLP_BODY_RECORDS scratch
#include "mlp_backward_body.h"
#undef MLP_BODY_T
#undef MLP_BODY_LDS
#undef MLP_BODY_LOAD_X
#undef MLP_BODY_LOAD_GY
#undef MLP_BODY_WANT_DA0
#undef MLP_BODY_STORE_DA0
#undef MLP_BODY_RECORDS
}

// the records added in a fixed order into g_W / g_b (mlp_finish_block, mlp_chain.h)
__global__ __launch_bounds__(256) void mlp_finish_kernel(MlpNet n, MlpGrads out, int records,
                                                         const float* __restrict__ scratch) {
    mlp_finish_block(n, out, records, scratch, blockIdx.x);
}

// ---- host ----------------------------------------------------------------------------------------------------
int64_t mlp_records(int64_t N) {
    const int64_t tiles = (N + 15) / 16;
    return tiles < PIGS_MLP_MAX_RECORDS ? tiles : PIGS_MLP_MAX_RECORDS;
}

static bool mlp_widths_ok(int L, const int* widths) {
    if (L < 1 || L > PIGS_MLP_MAX_LAYERS || !widths) return false;
    for (int l = 0; l <= L; ++l)
        if (widths[l] < 1 || widths[l] > PIGS_MLP_MAX_WIDTH) return false;
    return true;
}

int mlp_record_floats(int L, const int* widths) {
    int P = 0;
    for (int l = 0; l < L; ++l) P += widths[l + 1] * (widths[l] + 1);
    return P;
}

size_t mlp_scratch_bytes(int64_t N, int L, const int* widths) {
    if (N <= 0 || !mlp_widths_ok(L, widths)) return 0;
    return (size_t)mlp_records(N) * mlp_record_floats(L, widths) * sizeof(float);
}

static MlpNet mlp_net(const MlpStep& s, int* lds_floats) {
    return mlp_describe(s.L, s.widths, s.weights, s.biases, lds_floats);
}

void mlp_finish_launch(const MlpNet& n, const MlpGrads& out, int records, const float* scratch, hipStream_t stream) {
    hipLaunchKernelGGL(mlp_finish_kernel, dim3((unsigned)((n.P + 63) / 64)), dim3(256), 0, stream, n, out, records, scratch);
}

int mlp_forward(const MlpStep& s, hipStream_t stream) {
    int lds_floats;
    const MlpNet n = mlp_net(s, &lds_floats);
    const int64_t tiles = (s.N + 15) / 16, waves = tiles < MLP_FORWARD_WAVES ? tiles : MLP_FORWARD_WAVES;
    const unsigned groups = (unsigned)((waves + MLP_WAVES - 1) / MLP_WAVES);
    clear_hip_error();
    hipLaunchKernelGGL(mlp_forward_kernel, dim3(groups), dim3(64 * MLP_WAVES), lds_floats * sizeof(float), stream, s.N, tiles,
                       n, (const float*)s.x, (float*)s.y);
    return launch_status();
}

int mlp_backward(const MlpStep& s, hipStream_t stream) {
    int lds_floats;
    const MlpNet n = mlp_net(s, &lds_floats);
    MlpGrads out{};
    out.g_x = (float*)s.g_x;
    bool params = false;
    for (int l = 0; l < s.L; ++l) {
        out.g_W[l] = s.g_weights ? (float*)s.g_weights[l] : nullptr;
        out.g_b[l] = s.g_biases ? (float*)s.g_biases[l] : nullptr;
        params = params || out.g_W[l] || out.g_b[l];
    }
    const int64_t tiles = (s.N + 15) / 16, records = mlp_records(s.N);
    const unsigned groups = (unsigned)((records + MLP_WAVES - 1) / MLP_WAVES);
    const size_t lds = (size_t)(lds_floats + MLP_WAVES * (s.L + 1) * 16 * MLP_ROW) * sizeof(float);
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)mlp_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lds);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            g_last_hip_error = e;
            return PIGS_ERR_LAUNCH;
        }
    }
    clear_hip_error();
    hipLaunchKernelGGL(mlp_backward_kernel, dim3(groups), dim3(64 * MLP_WAVES), lds, stream, s.N, tiles, n, out,
                       (const float*)s.x, (const float*)s.g_y, (float*)s.scratch);
    if (params) mlp_finish_launch(n, out, (int)records, (const float*)s.scratch, stream);
    return launch_status();
}

}  // namespace pigs
