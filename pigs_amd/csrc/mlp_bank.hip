// A bank: B nets of ONE shape over ONE input (model_pn.py:203-226, :259-261: the query_transform / key_transform nets of
// all heads read the same features) in ONE launch forward and at most TWO backward.
//
//   y [G][N][B/G][w_L]:   y[b / (B/G)][row][b % (B/G)][:] = net_b(x[row])        1 <= B <= PIGS_MLP_BANK_MAX_NETS, G | B
//
// so that B = 4, G = 2 with the nets in the order (q0, q1, k0, k1) leaves y[0] = queries [N][H][K] and y[1] = keys
// [N][H][K], the arrays aggregate_neighbors_heads reads, without a stack or a copy.
//
// A workgroup belongs to one net (blockIdx.y): it stages that net's LDS image and runs mlp.hip's register-resident chain
// over its row tiles (blockIdx.x) through the same helpers -- mlp_stage, mlp_forward_tiles, mlp_backward_tiles,
// mlp_finish_block of mlp_chain.h -- so that y of net b has the bits of pigs_mlp_forward on that net, the LDS need is
// that of one net, and every shape mlp.hip takes is taken here for every B.  Only the addresses differ: rows of y and g_y
// lie (B/G) w_L floats apart, offset by group and slot.
//
// Backward.  Launch 1 is mlp.hip's backward per (wave, net): at most PIGS_MLP_MAX_RECORDS waves PER NET walk the row
// tiles, each writes one record of its net's dW / db; net 0 writes its g_x^(0) into g_x itself, net b > 0 its g_x^(b)
// into part b - 1 of the scratch.  Launch 2 adds every net's records in mlp.hip's fixed order (four interleaved partial
// sums, (p0 + p1) + (p2 + p3)) and, in further workgroups of the same launch, forms
//   g_x = (..((g_x^(0) + g_x^(1)) + g_x^(2)) + ..) + g_x^(B-1)
// element by element.  No float atomics, nothing waits for another workgroup: every output is a pure function of the
// inputs.  Launch 2 is left out when there is nothing for it to do (B = 1 with g_x alone).  A net none of whose
// gradients is wanted is not run when g_x is not wanted either: the launches' second grid dimension counts the nets
// that run.
//
// scratch (floats): records [B][min(ceil(N / 16), PIGS_MLP_MAX_RECORDS)][P], P = sum_l w_{l+1} (w_l + 1), then the parts
// [B - 1][N][w_0].
#include <hip/hip_runtime.h>

#include "launch.h"
#include "mlp_chain.h"

namespace pigs {

constexpr int BANK_NETS = PIGS_MLP_BANK_MAX_NETS;
constexpr int BANK_FORWARD_WAVES = 2048;       // per net, as mlp.hip's forward (MLP_FORWARD_WAVES)
constexpr int BANK_SUM_GROUPS = 1024;          // workgroups of 256 that add the g_x parts (a grid-stride loop beyond)

struct MlpBank {
    MlpNet shape;                              // the nets' common description; its W and b are not used
    int slots;                                 // B / G
    int run;                                   // nets in this launch = gridDim.y
    int net_of[BANK_NETS];                     // blockIdx.y -> net
    int64_t group_floats;                      // N * slots * w_L: one group of y
    const float* W[BANK_NETS][PIGS_MLP_MAX_LAYERS];
    const float* b[BANK_NETS][PIGS_MLP_MAX_LAYERS];
};

struct MlpBankGrads {
    MlpGrads net[BANK_NETS];                   // net[b].g_x: where net b's g_x^(b) goes (g_x itself, a part, or null)
};

// where net b's rows begin in y / g_y
__device__ __forceinline__ int64_t bank_offset(const MlpBank& bank, int b) {
    const int group = b / bank.slots;
    return group * bank.group_floats + (int64_t)(b - group * bank.slots) * bank.shape.w[bank.shape.L];
}

__global__ __launch_bounds__(64 * MLP_WAVES) void mlp_bank_forward_kernel(int64_t N, int64_t tiles, MlpBank bank,
                                                                          const float* __restrict__ x,
                                                                          float* __restrict__ y) {
    extern __shared__ float bank_lds[];
    const int b = bank.net_of[blockIdx.y];
    mlp_stage(bank.shape, bank.W[b], bank.b[b], bank_lds);
    mlp_forward_tiles(N, tiles, bank.shape, bank_lds, x, y + bank_offset(bank, b), bank.slots * bank.shape.w[bank.shape.L]);
}

// T: the accumulator tiles per layer side (mlp_backward_tiles).  A bank whose widths all fit one tile -- the model's --
// runs the instance with a ninth of the accumulators and a fraction of the code of the general one.
template <int T>
__global__ __launch_bounds__(64 * MLP_WAVES) void mlp_bank_backward_kernel(int64_t N, int64_t tiles, int64_t records,
                                                                           MlpBank bank, MlpBankGrads out,
                                                                           const float* __restrict__ x,
                                                                           const float* __restrict__ g_y,
                                                                           float* __restrict__ scratch) {
    extern __shared__ float bank_lds[];
    const int b = bank.net_of[blockIdx.y];
    mlp_stage(bank.shape, bank.W[b], bank.b[b], bank_lds);
    mlp_backward_tiles<T>(N, tiles, bank.shape, out.net[b], bank_lds, x, g_y + bank_offset(bank, b),
                          bank.slots * bank.shape.w[bank.shape.L], scratch + (int64_t)b * records * bank.shape.P);
}

// blockIdx.x < run * per_net: the records of net net_of[blockIdx.x / per_net], 64 parameters per workgroup; the other
// workgroups: g_x += the parts, in the order of the nets
__global__ __launch_bounds__(256) void mlp_bank_finish_kernel(MlpBank bank, MlpBankGrads out, int records, int per_net,
                                                              int parts, int64_t part_floats,
                                                              const float* __restrict__ scratch,
                                                              const float* __restrict__ part0, float* __restrict__ g_x) {
    const int sum_block = (int)blockIdx.x - bank.run * per_net;
    if (sum_block < 0) {
        const int b = bank.net_of[blockIdx.x / per_net];
        mlp_finish_block(bank.shape, out.net[b], records, scratch + (int64_t)b * records * bank.shape.P,
                         blockIdx.x % per_net);
        return;
    }
    const int64_t stride = (int64_t)(gridDim.x - bank.run * per_net) * 256;
    for (int64_t i = (int64_t)sum_block * 256 + threadIdx.x; i < part_floats; i += stride) {
        float sum = g_x[i];
        for (int p = 0; p < parts; ++p) sum += part0[p * part_floats + i];
        g_x[i] = sum;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------
size_t mlp_bank_scratch_bytes(int64_t N, int B, int L, const int* widths) {
    const size_t records = mlp_scratch_bytes(N, L, widths);      // 0 for N <= 0 or an unsupported net
    if (!records || B < 1 || B > BANK_NETS) return 0;
    return (size_t)B * records + (size_t)(B - 1) * (size_t)N * widths[0] * sizeof(float);
}

static MlpBank bank_describe(const MlpBankStep& s, int* lds_floats) {
    MlpBank bank{};
    bank.shape = mlp_describe(s.L, s.widths, s.weights, s.biases, lds_floats);
    for (int l = 0; l < s.L; ++l) bank.shape.W[l] = bank.shape.b[l] = nullptr;
    bank.slots = s.B / s.G;
    bank.group_floats = s.N * bank.slots * s.widths[s.L];
    for (int b = 0; b < s.B; ++b)
        for (int l = 0; l < s.L; ++l) {
            bank.W[b][l] = (const float*)s.weights[b * s.L + l];
            bank.b[b][l] = (const float*)s.biases[b * s.L + l];
        }
    return bank;
}

int mlp_bank_forward(const MlpBankStep& s, hipStream_t stream) {
    int lds_floats;
    MlpBank bank = bank_describe(s, &lds_floats);
    bank.run = s.B;
    for (int b = 0; b < s.B; ++b) bank.net_of[b] = b;
    const int64_t tiles = (s.N + 15) / 16, waves = tiles < BANK_FORWARD_WAVES ? tiles : BANK_FORWARD_WAVES;
    const unsigned groups = (unsigned)((waves + MLP_WAVES - 1) / MLP_WAVES);
    clear_hip_error();
    hipLaunchKernelGGL(mlp_bank_forward_kernel, dim3(groups, (unsigned)s.B), dim3(64 * MLP_WAVES),
                       lds_floats * sizeof(float), stream, s.N, tiles, bank, (const float*)s.x, (float*)s.y);
    return launch_status();
}

int mlp_bank_backward(const MlpBankStep& s, hipStream_t stream) {
    int lds_floats;
    MlpBank bank = bank_describe(s, &lds_floats);
    const int64_t tiles = (s.N + 15) / 16, records = mlp_records(s.N), part_floats = s.N * s.widths[0];
    float* const scratch = (float*)s.scratch;
    float* const part0 = scratch + s.B * records * bank.shape.P;
    MlpBankGrads out{};
    MlpBank finish = bank;                     // the nets with a record to add
    for (int b = 0; b < s.B; ++b) {
        MlpGrads& o = out.net[b];
        bool params = false;
        for (int l = 0; l < s.L; ++l) {
            o.g_W[l] = s.g_weights ? (float*)s.g_weights[b * s.L + l] : nullptr;
            o.g_b[l] = s.g_biases ? (float*)s.g_biases[b * s.L + l] : nullptr;
            params = params || o.g_W[l] || o.g_b[l];
        }
        if (s.g_x) o.g_x = b == 0 ? (float*)s.g_x : part0 + (b - 1) * part_floats;
        if (params || s.g_x) bank.net_of[bank.run++] = b;
        if (params) finish.net_of[finish.run++] = b;
    }
    const unsigned groups = (unsigned)((records + MLP_WAVES - 1) / MLP_WAVES);
    const size_t lds = (size_t)(lds_floats + MLP_WAVES * (s.L + 1) * 16 * MLP_ROW) * sizeof(float);
    int widest = 0;
    for (int l = 0; l <= s.L; ++l) widest = s.widths[l] > widest ? s.widths[l] : widest;
    const auto kernel = widest <= 16 ? mlp_bank_backward_kernel<1> : mlp_bank_backward_kernel<MLP_TILES>;
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            g_last_hip_error = e;
            return PIGS_ERR_LAUNCH;
        }
    }
    clear_hip_error();
    hipLaunchKernelGGL(kernel, dim3(groups, (unsigned)bank.run), dim3(64 * MLP_WAVES), lds, stream, s.N,
                       tiles, records, bank, out, (const float*)s.x, (const float*)s.g_y, scratch);
    const int parts = s.g_x ? s.B - 1 : 0, per_net = (bank.shape.P + 63) / 64;
    int64_t sum_groups = parts ? (part_floats + 255) / 256 : 0;
    if (sum_groups > BANK_SUM_GROUPS) sum_groups = BANK_SUM_GROUPS;
    if (finish.run || parts)
        hipLaunchKernelGGL(mlp_bank_finish_kernel, dim3((unsigned)(finish.run * per_net + sum_groups)), dim3(256), 0, stream,
                           finish, out, (int)records, per_net, parts, part_floats, (const float*)scratch,
                           (const float*)part0, (float*)s.g_x);
    return launch_status();
}

}  // namespace pigs
