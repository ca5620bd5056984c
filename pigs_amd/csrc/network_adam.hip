// The optimiser of the loop with the network: Adam over up to 128 small tensors in TWO launches, and the loss-weighted
// rate of that loop on the device.
//
// Replaces, per time step of main_pn.py:171-232: torch.optim.Adam(model.parameters()).step() (:59, :222), the rate
// g["lr"] = g["prev_lr"] * loss_weight (:217-218), loss_weight *= exp(-epsilon * current_loss.item()) (:225) and the
// reads of the loss for total_loss (:227) and all_sufficient (:228).  The reference's DynamicsNetwork is 90 trainable
// tensors of some 30 000 elements, most under 1 024: torch's Adam on it is a chain of launches at the launch floor.
//
// The state (doubles on the device): rate_scale, loss_sum, loss_max, loss_count, then per tensor steps[S], pow1[S] =
// beta1^t, pow2[S] = beta2^t, step_size[S], bc2_sqrt[S].  The moments are two flat arrays, tensor s at seg[s], every
// segment padded to a multiple of 4 elements.
//
// 1. network_adam_advance_kernel, one wave, lanes over the tensors: the running products and the step counts of the
//    tensors that have a gradient, and from them the two numbers the update needs, step_size = rate / (1 - pow1) and
//    bc2_sqrt = sqrt(1 - pow2), rate = lr * rate_scale.  Then one lane folds the loss in: rate_scale *= exp(-decay loss),
//    the sum, the maximum, the count.  The step uses the rate from BEFORE the decay (main_pn.py:217-225).
// 2. network_adam_step_kernel, 256 threads over 1 024 elements: a workgroup finds its (tensor, chunk) from a prefix of
//    block counts that travels, with the pointers, in the kernel's arguments (so a captured launch keeps the addresses it
//    was recorded with); a tensor without a gradient has no blocks.  adam_update_fma per element, 16 bytes at a time
//    where the parameter and the gradient allow it.
// Two launches, as optim_advance_kernel in front of optim_step_kernel: the second reads what the first wrote across the
// launch boundary, and nothing waits for another workgroup.
#include <hip/hip_runtime.h>

#include "adam_update.h"
#include "launch.h"

namespace pigs {

constexpr int NET_ADAM_CHUNK = 1024;     // elements per workgroup: 256 threads x 4

struct NetAdvanceBlock {
    double lr, beta1, beta2, decay;
    const double* dev_lr;                // one double or null
    const void* loss;                    // one float / double or null
    uint64_t present[2];                 // bit s: tensor s has a gradient
    int S, loss_f64;
};

__global__ __launch_bounds__(64) void network_adam_advance_kernel(double* state, NetAdvanceBlock k) {
    if (blockIdx.x != 0) return;
    const int lane = threadIdx.x;
    const double rate = (k.dev_lr ? *k.dev_lr : k.lr) * state[0];
    double* steps = state + NETWORK_ADAM_HEAD;
    double* pow1 = steps + k.S;
    double* pow2 = pow1 + k.S;
    double* step_size = pow2 + k.S;
    double* bc2_sqrt = step_size + k.S;
    for (int s = lane; s < k.S; s += 64) {
        if (!(k.present[s >> 6] >> (s & 63) & 1)) continue;
        steps[s] += 1.0;
        const double p1 = pow1[s] * k.beta1, p2 = pow2[s] * k.beta2;
        pow1[s] = p1;
        pow2[s] = p2;
        step_size[s] = rate / (1.0 - p1);
        bc2_sqrt[s] = sqrt(1.0 - p2);
    }
    __syncthreads();                     // every lane holds the rate from before the decay
    if (lane == 0 && k.loss) {
        const double loss = k.loss_f64 ? *(const double*)k.loss : (double)*(const float*)k.loss;
        state[0] *= exp(-k.decay * loss);
        state[1] += loss;
        if (loss > state[2] || loss != loss) state[2] = loss;
        state[3] += 1.0;
    }
}

template <typename T>
struct NetAdamTable {                    // the step kernel's argument block, about 3.1 KB
    T* p[NETWORK_ADAM_MAX];
    const T* g[NETWORK_ADAM_MAX];        // null: absent
    int first_block[NETWORK_ADAM_MAX + 1];       // prefix of the present tensors' chunk counts
    int end[NETWORK_ADAM_MAX];           // where tensor s's moments end; the next segment starts at the next multiple of 4
    const double* state;
    T *m, *v;                            // the flat moments
    double beta1, beta2, eps;
    int S;
};

template <typename T>
struct NetAdamConsts {
    T b1, omb1, b2, omb2, step_size, bc2_sqrt, eps;
};

template <typename T>
struct alignas(16) Quad {                // four elements: one 16-byte access (float) or two (double)
    T x[4];
};

template <typename T>
__global__ __launch_bounds__(256) void network_adam_step_kernel(NetAdamTable<T> k) {
    const int b = blockIdx.x;
    int s = 0, hi = k.S;                 // the last s with first_block[s] <= b: first_block[S], the grid, is > b
    while (hi - s > 1) {
        const int mid = (s + hi) >> 1;
        if (k.first_block[mid] > b) hi = mid; else s = mid;
    }
    const int seg = s ? (k.end[s - 1] + 3) & ~3 : 0;
    const int64_t n = k.end[s] - seg;
    const int64_t i0 = (int64_t)(b - k.first_block[s]) * NET_ADAM_CHUNK + 4 * threadIdx.x;
    if (i0 >= n) return;
    const double* per_tensor = k.state + NETWORK_ADAM_HEAD + 3 * k.S;
    const NetAdamConsts<T> a{T(k.beta1), T(1.0 - k.beta1), T(k.beta2), T(1.0 - k.beta2),
                             T(per_tensor[s]), T(per_tensor[k.S + s]), T(k.eps)};
    T* p = k.p[s];
    const T* g = k.g[s];
    T* m = k.m + seg;
    T* v = k.v + seg;
    const bool wide = (((uintptr_t)p | (uintptr_t)g) & 15) == 0;      // the segments of m and v always are
    if (wide && i0 + 4 <= n) {
        Quad<T> qp = *reinterpret_cast<const Quad<T>*>(p + i0);
        const Quad<T> qg = *reinterpret_cast<const Quad<T>*>(g + i0);
        Quad<T> qm = *reinterpret_cast<const Quad<T>*>(m + i0);
        Quad<T> qv = *reinterpret_cast<const Quad<T>*>(v + i0);
#pragma unroll
        for (int j = 0; j < 4; ++j) qp.x[j] = adam_update_fma(a, qp.x[j], qg.x[j], qm.x[j], qv.x[j]);
        *reinterpret_cast<Quad<T>*>(p + i0) = qp;
        *reinterpret_cast<Quad<T>*>(m + i0) = qm;
        *reinterpret_cast<Quad<T>*>(v + i0) = qv;
    } else {
        const int64_t i1 = i0 + 4 < n ? i0 + 4 : n;
        for (int64_t i = i0; i < i1; ++i) {
            T mi = m[i], vi = v[i];
            p[i] = adam_update_fma(a, p[i], g[i], mi, vi);
            m[i] = mi;
            v[i] = vi;
        }
    }
}

template <typename T>
static int launch_network_adam(const NetworkAdamStep& o, hipStream_t stream) {
    const PigsNetworkAdam& h = *o.block;
    NetAdamTable<T> t;
    NetAdvanceBlock adv{};
    int64_t seg = 0, blocks = 0;
    for (int s = 0; s < NETWORK_ADAM_MAX; ++s) {
        const bool in = s < h.tensors;
        t.p[s] = in ? (T*)h.params[s] : nullptr;
        t.g[s] = in ? (const T*)h.grads[s] : nullptr;
        t.first_block[s] = (int)blocks;
        if (in) {
            seg = ((seg + 3) & ~(int64_t)3) + h.counts[s];
            if (h.grads[s]) {
                blocks += (h.counts[s] + NET_ADAM_CHUNK - 1) / NET_ADAM_CHUNK;
                adv.present[s >> 6] |= (uint64_t)1 << (s & 63);
            }
        }
        t.end[s] = (int)seg;
    }
    t.first_block[NETWORK_ADAM_MAX] = (int)blocks;
    t.state = o.state;
    t.m = (T*)o.exp_avg;
    t.v = (T*)o.exp_avg_sq;
    t.beta1 = h.beta1; t.beta2 = h.beta2; t.eps = h.eps;
    t.S = h.tensors;
    adv.lr = h.lr; adv.beta1 = h.beta1; adv.beta2 = h.beta2; adv.decay = h.decay;
    adv.dev_lr = h.dev_lr;
    adv.loss = o.loss;
    adv.S = h.tensors;
    adv.loss_f64 = o.loss_dtype == PIGS_F64;
    clear_hip_error();
    hipLaunchKernelGGL(network_adam_advance_kernel, dim3(1), dim3(64), 0, stream, o.state, adv);
    hipLaunchKernelGGL(network_adam_step_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, stream, t);
    return launch_status();
}

// the caller (capi.hip) has checked the block: 1 <= S <= 128, counts > 0, the padded total < 2^31, a gradient somewhere
int network_adam_step(const NetworkAdamStep& o, hipStream_t stream) {
    if (o.dtype == PIGS_F32) return launch_network_adam<float>(o, stream);
    if (o.dtype == PIGS_F64) return launch_network_adam<double>(o, stream);
    return PIGS_ERR_UNSUPPORTED;
}

}  // namespace pigs
