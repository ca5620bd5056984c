// Adam's update of one element, shared by optim.hip (the d = 1 kernels) and network_adam.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace pigs {

// Adam as torch.optim.Adam defines it, with its multiply-adds written out.  `a` holds the launch's constants in T:
// b1, omb1 = 1 - b1, b2, omb2 = 1 - b2, step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t), eps.
// Kernels that must agree bit for bit (the d = 1 kernels with and without statistics; the 16-byte and the scalar path
// of network_adam_step_kernel) call this: under -ffp-contract=fast which of the two products of  b1 m + (1 - b1) g  the
// compiler contracts is its choice per instantiation (in double it differed between two kernels); with explicit fma
// there is no choice left.
template <typename T, typename A>
__device__ __forceinline__ T adam_update_fma(const A& a, T p, T g, T& m, T& v) {
    m = fma(a.b1, m, a.omb1 * g);
    v = fma(a.b2, v, (a.omb2 * g) * g);
    return fma(-a.step_size, m / (sqrt(v) / a.bc2_sqrt + a.eps), p);
}

}  // namespace pigs
