// What a Gaussian's (scaling, transform) row gives every kernel that needs its covariance: covariances.hip
// (the builder and its backward) and refine.hip (the split's eigenpair).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pigs {

//   h = tanh(t), r = sqrt(s0 s1), k = 1 / (1 - h^2)
// 1 / (1 - h^2) = cosh(t)^2 is evaluated as (1 + e)^2 / (4 e) with e = exp(-2 |t|): no cancellation for large |t|.
template <typename T>
struct CovTerms {
    T s0, s1, h, r, k;     // k = 1 / (1 - h^2)
    __device__ __forceinline__ CovTerms(const T* __restrict__ scaling, const T* __restrict__ transform, int64_t i) {
        s0 = scaling[2 * i];
        s1 = scaling[2 * i + 1];
        const T t = transform[i];
        const T e = exp(T(-2) * fabs(t));
        h = tanh(t);                                       // accurate near 0, where (1 - e) / (1 + e) cancels
        k = (T(1) + e) * (T(1) + e) / (T(4) * e);          // cosh(t)^2: accurate where 1 - h^2 cancels
        r = sqrt(s0 * s1);
    }
};

}  // namespace pigs
