// pem_search.h -- the leaf helpers the searches over the prior's quantile cube share (pem_de.hip, pem_nm.hip, pem_powell.hip)
// and the out-of-line prior transform that the samplers of pem_sampler.hip call as well.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "pem_philox.h"

namespace pem {
namespace search {

// pem::transform out of line, one copy with internal linkage per translation unit: inlined, the library exp / normcdfinv bodies
// are repeated at every call site and cost the sampler kernel 438 registers (one wave per SIMD)
static __device__ __attribute__((noinline)) double transform_call(int kind, double a, double b, double u) {
    return transform(kind, a, b, u);
}

// what scipy minimises: g = -f, a NaN f never wins
__device__ __forceinline__ double cost(double f) { return f == f ? -f : INFINITY; }

__device__ __forceinline__ double clip(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }

}  // namespace search
}  // namespace pem
