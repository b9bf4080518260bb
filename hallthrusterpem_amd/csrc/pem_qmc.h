// pem_qmc.h -- one point of the shifted Sobol' sequence, shared by the stand-alone sampler (pem_qmc.hip) and the fused Saltelli
// launch (pem_saltelli.hip).  Point (i, d) = XOR over the set bits j of gray(i) = i ^ (i >> 1) of PEM_SOBOL_V[d][j], XORed with
// a 30-bit shift s_d when the design is randomised; the uniform is the cell midpoint (x + 0.5) 2^-30 -- exact in fp64, never 0
// or 1.  There is no running state: any index can be formed on its own (tests/qmc_np.py restates it).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pem_philox.h"
#include "pem_sobol_seq.h"

namespace pem {

constexpr uint32_t QMC_SHIFT_COUNTER = 0x534F424Cu;   // "SOBL": counter word 2 of the shift's Philox block; the Monte-Carlo and
                                                      // Latin-hypercube blocks carry a dimension (pair) < 32 there
constexpr uint64_t QMC_MAX_POINTS = 1ull << PEM_SOBOL_BITS;

// the random digital shift of sequence dimension d: one Philox word keyed by (seed, stream, d); 0 without randomisation
inline uint32_t qmc_shift(uint64_t seed, uint32_t stream, int scramble, int d) {
    if (!scramble) return 0u;
    return philox4x32_10((uint32_t)d, 0u, QMC_SHIFT_COUNTER, stream, (uint32_t)seed, (uint32_t)(seed >> 32)).x >> (32 - PEM_SOBOL_BITS);
}

// Point (g, d) for a wave whose 64 lanes hold the 64 consecutive indices of one 64-aligned group: bits 6.. of gray(g) are then the
// same in every lane -- `gray_wave` is gray(g & ~63) -- and the 24 direction numbers they switch are folded ONCE PER WAVE, lane d
// doing it for sequence dimension d (qmc_wave_part; there are at most 32 dimensions and 64 lanes).  A lane then reads dimension d's
// fold with a readlane and adds the six direction numbers of its own low bits (qmc_lane_part).
// Every lane whose `sd` is a dimension in use must be active here, whether or not it has a sample of its own.
__device__ __forceinline__ uint32_t qmc_wave_part(uint32_t gray_wave, int sd) {
    uint32_t hi = 0u;
#pragma unroll 4     // (24 loads in flight at once cost the fp32 Saltelli launch its fourth wave per SIMD)
    for (int j = 6; j < PEM_SOBOL_BITS; ++j) hi ^= (0u - ((gray_wave >> j) & 1u)) & PEM_SOBOL_V[sd][j];
    return hi;
}
// d: wave-uniform (the six words come through the constant cache)
__device__ __forceinline__ uint32_t qmc_lane_part(uint32_t gray_lane, int d) {
    uint32_t lo = 0u;
#pragma unroll
    for (int j = 0; j < 6; ++j) lo ^= (0u - ((gray_lane >> j) & 1u)) & PEM_SOBOL_V[d][j];
    return lo;
}

__device__ __forceinline__ double qmc_uniform(uint32_t x) { return ((double)x + 0.5) * 0x1.0p-30; }

}  // namespace pem
