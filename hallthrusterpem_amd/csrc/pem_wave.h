// pem_wave.h -- wave-level fp64 reductions shared by the fused Saltelli launches (pem_saltelli.hip, pem_sobol_sweep.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace pem {

// Sum eight per-lane values over the 64 lanes of a wave, TRANSPOSING on the way: after the three halving steps each
// lane carries one of the eight sums, so the whole reduction costs 4 + 2 + 1 + 3 = 10 additions (and shuffles) instead
// of 8 x 6.  On return lane l holds the wave total of v[4 (l & 1) + 2 ((l >> 1) & 1) + ((l >> 2) & 1)].
__device__ __forceinline__ double wave_sum8(const double (&v)[8], int lane) {
    double w4[4], w2[2], w;
    const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double send = b0 ? v[k] : v[k + 4], keep = b0 ? v[k + 4] : v[k];
        w4[k] = keep + __shfl_xor(send, 1);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double send = b1 ? w4[k] : w4[k + 2], keep = b1 ? w4[k + 2] : w4[k];
        w2[k] = keep + __shfl_xor(send, 2);
    }
    {
        const double send = b2 ? w2[0] : w2[1], keep = b2 ? w2[1] : w2[0];
        w = keep + __shfl_xor(send, 4);
    }
    w += __shfl_xor(w, 8);
    w += __shfl_xor(w, 16);
    w += __shfl_xor(w, 32);
    return w;
}
// which of the eight values lane l ends up with
__device__ __forceinline__ int wave_sum8_slot(int lane) { return 4 * (lane & 1) + 2 * ((lane >> 1) & 1) + ((lane >> 2) & 1); }

}  // namespace pem
