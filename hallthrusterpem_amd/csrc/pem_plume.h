// pem_plume.h -- what the translation units of the plume, cathode and thruster kernels share: pem_kernels.hip (one sweep radius,
// plume_r1_kernel), pem_radii.hip (sweep-radius arrays) and pem_stages.hip (the elementwise stages).  Internal to libpem_hip.so.
#pragma once
#include "pem_common.h"
#include "pem_model.h"
#include "pem_qfused.h"

namespace pem {

constexpr int BLOCK = 256;                     // elementwise kernels
constexpr int WAVE = 64;

struct PlumeIO {
    long long n;
    double torr2pa;
    double radius;  // R = 1 fast path
    const double *P_b, *c0, *c1, *c2, *c3, *c4, *c5, *sigma, *I_B0, *T;
    double *j_ion, *div, *Tc;
    uint8_t* invalid;
    float* j_ion_f32;  // mixed mode: the profile is computed in fp64 and stored as fp32
    // fused likelihood mode (JMODE 3): measurement tables [n_cond][n_ang] and the per-sample result
    const int32_t* m_kidx;
    const double *m_wgt, *m_y, *m_inv_std;
    double* loglik;
    int n_cond, n_ang;
    // Where sample g of an input array lives: ptr[(g / 64) * in_tile_stride + g % 64].  64 = plain SoA arrays (every entry
    // point but one); 15 * 64 = the tile-interleaved layout of pem_coupled_tiled_f64_dev, whose 15 "arrays" are the rows of
    // one [tiles][15][64] block (R = 1 fast path only: the other plume kernels index the arrays directly).
    long long in_tile_stride = 64;
    // counting modes (JMODE 4 / 5): brackets in, counts and records out (csrc/pem_qfused.h)
    pem::CountIO q;
};

// the two LDS tables a workgroup of plume_r1_kernel / plume_rfew_kernel shares: simpson[NSIMP][2] | dpoly[32*12]
constexpr int NSIMP = 96;   // >= L*CH for L in {2, 4, 8}: padded with zero weights so the angle loop needs no branch
constexpr int TABLE_DOUBLES = 2 * NSIMP + PEM_NDI * PEM_NDC;

// Order LDS traffic inside ONE wave (after the table load a wave only ever reads LDS it wrote itself): the LDS
// unit executes a wave's DS instructions in issue order, so only the compiler has to be kept from reordering them.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

typedef double f64x2 __attribute__((ext_vector_type(2)));

// 16-byte store of the write-once profile stream.  Non-temporal: measured 227.6 -> 190.7 us per 1.25e6-sample
// launch against plain stores, interleaved A/B (tools/ab_bench.py); the same hint on the small input
// loads or on the per-sample QoI stores is slower and is not used (profiles/mall_probe_r02m.txt).
__device__ __forceinline__ void stream_store(f64x2 v, f64x2* dst) { __builtin_nontemporal_store(v, dst); }

// u_ion grid node c of sim_hallthruster.jl:46-47, z = range(z0, z1, length = ncells), and the denominator of u_ion there:
// one expression for thruster_uion_kernel and the fused multi-QoI mode, so that both see the same node values
__device__ __forceinline__ double uion_z(double z0, double z1, int ncells, int c) {
    return z0 + (z1 - z0) * ((double)c / (double)(ncells - 1));
}
__device__ __forceinline__ double uion_den(double z) { return 1.0 + exp(-100.0 * (z - 0.04)); }

// csrc/pem_radii.hip: pem_plume_f64_dev past its argument checks and its one-radius branch -- two or more sweep radii, or one with a
// j_ion that is not 16-byte aligned
__attribute__((visibility("hidden"))) int launch_plume_radii(size_t n, int n_radii, const double* radii, const PlumeIO& io, hipStream_t st);

}  // namespace pem
