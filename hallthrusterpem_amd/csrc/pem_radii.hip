// pem_radii.hip -- the plume stage over sweep-radius ARRAYS (gfx950): the kernels behind pem_plume_f64_dev for two or more radii, and
// for one radius whose j_ion is not 16-byte aligned.  The one-radius fast path is csrc/pem_kernels.hip (plume_r1_kernel); what the
// two share is csrc/pem_plume.h.  By number of radii R:
//   2 .. 8      plume_rfew_kernel<R>   the R = 1 design generalised: eight samples per wave in flight, radii in registers
//   13 .. 64    plume_rmid_kernel<S, 1> S = 64 / R samples per wave in flight, rows staged in LDS, line-aligned 16-byte stores
//   .. 256      plume_radii_kernel     one wave per sample, the (91, R) block streamed with lane = linear index
//   otherwise   plume_generic_kernel   one lane per sample, strided stores
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "pem_math.h"
#include "pem_plume.h"

namespace {

using namespace pem;
using namespace pem_model;

// ---------------------------------------------------------------------------------------------
// general path: any number of radii, one lane per sample, plain strided stores.  Used for
// sweep_radius arrays (tests/test_plume.py:31 uses 25 radii); not the benchmarked configuration.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void plume_generic_kernel(PlumeIO io, const double* __restrict__ radii, int R) {
    const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= io.n) return;
    const double c0 = io.c0[g], c1 = io.c1[g];
    const PlumeSetup ps = plume_setup(io.P_b[g], c1, io.c2[g], io.c3[g], io.c4[g], io.c5[g], io.torr2pa);
    const double n_neutral = ps.n_neutral, a1 = ps.a1, a2 = ps.a2;
    const double sigma = io.sigma[g], I_B0 = io.I_B0[g];
    const double u1 = 1.0 / (a1 * a1), u2 = 1.0 / (a2 * a2);
    const double A1 = (1.0 - c0) / normaliser(a1, u1, PEM_DPOLY);
    const double A2 = c0 / normaliser(a2, u2, PEM_DPOLY);
    constexpr double H = HALF_PI / 90.0;
    const double s1 = (H * H) * u1, s2 = (H * H) * u2;
    const double r10 = exp(-s1), r20 = exp(-s2), q1 = exp(-2.0 * s1), q2 = exp(-2.0 * s2);
    const bool have_T = io.T != nullptr;
    const double thrust = have_T ? io.T[g] : 0.0;

    int invalid = (a1 <= 0.0) ? 1 : 0;
    // `literal`: the Gaussians by direct exp() instead of the recurrence -- the sample is redone that way when pass 0
    // finds a value below 1e-290 / non-positive or a non-finite amplitude (the deep tail, see exact_chunk above)
    bool literal = false, uncertain = false;
    for (int pass = 0; pass < 2; ++pass) {  // pass 0: integrals + invalid flag; pass 1: profile stores
        for (int r = 0; r < R; ++r) {
            const double rad = radii[r];
            const double decay = exp(-rad * n_neutral * sigma);
            const double j_cex = I_B0 * (1.0 - decay) / (2.0 * PEM_PI * (rad * rad));
            const double base = I_B0 * decay / (rad * rad);
            const double B1 = base * A1, B2 = base * A2;
            if (!__builtin_isfinite(B1) || !__builtin_isfinite(B2)) uncertain = true;
            double e1 = (a1 == 0.0) ? __builtin_nan("") : 1.0, e2 = e1, r1 = r10, r2 = r20, den = 0.0, num = 0.0;
            for (int k = 0; k < NANG; ++k) {
                if (literal) {
                    const double alpha = k == NANG - 1 ? HALF_PI : (double)k * H;
                    const double t1 = alpha / a1, t2 = alpha / a2;
                    e1 = exp(-(t1 * t1));
                    e2 = exp(-(t2 * t2));
                }
                const double f = B1 * e1 + B2 * e2;
                const double ji = f + j_cex;
                if (pass == 0) {
                    invalid |= (ji <= 0.0) ? 1 : 0;
                    if (ji < 1e-290) uncertain = true;
                    den = fma(PEM_SIMPSON_CDEN[k], f, den);
                    num = fma(PEM_SIMPSON_CNUM[k], f, num);
                } else {
                    io.j_ion[((size_t)g * NANG + k) * R + r] = invalid ? 1e-20 : ji;
                }
                e1 *= r1;
                r1 *= q1;
                e2 *= r2;
                r2 *= q2;
            }
            if (pass == 0) {
                double cos_div = num / den;
                if (cos_div == __builtin_inf()) cos_div = __builtin_nan("");
                io.div[(size_t)g * R + r] = acos(cos_div);
                if (have_T) io.Tc[(size_t)g * R + r] = thrust * cos_div;
            }
        }
        if (pass == 0 && uncertain && !literal) {   // redo pass 0 literally; pass 1 then stores the literal values
            literal = true;
            invalid = (a1 <= 0.0) ? 1 : 0;
            pass = -1;
        }
    }
    if (io.invalid) io.invalid[g] = (uint8_t)invalid;
}

// ---------------------------------------------------------------------------------------------
// sweep_radius arrays, 2 <= R <= RADII_MAX: one WAVE per sample.  For a sample the (91, R) block of j_ion is the outer
// product  e1[k] B1[r] + e2[k] B2[r] + j_cex[r]  and is contiguous in memory: the wave computes the two Gaussians once
// (91 direct exp() each -- literally the reference's expression, so its deep tail comes for free), the per-radius
// amplitudes with lane = radius, and then streams the block with lane = linear index, 512 contiguous bytes per store,
// deciding plume.py:105 on the way.  The divergence integrals are linear in the amplitudes: four Simpson sums of the two
// Gaussians per sample, combined per radius.  The lane-per-sample
// kernel above writes the same block with a stride of 91 R doubles between lanes: 251 GB/s at R = 25 against
// this kernel's several TB/s (tools/radii_probe.py).
// ---------------------------------------------------------------------------------------------
constexpr int RADII_MAX = 256;
struct RadiiArg {   // the sweep radii travel in the kernel arguments: no device allocation, no copy to wait for
    double r[RADII_MAX];
};
__global__ __launch_bounds__(BLOCK) void plume_radii_kernel(PlumeIO io, RadiiArg radii_arg, int R, int ts) {
#pragma clang fp contract(off)
    __shared__ double lds_all[BLOCK / WAVE][2 * 96 + 3 * RADII_MAX];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* e1 = lds_all[wave];
    double* e2 = e1 + 96;
    double* B1 = e2 + 96;
    double* B2 = B1 + RADII_MAX;
    double* JC = B2 + RADII_MAX;
    const long long nwaves = (long long)gridDim.x * (BLOCK / WAVE);
    const bool have_T = io.T != nullptr;
    const int step_r = WAVE % R, step_k = WAVE / R;
    // A wave takes `ts` (<= 64) consecutive samples at a time: their parameters are computed once, one lane per sample
    // (coalesced input loads), and handed to the whole wave by shuffles as it walks through the blocks.  The host picks
    // ts = 64 for large batches and smaller tiles when there would otherwise be too few of them to fill the chip.
    const long long ntiles = (io.n + ts - 1) / ts;
    for (long long t = (long long)blockIdx.x * (BLOCK / WAVE) + wave; t < ntiles; t += nwaves) {
    const long long gl = (lane < ts && t * ts + lane < io.n) ? t * ts + lane : io.n - 1;    // idle lanes repeat the last sample
    const double c0_l = io.c0[gl], c1_l = io.c1[gl];
    const PlumeSetup ps_l = plume_setup(io.P_b[gl], c1_l, io.c2[gl], io.c3[gl], io.c4[gl], io.c5[gl], io.torr2pa);
    const double nn_l = ps_l.n_neutral, sigma_l = io.sigma[gl];
    const double IB0_l = io.I_B0[gl];
    const double a1_l = ps_l.a1, a2_l = ps_l.a2;
    const double A1_l = (1.0 - c0_l) / normaliser(a1_l, 1.0 / (a1_l * a1_l), PEM_DPOLY);
    const double A2_l = c0_l / normaliser(a2_l, 1.0 / (a2_l * a2_l), PEM_DPOLY);
    const double thrust_l = have_T ? io.T[gl] : 0.0;
    const int in_tile = (int)(io.n - t * ts < ts ? io.n - t * ts : ts);
    for (int smp = 0; smp < in_tile; ++smp) {
        const long long g = t * ts + smp;
        const double a1 = __shfl(a1_l, smp), a2 = __shfl(a2_l, smp), A1 = __shfl(A1_l, smp), A2 = __shfl(A2_l, smp);
        const double n_neutral = __shfl(nn_l, smp), sigma = __shfl(sigma_l, smp);
        const double I_B0 = __shfl(IB0_l, smp), thrust = __shfl(thrust_l, smp);
        // the two Gaussians of plume.py:99-100 on the 91-point grid, and their four Simpson functionals: the sums of
        // plume.py:117-123 are linear in the amplitudes, den[r] = B1[r] sum_k w_k e1[k] + B2[r] sum_k w_k e2[k]
        double s1d = 0.0, s1n = 0.0, s2d = 0.0, s2n = 0.0;
        for (int k = lane; k < NANG; k += WAVE) {
            const double alpha = k == NANG - 1 ? HALF_PI : (double)k * GRID_H;
            const double t1 = alpha / a1, t2 = alpha / a2;
            const double g1 = exp(-(t1 * t1)), g2 = exp(-(t2 * t2));
            e1[k] = g1;
            e2[k] = g2;
            s1d = __builtin_fma(PEM_SIMPSON_CDEN[k], g1, s1d);
            s1n = __builtin_fma(PEM_SIMPSON_CNUM[k], g1, s1n);
            s2d = __builtin_fma(PEM_SIMPSON_CDEN[k], g2, s2d);
            s2n = __builtin_fma(PEM_SIMPSON_CNUM[k], g2, s2n);
        }
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) {
            s1d += __shfl_xor(s1d, sh);
            s1n += __shfl_xor(s1n, sh);
            s2d += __shfl_xor(s2d, sh);
            s2n += __shfl_xor(s2n, sh);
        }
        // per radius (lane = radius): amplitudes and the divergence angle
        for (int r0 = 0; r0 < R; r0 += WAVE) {
            const int r = r0 + lane;
            if (r < R) {
                const double rad = radii_arg.r[r];
                const double decay = exp(-rad * n_neutral * sigma);
                const double j_cex = I_B0 * (1.0 - decay) / (2.0 * PEM_PI * (rad * rad));
                const double base = I_B0 * decay / (rad * rad);
                const double b1 = base * A1, b2 = base * A2;
                B1[r] = b1;
                B2[r] = b2;
                JC[r] = j_cex;
                double num = b1 * s1n + b2 * s2n, den = b1 * s1d + b2 * s2d;
                if (!(fabs(b1) + fabs(b2) < 1e300) || ((b1 < 0.0) != (b2 < 0.0) && b1 != 0.0 && b2 != 0.0)) {
                    // Sum as the reference does (rare) when the amplitudes are near the overflow threshold (exp(+x) of a
                    // negative density: its f_k = b1 e1[k] + b2 e2[k] overflows where the factored sums do not), or of
                    // opposite sign (c0 outside [0, 1]): the reference cancels angle by angle, the factored form would
                    // cancel two large sums at the end
                    num = 0.0;
                    den = 0.0;
                    for (int k = 0; k < NANG; ++k) {
                        const double f = b1 * e1[k] + b2 * e2[k];
                        den = __builtin_fma(PEM_SIMPSON_CDEN[k], f, den);
                        num = __builtin_fma(PEM_SIMPSON_CNUM[k], f, num);
                    }
                }
                double cos_div = num / den;
                if (cos_div == __builtin_inf()) cos_div = __builtin_nan("");
                io.div[(size_t)g * R + r] = acos(cos_div);
                if (have_T) io.Tc[(size_t)g * R + r] = thrust * cos_div;
            }
        }
        wave_lds_sync();
        // the (91, R) block, contiguous: lane = linear index k R + r; plume.py:105 is decided on the way
        double* dst = io.j_ion + (size_t)g * NANG * R;
        bool bad = a1 <= 0.0;
        {
            int k = lane / R, r = lane - k * R;
            for (int idx = lane; idx < NANG * R; idx += WAVE) {
                const double ji = (B1[r] * e1[k] + B2[r] * e2[k]) + JC[r];
                bad |= ji <= 0.0;
                __builtin_nontemporal_store(ji, dst + idx);
                r += step_r;
                k += step_k;
                if (r >= R) {
                    r -= R;
                    ++k;
                }
            }
        }
        const bool invalid = __ballot(bad) != 0;
        if (invalid)   // plume.py:106: the whole block becomes 1e-20 (rare: a second pass over it)
            for (int idx = lane; idx < NANG * R; idx += WAVE) dst[idx] = 1e-20;
        if (io.invalid && lane == 0) io.invalid[g] = (uint8_t)invalid;
        wave_lds_sync();   // the staged rows are rewritten for the next sample
    }
    }
}

// ---------------------------------------------------------------------------------------------
// sweep_radius arrays, RADII_SMALL < R <= RMID_MAX (tests/test_plume.py:31 uses 25): the recipe of the few-radii kernel below
// applied to the wave-per-sample kernel above -- several samples in flight per wave, the block staged in LDS in final order,
// 16-byte stores of whole contiguous runs.  G = 64 / R samples share a wave (7 at 9 radii ... 1 above 32): lane (grp, r) owns radius
// r of sample grp, keeps its amplitudes in registers and walks the 91 angles; the two Gaussians of a sample (by recurrence from
// three exp per beam and lane, literal exp() where the reference's own has left the normal range) are read from LDS as one
// broadcast 16-byte word per angle.
// What the lane produces -- b1[r] e1[k] + b2[r] e2[k] + j_cex[r], the Simpson sums of plume.py:117-123 taken angle by angle as the
// reference takes them -- goes to an LDS tile laid out as j_ion is, `kc` rows of every sample at a time (8 KB per wave), and
// leaves as runs of kc R contiguous doubles: one leading 8-byte store where a run starts on an odd double (the LDS copy is
// placed with the same parity), then 1 KiB per instruction.  Against the kernel above this halves the LDS reads per value
// (2.5 instead of 5), removes the per-value index arithmetic and never assembles a cache line from 8-byte pieces.
// ---------------------------------------------------------------------------------------------
// A run of `len` doubles from LDS to `dst`, the whole wave on it.  `from` has the 16-byte parity of `dst` (the LDS copy is placed
// so).  Store instructions that cover WHOLE 128-byte lines are what the memory system wants: with every instruction straddling
// a line boundary the same kernels run a quarter slower (block sizes 91 R x 8 bytes: 4.65 TB/s at R = 32, 3.39 at R = 33;
// profiles/radii_mid_r03.txt).  So: the doubles up to the next line boundary as one partial instruction of 8-byte stores, then
// 16 bytes per lane, 1 KiB per instruction, line-aligned; an odd double left at the end goes out alone.
__device__ __forceinline__ void stream_run(const double* from, double* dst, int len, int lane) {
    int head = (int)((0 - (reinterpret_cast<uintptr_t>(dst) >> 3)) & 15);
    head = head < len ? head : len;
    if (lane < head) __builtin_nontemporal_store(from[lane], dst + lane);
    const int body = (len - head) >> 1;
    const f64x2* s2 = reinterpret_cast<const f64x2*>(from + head);
    f64x2* d2 = reinterpret_cast<f64x2*>(dst + head);
    for (int i = lane; i < body; i += WAVE) stream_store(s2[i], &d2[i]);
    if (((len - head) & 1) && lane == 0) __builtin_nontemporal_store(from[len - 1], dst + (len - 1));
}

constexpr int RADII_SMALL = 8;                  // up to here: the recurrence kernel with the radii in registers (plume_rfew_kernel)
constexpr int RMID_MAX = 64;
constexpr int RMID_G_MAX = 5;                   // samples in flight per wave the staged kernel is instantiated for (R >= 11)
// doubles of staged rows per wave: 10 KB -- with the Gaussians' 1.5 KB per sample what three workgroups per CU leave each other.
// (Round 4, profiles/radii_mid_r04.txt: 512 / 768 / 1024 / 1280 doubles give 3.08 / 3.38 / 3.58 / 3.82 TB/s at 17 radii, 3.36 / 3.55 /
// 3.73 / 3.85 at 25; radius counts whose rows are whole lines -- 32, 64 -- do not care.)
#ifndef PEM_RMID_TILE_DOUBLES
#define PEM_RMID_TILE_DOUBLES 1280
#endif
constexpr int RMID_TILE = PEM_RMID_TILE_DOUBLES;
struct RadiiMidArg {
    double r[RMID_MAX];
};
constexpr int RMID_ES = 97;                     // 16-byte words of E per sample: an odd stride, so that the G broadcast reads of an
                                                // instruction fall on different banks (96: all on the same ones, G-way conflict)
template <int G>
constexpr int rmid_wave_doubles() { return ((G * RMID_ES * 2 + 1) & ~1) + RMID_TILE + 4; }   // E | tile | the samples' invalid flags (G <= 7 ints)

#ifndef PEM_RMID_WAVES
#define PEM_RMID_WAVES 3
#endif
// S samples share a wave in P passes: the S R (sample, radius) pairs are dealt over the lanes pass by pass -- pair f = 64 p + lane
// is radius f % R of sample f / R.  Only P = 1 is instantiated, S <= 64 / R samples side by side with the lanes past their pairs
// idle (25 radii use 50 lanes of 64, 33 radii 33): two- and three-pass packings fill 86-98 % of the lane slots and measured slower
// at every radius count (profiles/radii_mid_r04.txt).  The parameter itself stays for now: written without
// the one-iteration loops over p the five kernels compile to other instruction schedules, which a pure move of code must not do.
// (four samples' Gaussians and rows, or a second pass' amplitudes, leave LDS / registers for two waves per SIMD only)
template <int S, int P>
constexpr int rmid_waves_per_simd() { return (S >= 4 || P >= 2) ? 2 : PEM_RMID_WAVES; }
template <int S, int P>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(rmid_waves_per_simd<S, P>())))
void plume_rmid_kernel(PlumeIO io, RadiiMidArg radii_arg, int R, int ts) {
#pragma clang fp contract(off)
    constexpr int RS = (RMID_TILE / S) & ~1;    // doubles of the tile per sample (even)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* mine = reinterpret_cast<double*>(smem_raw) + (size_t)wave * rmid_wave_doubles<S>();
    double2* E = reinterpret_cast<double2*>(mine);   // [S][RMID_ES] {e1[k], e2[k]}
    double* tile = mine + ((S * RMID_ES * 2 + 1) & ~1);   // [S][RS] staged rows (16-byte aligned)
    int* badflag = reinterpret_cast<int*>(tile + RMID_TILE);   // [S] (the two spare doubles of the tile hold up to four; S <= 7: see rmid_wave_doubles)
    // this lane's pairs: (sample of the group, radius) per pass; a lane past the S R pairs repeats the last pair and keeps nothing
    int grp[P], rr[P];
    bool on[P];
    double rad[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int f = 64 * p + lane;
        on[p] = f < S * R;
        const int ff = on[p] ? f : S * R - 1;
        grp[p] = ff / R;
        rr[p] = ff - grp[p] * R;
        rad[p] = radii_arg.r[rr[p]];
    }
    const int kc = (RS - 2) / R;                      // rows per chunk: kc R + 1 <= RS - 1
    const long long nwaves = (long long)gridDim.x * (BLOCK / WAVE);
    const bool have_T = io.T != nullptr;
    const long long ntiles = (io.n + ts - 1) / ts;
    for (long long t = (long long)blockIdx.x * (BLOCK / WAVE) + wave; t < ntiles; t += nwaves) {
        // parameters of the tile's samples, one lane per sample (as plume_radii_kernel)
        const long long gl = (lane < ts && t * ts + lane < io.n) ? t * ts + lane : io.n - 1;
        const double c0_l = io.c0[gl], c1_l = io.c1[gl];
        const PlumeSetup ps_l = plume_setup(io.P_b[gl], c1_l, io.c2[gl], io.c3[gl], io.c4[gl], io.c5[gl], io.torr2pa);
        // (sigma, I_B0 and T of a sample are read again by its own lanes when its group comes up -- three loads that hit the cache --
        // instead of being carried in registers across the tile: with them the kernel was eight registers over three waves per SIMD)
        const double nn_l = ps_l.n_neutral;
        const double a1_l = ps_l.a1, a2_l = ps_l.a2;
        const double A1_l = (1.0 - c0_l) / normaliser(a1_l, 1.0 / (a1_l * a1_l), PEM_DPOLY);
        const double A2_l = c0_l / normaliser(a2_l, 1.0 / (a2_l * a2_l), PEM_DPOLY);
        const int in_tile = (int)(io.n - t * ts < ts ? io.n - t * ts : ts);
        for (int s0 = 0; s0 < in_tile; s0 += S) {
            // The Gaussians of the group's samples: the R lanes of a (sample, pass) take CHK consecutive angles each and advance
            // e_k = exp(-(k h / a)^2) by the two-term recurrence of the R = 1 kernel (e_{k+1} = e_k r_k, r_{k+1} = r_k q) from
            // three branch-free exp per beam.  A chunk in which the reference's own exp() has left the normal range (a value
            // below 1e-290), or whose widths are not finite numbers, is evaluated literally as the reference does
            // (plume.py:99-100), deep tail included.  (Straight into LDS: kept in a register array first the kernel spilled.)
            if (lane < S) badflag[lane] = 0;
            const int chk = (NANG + R - 1) / R;
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const int k0 = rr[p] * chk;
                const int sm = s0 + grp[p] < in_tile ? s0 + grp[p] : in_tile - 1;
                const double a1g = __shfl(a1_l, sm), a2g = __shfl(a2_l, sm);
                const double s1 = (GRID_H * GRID_H) * (1.0 / (a1g * a1g)), s2 = (GRID_H * GRID_H) * (1.0 / (a2g * a2g));
                double e1 = exp_nonpos(-(double)(k0 * k0) * s1), r1 = exp_nonpos(-(double)(2 * k0 + 1) * s1);
                double e2 = exp_nonpos(-(double)(k0 * k0) * s2), r2 = exp_nonpos(-(double)(2 * k0 + 1) * s2);
                const double q1 = exp_nonpos(-2.0 * s1), q2 = exp_nonpos(-2.0 * s2);
                double lo = __builtin_inf();
                for (int i = 0; i < chk; ++i) {
                    if (on[p] && k0 + i < NANG) E[grp[p] * RMID_ES + k0 + i] = make_double2(e1, e2);
                    lo = fmin(lo, fmin(e1, e2));
                    e1 *= r1;
                    r1 *= q1;
                    e2 *= r2;
                    r2 *= q2;
                }
                if (!(lo >= 1e-290) || !__builtin_isfinite(s1) || !__builtin_isfinite(s2)) {
                    for (int i = 0; i < chk; ++i) {
                        const int k = k0 + i;
                        const double alpha = k >= NANG - 1 ? HALF_PI : (double)k * GRID_H;
                        const double t1 = alpha / a1g, t2 = alpha / a2g;
                        if (on[p] && k < NANG) E[grp[p] * RMID_ES + k] = make_double2(exp(-(t1 * t1)), exp(-(t2 * t2)));
                    }
                }
            }
            // this lane's (sample, radius) pairs: amplitudes of plume.py:95-100
            bool smp_on[P];
            long long g[P];
            double b1[P], b2[P], jcx[P], den[P], num[P], thrust[P];
            bool bad[P];
#pragma unroll
            for (int p = 0; p < P; ++p) {
                smp_on[p] = on[p] && s0 + grp[p] < in_tile;
                const int src = s0 + grp[p] < in_tile ? s0 + grp[p] : in_tile - 1;      // an idle pair repeats the last sample and stores nothing
                g[p] = t * ts + src;
                const double A1 = __shfl(A1_l, src), A2 = __shfl(A2_l, src);
                const double n_neutral = __shfl(nn_l, src), sigma = io.sigma[g[p]];
                const double I_B0 = io.I_B0[g[p]];
                thrust[p] = have_T ? io.T[g[p]] : 0.0;
                const double decay = exp(-rad[p] * n_neutral * sigma);
                jcx[p] = I_B0 * (1.0 - decay) / (2.0 * PEM_PI * (rad[p] * rad[p]));
                const double base = I_B0 * decay / (rad[p] * rad[p]);
                b1[p] = base * A1;
                b2[p] = base * A2;
                den[p] = 0.0;
                num[p] = 0.0;
                bad[p] = false;
            }
            wave_lds_sync();
            for (int k0 = 0; k0 < NANG; k0 += kc) {
                const int rows = NANG - k0 < kc ? NANG - k0 : kc;
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    // where this pair's run starts in j_ion: the LDS copy gets the same parity
                    const double* gdst = io.j_ion + ((size_t)g[p] * NANG + k0) * R;
                    double* run = tile + grp[p] * RS + (int)((reinterpret_cast<uintptr_t>(gdst) >> 3) & 1);
                    if (on[p]) {
#pragma unroll 4
                        for (int kk = 0; kk < rows; ++kk) {
                            const int k = k0 + kk;
                            const double2 ee = E[grp[p] * RMID_ES + k];
                            const double f = b1[p] * ee.x + b2[p] * ee.y;      // j_beam + j_scat
                            const double ji = f + jcx[p];                      // plume.py:102
                            run[kk * R + rr[p]] = ji;
                            den[p] = __builtin_fma(PEM_SIMPSON_CDEN[k], f, den[p]);
                            num[p] = __builtin_fma(PEM_SIMPSON_CNUM[k], f, num[p]);
                            bad[p] |= ji <= 0.0;
                        }
                    }
                }
                wave_lds_sync();
                // the runs leave one after the other, the whole wave on each
                for (int gi = 0; gi < S; ++gi) {
                    if (s0 + gi >= in_tile) break;
                    double* dst = io.j_ion + ((size_t)(t * ts + s0 + gi) * NANG + k0) * R;
                    stream_run(tile + gi * RS + (int)((reinterpret_cast<uintptr_t>(dst) >> 3) & 1), dst, rows * R, lane);
                }
                wave_lds_sync();
            }
            // plume.py:105: a sample is invalid if alpha1 <= 0 or any of its values is <= 0 -- its pairs sit on several lanes and passes
#pragma unroll
            for (int p = 0; p < P; ++p)
                if (smp_on[p] && bad[p]) badflag[grp[p]] = 1;
            wave_lds_sync();
#pragma unroll
            for (int p = 0; p < P; ++p) {
                double cos_div = num[p] / den[p];   // plume.py:124-127
                if (cos_div == __builtin_inf()) cos_div = __builtin_nan("");
                const int src = s0 + grp[p] < in_tile ? s0 + grp[p] : in_tile - 1;
                const bool invalid = __shfl(a1_l, src) <= 0.0 || badflag[grp[p]] != 0;
                if (smp_on[p]) {
                    io.div[(size_t)g[p] * R + rr[p]] = acos(cos_div);
                    if (have_T) io.Tc[(size_t)g[p] * R + rr[p]] = thrust[p] * cos_div;
                    if (io.invalid && rr[p] == 0) io.invalid[g[p]] = (uint8_t)invalid;
                }
            }
            // plume.py:106: the whole block of an invalid sample becomes 1e-20 (rare: a second pass over it, the whole wave on each)
            for (int gi = 0; gi < S; ++gi) {
                if (s0 + gi >= in_tile) break;
                const bool invalid = __shfl(a1_l, s0 + gi) <= 0.0 || badflag[gi] != 0;
                if (invalid) {
                    double* blk = io.j_ion + (size_t)(t * ts + s0 + gi) * NANG * R;
                    for (int idx = lane; idx < NANG * R; idx += WAVE) blk[idx] = 1e-20;
                }
            }
            wave_lds_sync();
        }
        wave_lds_sync();
    }
}

struct RadiiSmallArg {
    double r[RADII_SMALL];
};

// ---------------------------------------------------------------------------------------------
// FEW radii by recurrence: the R = 1 fast path generalised (2 <= R <= RADII_SMALL).  The wave-per-sample kernel above is
// bound by LATENCY, not by issue or HBM: a wave has one sample in flight, and every sample is a chain Gaussians -> LDS ->
// wave reduction -> LDS -> block stream (5.4k cycles per sample measured at R = 2 where the instruction count says 1.3k;
// moving the per-radius work out of that chain gained 10-19 %: profiles/radii_probe_r02.txt).  Here a wave works on 8 samples at a time as plume_r1_kernel does: lane (s, c) walks
// angles k = 12 c .. 12 c + 11 of sample s, advancing the two Gaussians by the two-term recurrence (4 multiplies per
// angle) from chunk starts that come from the same recurrence at stride 12; per angle it forms the R values
// b1[r] e1 + b2[r] e2 + j_cex[r] from amplitudes it holds in registers and puts them -- R consecutive doubles -- into an LDS
// tile laid out as j_ion is, which leaves as 1-KiB-per-instruction 16-byte stores when the round is done.  The Simpson functionals of the two Gaussians ride along (4 FMAs per angle) and are folded over
// the 8 chunk lanes; cos_div / arccos / T_c of all (sample, radius) pairs of the 64-sample tile follow, one lane per pair.
// "Equal to the reference" in the deep tail is kept as in the R = 1 path: a chunk with a value below 1e-290 (or <= 0, or
// a non-finite amplitude) is re-evaluated literally with direct exp(); amplitudes of opposite sign or near overflow send
// the pair's divergence integrals through the literal angle-by-angle sum.
// LDS (doubles): shared: simpson[96][2] | dpoly[384];  per wave: params[8][64] | PB[64][R][3] | tile[8][91][R]
// ---------------------------------------------------------------------------------------------
constexpr int RF_L = 8, RF_S = WAVE / RF_L, RF_CH = 12;
static_assert(RF_L * RF_CH >= NANG && RF_L * RF_CH <= NSIMP, "8 chunks of 12 angles cover the 91-point grid inside the padded table");
// per wave: params[8][64] | PB[64][R][3] | tile[8][91][R] + 2; the workgroup has as many waves as fit 160 KB beside the tables
template <int R>
constexpr int rfew_wave_doubles() { return 8 * WAVE + 3 * WAVE * R + RF_S * NANG * R + 2; }
template <int R>
constexpr int rfew_waves() { return R <= 4 ? 4 : (R <= 6 ? 3 : 2); }

template <int R>   // the number of radii is a compile-time constant: amplitudes and the values of two angles live in registers
__global__ __launch_bounds__(WAVE * rfew_waves<R>()) void plume_rfew_kernel(PlumeIO io, RadiiSmallArg radii_arg) {
    constexpr int RM = R;
    // A round's 8 x 91 x R values go to an LDS tile in final order and leave as 1-KiB-per-instruction 16-byte stores, as in
    // the R = 1 path.  (Stored straight from the angle loop instead -- 16 bytes per lane, 64 separate pieces per instruction
    // -- the kernel ran at 2.1-2.4 TB/s; staged 3.7-4.7: profiles/radii_probe_r02.txt.)  The tile grows with R, so the
    // workgroup shrinks: 4 waves up to R = 4, 3 up to 6, 2 for 7 and 8.
    constexpr int NW = rfew_waves<R>();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* lds = reinterpret_cast<double*>(smem_raw);
    double2* tab_simpson = reinterpret_cast<double2*>(lds);
    double* tab_poly = lds + 2 * NSIMP;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    constexpr int per_wave = rfew_wave_doubles<R>();
    double* params = lds + TABLE_DOUBLES + wave * per_wave;     // rows: a1 a2 | r0 G E (beam 1) | r0 G E (beam 2)
    // a sample's rows 2..5 are free once its round has read them: they then carry its {s1d, s1n, s2d, s2n}
    double* PB = params + 8 * WAVE;                             // [64][R][3] {b1, b2, j_cex}
    double* tile = PB + 3 * WAVE * R;                           // [8][91][R] + 2
    for (int i = tid; i < NSIMP; i += WAVE * NW)
        tab_simpson[i] = i < NANG ? make_double2(PEM_SIMPSON_CDEN[i], PEM_SIMPSON_CNUM[i]) : make_double2(0.0, 0.0);
    for (int i = tid; i < PEM_NDI * PEM_NDC; i += WAVE * NW) tab_poly[i] = PEM_DPOLY[i];
    __syncthreads();

    const int s = lane % RF_S, c = lane / RF_S, k0 = c * RF_CH;
    const double2* my_w = tab_simpson + k0;
    const bool have_T = io.T != nullptr;
    const long long ntiles = (io.n + WAVE - 1) / WAVE;
    const long long nwaves = (long long)gridDim.x * NW;
    const size_t blk = (size_t)NANG * R;
    for (long long t = (long long)blockIdx.x * NW + wave; t < ntiles; t += nwaves) {
        const int in_tile = (int)(io.n - t * WAVE < WAVE ? io.n - t * WAVE : WAVE);
        const long long gl = lane < in_tile ? t * WAVE + lane : io.n - 1;     // idle lanes repeat the last sample
        // ------------------------------ prelude: one lane per sample ------------------------------
        unsigned literal_l = 0;
        {
            const double c0_l = io.c0[gl];
            const PlumeSetup ps = plume_setup(io.P_b[gl], io.c1[gl], io.c2[gl], io.c3[gl], io.c4[gl], io.c5[gl], io.torr2pa);
            const double sigma_l = io.sigma[gl], IB0_l = io.I_B0[gl];
            const double u1 = 1.0 / (ps.a1 * ps.a1), u2 = 1.0 / (ps.a2 * ps.a2);
            const double A1 = (1.0 - c0_l) / normaliser(ps.a1, u1, tab_poly);
            const double A2 = c0_l / normaliser(ps.a2, u2, tab_poly);
            const double s1 = (GRID_H * GRID_H) * u1, s2 = (GRID_H * GRID_H) * u2;
            params[0 * WAVE + lane] = ps.a1;
            params[1 * WAVE + lane] = ps.a2;
            params[2 * WAVE + lane] = exp_nonpos(-s1);
            params[3 * WAVE + lane] = exp_nonpos(-(2.0 * RF_CH) * s1);
            params[4 * WAVE + lane] = exp_nonpos(-(double)(RF_CH * RF_CH) * s1);
            params[5 * WAVE + lane] = exp_nonpos(-s2);
            params[6 * WAVE + lane] = exp_nonpos(-(2.0 * RF_CH) * s2);
            params[7 * WAVE + lane] = exp_nonpos(-(double)(RF_CH * RF_CH) * s2);
            for (int r = 0; r < R; ++r) {
#pragma clang fp contract(off)
                const double rad = radii_arg.r[r];
                const double decay = exp(-rad * ps.n_neutral * sigma_l);
                const double j_cex = IB0_l * (1.0 - decay) / (2.0 * PEM_PI * (rad * rad));
                const double base = IB0_l * decay / (rad * rad);
                const double b1 = base * A1, b2 = base * A2;
                double* pb = PB + (lane * R + r) * 3;
                pb[0] = b1;
                pb[1] = b2;
                pb[2] = j_cex;
                if (!(fabs(b1) + fabs(b2) < 1e300) || ((b1 < 0.0) != (b2 < 0.0) && b1 != 0.0 && b2 != 0.0)) literal_l |= 1u << r;
            }
        }
        const unsigned long long a1_nonpos = __ballot(params[0 * WAVE + lane] <= 0.0);
        wave_lds_sync();
        unsigned long long inv_mask = 0;
        // ------------------------------ rounds: 8 samples, 8 chunk lanes each ------------------------------
        for (int round = 0; round < RF_L; ++round) {
            const int smp = round * RF_S + s;
            const double r01 = params[2 * WAVE + smp], G1 = params[3 * WAVE + smp], E1 = params[4 * WAVE + smp];
            const double r02 = params[5 * WAVE + smp], G2 = params[6 * WAVE + smp], E2 = params[7 * WAVE + smp];
            double b1[RM], b2[RM], jc[RM];
            bool finite = true;
#pragma unroll
            for (int r = 0; r < RM; ++r) {
                const double* pb = PB + (smp * R + (r < R ? r : 0)) * 3;
                b1[r] = pb[0];
                b2[r] = pb[1];
                jc[r] = pb[2];
                finite = finite && __builtin_isfinite(b1[r]) && __builtin_isfinite(b2[r]);
            }
            // chunk start k0 = 12 c by the coarse recurrence: e_{k0} = E^(c^2), r_{k0} = r0 G^c
            double e1 = 1.0, e2 = 1.0, rr1 = r01, rr2 = r02, rho1 = E1, rho2 = E2;
            if (params[0 * WAVE + smp] == 0.0) e1 = e2 = __builtin_nan("");   // alpha1 = 0: exp(-(0/0)^2) is NaN in the reference
            const double E1sq = E1 * E1, E2sq = E2 * E2;
#pragma unroll
            for (int i = 0; i < RF_L - 1; ++i) {
                if (i < c) {
                    e1 *= rho1;
                    rho1 *= E1sq;
                    rr1 *= G1;
                    e2 *= rho2;
                    rho2 *= E2sq;
                    rr2 *= G2;
                }
            }
            const double q1 = r01 * r01, q2 = r02 * r02;
            double part[4] = {0.0, 0.0, 0.0, 0.0}, lo = __builtin_inf();
            double* dst = tile + (size_t)s * blk + (size_t)k0 * R;
            // The chunk's values are one run of 12 R consecutive doubles of the tile (laid out as j_ion is).  Two angles = 2 R doubles per iteration,
            // stored as R 16-byte pieces.  For an odd R the run of an odd sample starts at an odd double (the start is
            // (g 91 + 12 c) R doubles into a 16-byte aligned array): such a lane stores its first double on its own, then
            // pieces shifted by one element (the last element of an iteration is carried into the next), and the last
            // double on its own again -- selected per lane, so that every 16-byte store has all 64 lanes in it.
            const bool mis = (R & 1) && (smp & 1);
            double carry = 0.0;
#pragma unroll 1
            for (int jj = 0; jj < RF_CH; jj += 2) {
                double ev[2 * RM];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const double2 w = my_w[jj + h];
#pragma unroll
                    for (int r = 0; r < RM; ++r) ev[h * RM + r] = fma(b1[r], e1, b2[r] * e2) + jc[r];
                    part[0] = fma(w.x, e1, part[0]);
                    part[1] = fma(w.y, e1, part[1]);
                    part[2] = fma(w.x, e2, part[2]);
                    part[3] = fma(w.y, e2, part[3]);
                    e1 *= rr1;
                    rr1 *= q1;
                    e2 *= rr2;
                    rr2 *= q2;
                }
                double* d = dst + (size_t)jj * R;
                if (k0 + jj + 1 < NANG) {                  // both angles exist (all but the last iterations of the last chunk)
#pragma unroll
                    for (int i = 0; i < 2 * RM; ++i) lo = fmin(lo, ev[i]);
                    {
                        if constexpr ((R & 1) == 0) {
#pragma unroll
                            for (int q = 0; q < RM; ++q) *reinterpret_cast<f64x2*>(d + 2 * q) = f64x2{ev[2 * q], ev[2 * q + 1]};
                        } else {
                            if (mis && jj == 0) d[0] = ev[0];
#pragma unroll
                            for (int q = 0; q < RM; ++q) {
                                f64x2 pr;
                                pr.x = mis ? (q == 0 ? carry : ev[2 * q - 1]) : ev[2 * q];
                                pr.y = mis ? ev[2 * q] : ev[2 * q + 1];
                                if (!(mis && jj == 0 && q == 0)) *reinterpret_cast<f64x2*>(d + 2 * q - (mis ? 1 : 0)) = pr;
                            }
                            carry = ev[2 * RM - 1];
                            if (mis && jj + 2 >= RF_CH) d[2 * RM - 1] = carry;      // the run ends here: its last double
                        }
                    }
                } else {                                   // past 90 degrees: at most the first angle of the pair exists
                    if (k0 + jj < NANG) {
#pragma unroll
                        for (int r = 0; r < RM; ++r) lo = fmin(lo, ev[r]);
                        {
                            if ((R & 1) && mis && jj > 0) d[-1] = carry;           // the carried double of the iteration before
#pragma unroll
                            for (int r = 0; r < RM; ++r) d[r] = ev[r];
                        }
                    } else if ((R & 1) && mis && jj > 0 && k0 + jj - 1 < NANG) {
                        d[-1] = carry;
                    }
                    carry = 0.0;
                    // (nothing further of this chunk exists; the recurrence runs on harmlessly)
                }
            }
            // deep tail: where the reference's own exp() has left the normal range the chunk is evaluated literally
            const bool uncertain = lo < 1e-290 || !finite;
            if (__ballot(uncertain)) {
                if (uncertain) {
#pragma clang fp contract(off)
                    const double a1s = params[0 * WAVE + smp], a2s = params[1 * WAVE + smp];
                    part[0] = part[1] = part[2] = part[3] = 0.0;
                    lo = __builtin_inf();
                    for (int j = 0; j < RF_CH; ++j) {
                        const int k = k0 + j;
                        if (k >= NANG) break;
                        const double alpha = k == NANG - 1 ? HALF_PI : (double)k * GRID_H;
                        const double t1 = alpha / a1s, t2 = alpha / a2s;
                        const double g1 = exp(-(t1 * t1)), g2 = exp(-(t2 * t2));
                        for (int r = 0; r < R; ++r) {
                            const double* pb = PB + (smp * R + r) * 3;
                            const double ji = (pb[0] * g1 + pb[1] * g2) + pb[2];
                            lo = fmin(lo, ji);
                            dst[(size_t)j * R + r] = ji;
                        }
                        part[0] = __builtin_fma(my_w[j].x, g1, part[0]);
                        part[1] = __builtin_fma(my_w[j].y, g1, part[1]);
                        part[2] = __builtin_fma(my_w[j].x, g2, part[2]);
                        part[3] = __builtin_fma(my_w[j].y, g2, part[3]);
                    }
                }
            }
            // fold the 8 chunk lanes of a sample: Simpson functionals and plume.py:105
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int sh = RF_S; sh < WAVE; sh <<= 1) part[q] += __shfl_xor(part[q], sh);
            }
            if (c == 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) params[(2 + q) * WAVE + smp] = part[q];
            }
            unsigned long long bad = __ballot(lo <= 0.0);
#pragma unroll
            for (int sh = RF_S; sh < WAVE; sh <<= 1) bad |= bad >> sh;
            bad = (bad | (a1_nonpos >> (round * RF_S))) & ((1ull << RF_S) - 1);
            inv_mask |= bad << (round * RF_S);
            if ((bad >> s) & 1) {   // plume.py:106: the whole block of an invalid sample becomes 1e-20 (rare)
                for (int j = 0; j < RF_CH; ++j)
                    if (k0 + j < NANG)
                        for (int r = 0; r < R; ++r) dst[(size_t)j * R + r] = 1e-20;
            }
            {
                // the round's samples are one contiguous, 16-byte aligned piece of j_ion (round * 8 is even)
                wave_lds_sync();
                const long long first = t * WAVE + (long long)round * RF_S;
                long long valid = (io.n - first) * (long long)blk;          // doubles of this round that exist
                if (valid > (long long)RF_S * (long long)blk) valid = (long long)RF_S * (long long)blk;
                // (for an odd R every other round starts 64 bytes into a 128-byte line: stream_run brings the body back onto
                // line boundaries with one leading partial instruction)
                if (valid > 0) stream_run(tile, io.j_ion + (size_t)first * blk, (int)valid, lane);
                wave_lds_sync();   // the tile is rewritten by the next round
            }
        }
        wave_lds_sync();
        if (io.invalid && lane < in_tile) io.invalid[t * WAVE + lane] = (uint8_t)((inv_mask >> lane) & 1);
        // ------------------------------ postlude: one lane per (sample, radius) pair ------------------------------
        const int pairs = in_tile * R;
        for (int idx = lane; idx < pairs; idx += WAVE) {
            const int smp = idx / R, r = idx - smp * R;
            const unsigned literal = (unsigned)__shfl((int)literal_l, smp);
            const double* pb = PB + idx * 3;
            const double s1d = params[2 * WAVE + smp], s1n = params[3 * WAVE + smp], s2d = params[4 * WAVE + smp], s2n = params[5 * WAVE + smp];
            double num, den;
            {
#pragma clang fp contract(off)
                num = pb[0] * s1n + pb[1] * s2n;
                den = pb[0] * s1d + pb[1] * s2d;
            }
            if ((literal >> r) & 1) {   // the reference's own summation order (amplitudes of opposite sign / near overflow)
#pragma clang fp contract(off)
                const double a1s = params[0 * WAVE + smp], a2s = params[1 * WAVE + smp];
                num = 0.0;
                den = 0.0;
                for (int k = 0; k < NANG; ++k) {
                    const double alpha = k == NANG - 1 ? HALF_PI : (double)k * GRID_H;
                    const double t1 = alpha / a1s, t2 = alpha / a2s;
                    const double f = pb[0] * exp(-(t1 * t1)) + pb[1] * exp(-(t2 * t2));
                    den = __builtin_fma(tab_simpson[k].x, f, den);
                    num = __builtin_fma(tab_simpson[k].y, f, num);
                }
            }
            double cos_div = num / den;
            if (cos_div == __builtin_inf()) cos_div = __builtin_nan("");
            const long long g = t * WAVE + smp;
            io.div[(size_t)g * R + r] = acos(cos_div);
            if (have_T) io.Tc[(size_t)g * R + r] = io.T[g] * cos_div;
        }
        wave_lds_sync();   // params / PB are rewritten by the next tile
    }
}

template <int R>
int launch_rfew(size_t n, hipStream_t st, const PlumeIO& io, const RadiiSmallArg& ra) {
    constexpr int NW = rfew_waves<R>();
    constexpr size_t lds = (size_t)(TABLE_DOUBLES + NW * rfew_wave_doubles<R>()) * 8;
    static_assert(lds <= 160 * 1024, "the few-radii kernel's workgroup must fit the LDS");
    if (lds > 64 * 1024) {
        static pem::LdsAttrOnce attr;
        HIP_TRY(attr.ensure(reinterpret_cast<const void*>(plume_rfew_kernel<R>)));
    }
    int cus = 256;
    HIP_TRY(pem::device_cus(&cus));
    const size_t per_cu = (160 * 1024) / lds < 2 ? 1 : 2;          // persistent: workgroups resident per CU
    size_t grid = ((n + WAVE - 1) / WAVE + NW - 1) / NW;
    grid = balanced_grid(grid, (size_t)cus * per_cu);     // (grids of 2 / 4 x the slots or one tile per wave: within 2 %, r03o)
    hipLaunchKernelGGL(plume_rfew_kernel<R>, dim3((unsigned)grid), dim3(WAVE * NW), lds, st, io, ra);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

}  // namespace

// pem_plume_f64_dev (csrc/pem_kernels.hip) past its argument checks and its one-radius branch
int pem::launch_plume_radii(size_t n, int n_radii, const double* radii, const PlumeIO& io, hipStream_t st) {
    if (n_radii >= 2 && n_radii <= RADII_SMALL && aligned16(io.j_ion)) {
        // few radii: eight samples per wave in flight, Gaussians by recurrence, profile stored from the angle loop
        RadiiSmallArg ra;
        for (int r = 0; r < RADII_SMALL; ++r) ra.r[r] = r < n_radii ? radii[r] : 1.0;
        switch (n_radii) {
            case 2: return launch_rfew<2>(n, st, io, ra);
            case 3: return launch_rfew<3>(n, st, io, ra);
            case 4: return launch_rfew<4>(n, st, io, ra);
            case 5: return launch_rfew<5>(n, st, io, ra);
            case 6: return launch_rfew<6>(n, st, io, ra);
            case 7: return launch_rfew<7>(n, st, io, ra);
            default: return launch_rfew<8>(n, st, io, ra);
        }
    }
    // (read per call: tests walk through the instantiations)
    int rmid_min = getenv("PEM_RMID_MIN") ? atoi(getenv("PEM_RMID_MIN")) : 13;
    if (rmid_min < WAVE / RMID_G_MAX + 1) rmid_min = WAVE / RMID_G_MAX + 1;
    if (n_radii >= rmid_min && n_radii > RADII_SMALL && n_radii <= RMID_MAX) {
        // S samples in flight per wave in one pass, rows staged in LDS, line-aligned 16-byte stores (plume_rmid_kernel): as many samples, of the
        // one to RMID_G_MAX it is instantiated for, as fill the most lanes, S R of 64 (25 radii: two samples, 50 lanes).
        // From 13 radii on (round 4, with the 10-KB tile: 13 / 14 / 15 / 16 radii 3.02 -> 3.35, 3.30 -> 3.73, 3.35 -> 3.57, 4.26 -> 4.38 TB/s
        // against the wave-per-sample kernel below, interleaved; profiles/radii_mid_r04.txt); at 11 and 12 radii (PEM_RMID_MIN=11) it
        // works and gains nothing.
        // The kernel's bound is its phase structure -- the head / body / tail of a run and the two syncs around it -- not idle lanes
        // (why packing more samples into a wave in several passes lost: DESIGN.md section 4.2).  What separates 32 / 40 / 48 / 64 radii
        // (4.6-4.9 TB/s) from their neighbours (3.7-4.3) is the alignment of a sample's rows to 128-byte lines, not the lane count.
        int S = 1;
        for (int c = 2; c <= RMID_G_MAX; ++c)
            if (c * n_radii <= WAVE && (RMID_TILE / c - 2) / n_radii >= 1) S = c;      // (a staged row per sample must fit)
        if (const char* e = getenv("PEM_RMID_SP")) {                                   // tests / experiments: "S,1" of an instantiated S
            int es = 0, ep = 0;
            if (sscanf(e, "%d,%d", &es, &ep) == 2 && ep == 1 && es >= 1 && es <= RMID_G_MAX && es * n_radii <= WAVE &&
                (RMID_TILE / es - 2) / n_radii >= 1)
                S = es;
        }
        RadiiMidArg ra;
        for (int r = 0; r < RMID_MAX; ++r) ra.r[r] = r < n_radii ? radii[r] : 1.0;
        int ts = WAVE;                             // samples per wave tile: fewer when the batch is small
        while (ts > 8 && (n + ts - 1) / ts < 256 * 32) ts >>= 1;
        ts = ts / S * S;                           // whole groups only
        if (ts < 2 * S) ts = 2 * S <= WAVE ? 2 * S : S;
        if (const char* e = getenv("PEM_RMID_TS")) ts = atoi(e);                      // experiments
        if (ts < 1 || ts > WAVE) return fail(PEM_ERR_INVALID_ARG, "pem_plume: PEM_RMID_TS must be 1..64");
        const size_t ntiles = (n + ts - 1) / ts;
        int cus = 256;
        HIP_TRY(pem::device_cus(&cus));
        size_t blocks = (ntiles + BLOCK / WAVE - 1) / (BLOCK / WAVE);
#define PEM_RMID_LAUNCH(S_)                                                                                         \
    do {                                                                                                            \
        const size_t lds = (size_t)(BLOCK / WAVE) * rmid_wave_doubles<S_>() * 8;                                    \
        size_t per_cu = (160 * 1024) / lds;                                                                         \
        if (per_cu > (size_t)rmid_waves_per_simd<S_, 1>()) per_cu = rmid_waves_per_simd<S_, 1>();                   \
        static pem::LdsAttrOnce attr;                          /* (four and five samples per wave: more than 64 KB) */ \
        HIP_TRY(attr.ensure(reinterpret_cast<const void*>(plume_rmid_kernel<S_, 1>)));                              \
        blocks = balanced_grid(blocks, (size_t)cus * per_cu);                                                       \
        hipLaunchKernelGGL((plume_rmid_kernel<S_, 1>), dim3((unsigned)blocks), dim3(BLOCK), lds, st, io, ra, n_radii, ts); \
    } while (0)
        switch (S) {
            case 1: PEM_RMID_LAUNCH(1); break;
            case 2: PEM_RMID_LAUNCH(2); break;
            case 3: PEM_RMID_LAUNCH(3); break;
            case 4: PEM_RMID_LAUNCH(4); break;
            default: PEM_RMID_LAUNCH(5); break;
        }
#undef PEM_RMID_LAUNCH
        HIP_TRY(hipGetLastError());
        return PEM_OK;
    }
    if (n_radii >= 2 && n_radii <= RADII_MAX) {
        // wave per sample, coalesced (91, R) blocks, literal Gaussians (per 1e5..1e6 samples, tools/radii_probe.py: R = 25:
        // 7415 -> 614 us, R = 5: 2089 -> 795 us, R = 3: 1262 -> 940 us, R = 2: 1183 -> 1314 us)
        RadiiArg ra;
        for (int r = 0; r < RADII_MAX; ++r) ra.r[r] = r < n_radii ? radii[r] : 1.0;
        int ts = WAVE;                             // samples per wave tile: fewer when the batch is small
        while (ts > 4 && (n + ts - 1) / ts < 256 * 20) ts >>= 1;
        const size_t ntiles = (n + ts - 1) / ts;
        size_t blocks = (ntiles + BLOCK / WAVE - 1) / (BLOCK / WAVE);
        blocks = balanced_grid(blocks, 256 * 5);   // persistent: 31 KB of LDS per workgroup, five per CU
        hipLaunchKernelGGL(plume_radii_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, st, io, ra, n_radii, ts);
        HIP_TRY(hipGetLastError());
        return PEM_OK;
    }
    // lane-per-sample kernel (more than RADII_MAX radii; one radius with an unaligned j_ion): the radii go to the device
    // through a small stream-ordered allocation, and -- `radii` being the caller's host memory -- this one path waits
    // for the stream before it returns
    double* d_radii = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&d_radii), sizeof(double) * n_radii, st));
    HIP_TRY(hipMemcpyAsync(d_radii, radii, sizeof(double) * n_radii, hipMemcpyHostToDevice, st));
    const size_t blocks = (n + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(plume_generic_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, st, io, d_radii, n_radii);
    hipError_t le = hipGetLastError();
    HIP_TRY(hipFreeAsync(d_radii, st));
    HIP_TRY(le);
    HIP_TRY(hipStreamSynchronize(st));
    return PEM_OK;
}
