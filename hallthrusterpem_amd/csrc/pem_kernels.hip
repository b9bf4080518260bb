// pem_kernels.hip -- the gfx950 (MI355X, CDNA4) kernel of the one-radius plume path, plume_r1_kernel, its launch planning and the
// entry points of libpem_hip.so's C ABI that launch it.
//
// What is computed (reference file:line, upstream repository root):
//   cathode stage    src/hallmd/models/cathode.py:24-38
//   thruster stage   tests/sim_hallthruster.jl:35-48 (the reference's analytic test double)
//   plume stage      src/hallmd/models/plume.py:39-140
//
// Kernel shape (DESIGN.md holds the measurements behind each choice).  The path is a streaming map,
// 120 B in and 752 B out per sample; the first version was VALU-bound on fp64 transcendentals
// (1246 VALU instructions per 16 samples), so the design removes them until HBM writes are the bound:
//   * One 64-lane wave owns 64 consecutive samples per tile and is persistent over tiles; a workgroup is 4 such
//     waves that share two LDS tables and nothing else (8 waves per CU).
//   * PRELUDE, one lane per sample, nothing redundant: cathode + thruster stages, alpha1/alpha2, the two
//     normalisers, beam amplitudes.  The normaliser D(a) = 2 pi Int_0^{pi/2} exp(-(t/a)^2) sin t dt
//     (identical to the six complex erfi of plume.py:64-85) is a degree-11 polynomial in u = 1/a^2 from a
//     32-interval LDS table (|a| >= 0.25) or a 10-term series (|a| < 0.25) -- no quadrature, no erfi.
//   * ROUNDS: the wave then walks its 64 samples in L rounds of S = 64/L samples; in a round lane
//     (s, c) produces angles k = c*CH .. c*CH+CH-1 (CH = ceil(91/L)) of sample s.  The two Gaussians
//     exp(-(k h / a)^2) advance along k by the two-term recurrence e_{k+1} = e_k r_k, r_{k+1} = r_k q,
//     and the chunk starts come from the same recurrence at stride CH -- so a sample costs 7 exp in
//     total (3 per beam + the CEX decay) instead of 182 + 6 erfi.
//   * The Simpson sums of plume.py:117-123 ride in the same loop (folded weights from an LDS table).
//   * A round's S x 91 profile block is contiguous in j_ion (R = 1): it is staged in LDS in final order
//     and leaves as 16-byte-per-lane, 1-KiB-per-instruction stores.
//   * EPILOGUE, one lane per sample again: cos_div, arccos, T_c, coalesced 512-byte stores.
//   * Without a profile (reduced-QoI mode) the rounds are skipped: the divergence integrals come from tabulated
//     Simpson functionals of the beam width (simpson_functionals), per sample, wherever that is exact to rounding.
//   * Where the reference's own exp() has left the normal range (deep tail of a narrow beam with j_cex = 0, infinite
//     amplitudes) a chunk is re-evaluated literally (exact_chunk): "equal to the reference" beats "accurate" there.
//   * The same tile loop carries the fused modes: Monte-Carlo inputs generated in the prelude (MC) and the likelihood of
//     measured current densities (JMODE 3) consuming the profile on chip.  (The fused SVD compression is a lane-per-sample
//     kernel of its own, csrc/pem_latent.hip.)
//   Elsewhere: plume_rfew_kernel (2..8 sweep radii: this design generalised), plume_rmid_kernel / plume_radii_kernel /
//   plume_generic_kernel (more radii) in csrc/pem_radii.hip; cathode, thruster, u_ion profile and the post-run filters in
//   csrc/pem_stages.hip; the host-pointer entry points in csrc/pem_host.hip; the host side of the fused campaign statistics in
//   csrc/pem_campaign.hip.  What these share is csrc/pem_plume.h; the per-sample scalar stages and tables are csrc/pem_model.h
//   (shared with the lane-per-sample kernels, csrc/pem_saltelli.hip and csrc/pem_latent.hip).
//
// This file is written for gfx950 only: 64-wide waves, 160 KiB LDS, no portability layer.
#include <cmath>
#include <cstdlib>
#include <atomic>
#include <mutex>
#include <type_traits>

#include "pem_math.h"
#include "pem_philox.h"
#include "pem_plume.h"

namespace {

using namespace pem;
using namespace pem_model;

// ---------------------------------------------------------------------------------------------
// kernel arguments
// ---------------------------------------------------------------------------------------------
struct CoupledIO {
    const double *V_a, *T_e, *V_vac, *Pstar, *P_T, *mdot_a, *a_1;
    double *V_cc, *I_B0, *T;
};

// fused Monte-Carlo mode: the 15 coupled inputs are generated in registers from the counter-based design instead
// of being read from HBM (order of COUPLED inputs: P_b V_a T_e V_vac Pstar P_T mdot_a a_1 c0..c5 sigma_cex)
struct McDesign {
    unsigned long long seed, first;
    unsigned int stream;
    int swap_dim;           // Saltelli blocks, as pem_sample_f64_dev: -1 plain, -2 all from stream+1, d >= 0 column d
    int kind[15];
    double a[15], b[15];
    double* x_out;          // optional [15][ld] copy of the generated inputs
    unsigned long long ld;
};

// fused multi-QoI likelihood mode (JMODE 6): the ragged measurement table, copied into LDS at kernel start.  Records are
// 32 bytes {w, y, 1/std, bits} (pem_hip.h, pem_coupled_system_loglik_f64_dev): j_ion {w, y, 1/std, k}, u_ion {w, y, 1/std, p},
// V_cc and T {0, y, 1/std, 0}; span[c][kind] = {first record, count} of condition c, kinds PEM_SYS_* (j_ion, V_cc, T, u_ion);
// node[p] = a grid index of u_ion, whose denominator 1 + exp(-100 (z - 0.04)) is evaluated once per workgroup.
struct SystemTable {
    const double* rec;
    const int32_t* span;
    const int32_t* node;
    int n_rec, n_node;
    double z0, z1;
    int ncells;
};

// record predictions (JMODE 7): JMODE 6's table, and where the model value of every record goes -- pred[d * ld_pred + r]
// for record r of sample i = d * n_cond + c (pem_coupled_system_predict_f64_dev)
struct SystemPredict : SystemTable {
    double* pred;
    long long ld_pred;
};

// several sweep radii (JMODE 8 / 9): JMODE 6 / 7's table with the fourth word of a j_ion record carrying k | (ridx << 8), ridx an
// index into `radii` (pem_coupled_system_loglik_radii_f64_dev); `pred` is unused in JMODE 8.  The radii travel in the kernel
// arguments: no device allocation, no copy to wait for.
constexpr int SYS_RADII_MAX = PEM_FUSED_SYSTEM_MAX_RADII;
struct SystemRadii : SystemPredict {
    int n_radii;
    double radii[SYS_RADII_MAX];
};

// the per-sample inputs of one lane, prefetched one tile ahead
template <bool COUPLED>
struct SampleIn {
    double P_b, c0, c1, c2, c3, c4, c5, sigma;
    double x0, x1, x2, x3, x4, x5, x6;  // COUPLED: V_a T_e V_vac Pstar P_T mdot_a a_1 ; else I_B0, T, unused
};

template <bool COUPLED>
__device__ __forceinline__ SampleIn<COUPLED> load_sample(const PlumeIO& io, const CoupledIO& cio, long long gi) {
    SampleIn<COUPLED> v;
    gi = (gi >> 6) * io.in_tile_stride + (gi & 63);
    v.P_b = io.P_b[gi];
    v.c0 = io.c0[gi];
    v.c1 = io.c1[gi];
    v.c2 = io.c2[gi];
    v.c3 = io.c3[gi];
    v.c4 = io.c4[gi];
    v.c5 = io.c5[gi];
    v.sigma = io.sigma[gi];
    if constexpr (COUPLED) {
        v.x0 = cio.V_a[gi];
        v.x1 = cio.T_e[gi];
        v.x2 = cio.V_vac[gi];
        v.x3 = cio.Pstar[gi];
        v.x4 = cio.P_T[gi];
        v.x5 = cio.mdot_a[gi];
        v.x6 = cio.a_1[gi];
    } else {
        v.x0 = io.I_B0[gi];
        v.x1 = io.T ? io.T[gi] : 0.0;
        v.x2 = v.x3 = v.x4 = v.x5 = v.x6 = 0.0;
    }
    return v;
}

// Out of line on purpose: inlined fifteen times, the library exp / normcdfinv bodies of the transforms pushed the
// fused kernel past 256 VGPRs (204 bytes of scratch per lane).
__device__ __attribute__((noinline)) double transform_call(int kind, double a, double b, double u) {
    return pem::transform(kind, a, b, u);
}

// inputs of global sample `g` from the design: bit-identical to pem_sample_f64_dev followed by a load
// `design`: the LDS copy of the design's 15 x (a, b, kind) made at kernel start (MC_LDS_DOUBLES: a[15] | b[15] | pad |
// kind[15] as ints).  Read from the kernel arguments inside the tile loop instead, those 75 SGPRs were spilled to VGPR
// lanes and restored around every out-of-line transform call: ~370 v_readlane / v_writelane per tile (310 SGPR spills).
constexpr int MC_LDS_DOUBLES = 48;
__device__ __forceinline__ SampleIn<true> generate_sample(const McDesign& mc, const double* design, long long g_local) {
    const int* design_kind = reinterpret_cast<const int*>(design + 32);
    const unsigned long long g = mc.first + (unsigned long long)g_local;
    const unsigned int k0 = (unsigned int)mc.seed, k1 = (unsigned int)(mc.seed >> 32);
    double x[16];
    // All eight Philox blocks first: they are independent chains of quarter-rate 32x32 multiplies, and the out-of-line
    // transform calls between them would keep the scheduler from interleaving them.
    double u[16];
#pragma unroll
    for (int pair = 0; pair < 8; ++pair) {
        // the two dimensions of a pair may come from different streams in a Saltelli block (wave-uniform choice)
        const unsigned int st0 = mc.stream + ((mc.swap_dim == -2 || mc.swap_dim == 2 * pair) ? 1u : 0u);
        const unsigned int st1 = mc.stream + ((mc.swap_dim == -2 || mc.swap_dim == 2 * pair + 1) ? 1u : 0u);
        const pem::Philox4 r = pem::philox4x32_10((unsigned int)g, (unsigned int)(g >> 32), (unsigned int)pair, st0, k0, k1);
        pem::Philox4 r1 = r;
        if (2 * pair + 1 < 15 && st1 != st0)
            r1 = pem::philox4x32_10((unsigned int)g, (unsigned int)(g >> 32), (unsigned int)pair, st1, k0, k1);
        u[2 * pair] = pem::u53(r.x, r.y);
        u[2 * pair + 1] = pem::u53(r1.z, r1.w);
    }
#pragma unroll
    for (int d = 0; d < 15; ++d) x[d] = transform_call(__builtin_amdgcn_readfirstlane(design_kind[d]), design[d], design[15 + d], u[d]);
    if (mc.x_out) {
#pragma unroll
        for (int d = 0; d < 15; ++d) mc.x_out[(size_t)d * mc.ld + g_local] = x[d];
    }
    SampleIn<true> v;
    v.P_b = x[0]; v.x0 = x[1]; v.x1 = x[2]; v.x2 = x[3]; v.x3 = x[4]; v.x4 = x[5]; v.x5 = x[6]; v.x6 = x[7];
    v.c0 = x[8]; v.c1 = x[9]; v.c2 = x[10]; v.c3 = x[11]; v.c4 = x[12]; v.c5 = x[13]; v.sigma = x[14];
    return v;
}

// ---------------------------------------------------------------------------------------------
// fast path: R = 1.  Each wave is persistent over 64-sample tiles; WPB independent waves per workgroup.
//   L        lanes that share a sample during the rounds (2, 4 or 8)
//   COUPLED  cathode + thruster stages are evaluated in front of the plume (inputs from CoupledIO)
//   JMODE    0: reduced-QoI mode, no profile;  1: stage and store the 91-point profile as fp64;
//            2: mixed mode -- same fp64 arithmetic, profile rounded once to fp32 when it is staged
//            3: fused likelihood -- the profile is staged in LDS only and reduced against measured current
//               densities there (csrc/pem_likelihood.hip's formula); nothing but scalars leaves the chip
//            (the fused compression mode -- latent = norm(j_ion) @ basis -- is a kernel of its own, one lane per sample:
//            csrc/pem_latent.hip)
//            4: as 1, and the staged profile is COUNTED against the brackets of a percentile selection on its way out (count_round);
//            5: the same without the stores -- the percentiles of a profile that is never written
//            6: fused multi-QoI likelihood -- JMODE 3's j_ion records against the staged profile, plus V_cc, thrust and u_ion
//               records of the sample's condition in the epilogue (system_epilogue_sum)
//            7: record predictions -- JMODE 6's table, the model value of every record stored instead of compared
//               (j_ion in the rounds, jion_records_store; the others in the epilogue, system_epilogue_store)
//            8, 9: JMODE 6 and 7 against j_ion measured at 2 .. 8 sweep radii, still ONE model evaluation per sample.  The profile
//               is j_ion(r, alpha_k) = base(r) g(alpha_k) + j_cex(r) and the shape g = A1 exp(-(alpha/a1)^2) + A2 exp(-(alpha/a2)^2)
//               does not depend on r: the rounds stage g (the angle loop with amplitudes A1, A2 and no j_cex), the sample's pairs
//               {base(r), j_cex(r)} sit beside it, and a record applies the pair of its radius to the interpolated g.
// LDS map (doubles): shared by the workgroup: simpson[96][2] | dpoly[32*12];  per wave: params[NROWS][64] |
// tile[S*91] | 2 (sink).  The Simpson table is padded with zero weights to L*CH <= 96 entries so the angle loop
// needs no branch (NSIMP, TABLE_DOUBLES: csrc/pem_plume.h).  The den/num partial sums of a round reuse the rows of
// `params` that the round has consumed.
// ---------------------------------------------------------------------------------------------
constexpr int NPARAM = 9;   // X1 X2 jcex | r0 G E (beam 1) | r0 G E (beam 2)
constexpr int WPB = 4;      // waves per workgroup (they share the two tables and nothing else)
template <int L>
constexpr int param_rows() { return 2 * L > NPARAM ? 2 * L : NPARAM; }   // rows 2c, 2c+1 are reused for the Simpson partials
constexpr int QPOLY_DOUBLES = (PEM_NDI + PEM_NQB) * PEM_NDC * 2;
template <int L, int JMODE>
constexpr int wave_lds_doubles() {
    return param_rows<L>() * WAVE +
           ((JMODE == 1 || JMODE == 3 || JMODE == 4 || JMODE == 5 || JMODE == 6 || JMODE == 7 || JMODE == 8 || JMODE == 9) ? (WAVE / L) * NANG + 2 : JMODE == 2 ? ((WAVE / L) * NANG + 4) / 2 : 0);
}
template <int L, int JMODE>
constexpr int fast_lds_doubles() { return TABLE_DOUBLES + WPB * wave_lds_doubles<L, JMODE>(); }

// tuning knobs of the fused modes (file scope: a #define inside a function body does not survive -save-temps)
#ifndef PEM_LOGLIK_MU
#define PEM_LOGLIK_MU 2       // measurement records in flight per lane in the fused likelihood mode
#endif

// LDS views of one wave
struct WaveLds {
    const double* meas;      // fused likelihood: [n_cond*n_ang] records {weight, y, inv_std, k (integer bits)}, or nullptr
    const int2* span;        // JMODE 6: [n_cond][4] {first record, count} of each kind (meas holds the records)
    const double* unode;     // JMODE 6: [max(n_node, 2)] u_ion denominators 1 + exp(-100 (z_k - 0.04))
    int n_unode;
    double* pred;            // JMODE 7: the [draws][ld_pred] predictions in HBM
    long long ld_pred;
    const double* rtab;      // JMODE 8 / 9: [n_radii][3] {r, 1 / r^2, 1 / (2 pi r^2)}
    double2* pairs;          // JMODE 8 / 9: this wave's [S][n_radii] {base(r), j_cex(r)} of the round's samples
    int n_radii;
    const double2* simpson;  // [96] {cden, cnum}
    const double* poly;      // [32*12]
    const double2* qpoly;    // reduced-QoI mode: [(32+64)*12] {Qd, Qn} coefficients of the Simpson functionals, or nullptr
    double* params;          // [9][64]
    double* tile;            // [S*91] + 2
    unsigned tile_off;       // its byte offset in the workgroup's dynamic LDS (counting modes)
};

// The slow, literal evaluation of one lane's chunk of angles: direct exp() of -(alpha_k / alpha)^2 per beam, every
// product and sum rounded separately, as plume.py:99-102 (and the oracle) do.  The recurrence of the angle loop is
// accurate to ~1e-14 relative -- also where the reference's own exp() has run into the denormal range (argument
// below -708) or rounded to zero (below -745.13), which is where "accurate" and "equal to the reference" part ways:
// with j_cex = 0 the reference sees j_ion = 0 there and flags the sample invalid (plume.py:105).  A chunk whose
// smallest value is below 1e-290 (or <= 0) is therefore recomputed this way; under the PEM-v0 priors j_cex > 1e-6
// and this never runs.  Out of line: it must not cost the angle loop registers.
struct ChunkSums {
    double den, num, lo;
};
template <typename JT, bool WRITE_J>
__device__ __attribute__((noinline)) ChunkSums exact_chunk(double X1a, double X2a, double jcex, double a1, double a2, int k0,
                                                           int nk, const double2* w, JT* tile_row) {
#pragma clang fp contract(off)
    ChunkSums r{0.0, 0.0, __builtin_inf()};
    for (int j = 0; j < nk; ++j) {
        const int k = k0 + j;
        if (k >= NANG) break;
        const double alpha = k == NANG - 1 ? HALF_PI : (double)k * GRID_H;   // np.linspace(0, pi/2, 91)
        const double t1 = alpha / a1, t2 = alpha / a2;
        const double f = X1a * exp(-(t1 * t1)) + X2a * exp(-(t2 * t2));
        const double ji = f + jcex;
        if (WRITE_J) tile_row[j] = (JT)ji;
        r.lo = fmin(r.lo, WRITE_J ? ji : f);
        r.den = __builtin_fma(w[j].x, f, r.den);
        r.num = __builtin_fma(w[j].y, f, r.num);
    }
    return r;
}

// ---- counting modes (JMODE 4 / 5): the round tile against the brackets of a percentile selection -------------------------------
// The profile's percentiles over the samples (gen_data.py:163-168, monte_carlo.py:363-658) need, per (angle, quantile), the
// number of values below a bracket and the values inside it (csrc/pem_quantile.hip: the pilot form).  A round's S x 91 values sit
// in LDS in final order, so the wave changes roles once more: lane = angle (two slots: angles 0..63 and 64..90), down the S
// samples of the round.  Per (value, bracket) one subtraction of high words -- its borrow is "below", t <= words is "inside"
// (brackets end on whole words and do not overlap: the selection falls back otherwise) -- with the counts in registers for a round
// and in per-workgroup LDS counters between rounds.  The few per cent of values inside a bracket are noted as one bit per (slot,
// sample) and leave as 16-byte records {key, angle * nq + quantile}, appended to the wave's own region of the record buffer
// (no atomics: the count lives in a scalar register) by however many lanes have one left, until none has.
// Its LDS operands are byte offsets into the workgroup's dynamic LDS (as an out-of-line function it must not take generic pointers:
// they would turn its LDS traffic into flat accesses).
// What count_round needs and the rounds do not: kept in the wave's own LDS words (a record of 48 bytes written once per launch),
// so that the call carries four arguments and nothing of this stays live in the caller's registers across the rounds (as
// arguments they cost the counting kernels 8-56 bytes of stack for registers saved around the call).
struct CountCtx {
    pem::Record* rec;            // this wave's region of the record buffer
    uint8_t* row_certain;        // the premask's per-sample counts (whole arrays), or nullptr
    uint8_t* row_uncertain;
    unsigned cap;                // records the region holds
    unsigned tab_off;            // LDS [91][NQ] {loh, words}
    unsigned below_off;          // LDS [NQ][91]
    unsigned pm_off;             // LDS [91] uint4: the premask's thresholds
};
struct QCount {
    unsigned ctx_off;            // LDS: this wave's CountCtx
    unsigned below_off;          // LDS [NQ][91] (the kernel's final flush)
    unsigned cap, cnt;           // region size; records produced so far (wave-uniform)
};
struct NoCount {};

// PM: the outlier test of gen_data.py:163-168 rides along (the "premask").  A sample is an outlier of the profile when more than
// int(0.75 * 91) of its values lie outside [p25 - f iqr, p75 + f iqr] per angle -- bounds that are not known until the selection
// is done.  But p25 and p75 are known to lie in their brackets, so the bounds lie in intervals [lo_min, lo_max], [hi_min, hi_max]
// (rounded as numpy rounds them; every operation is monotone), and a value is either OUTSIDE FOR CERTAIN (below lo_min or above
// hi_max), INSIDE FOR CERTAIN, or uncertain (in one of the two intervals: about one value in a hundred).  Per sample the two
// counts leave as bytes; the caller settles the few samples whose verdict the uncertain values could change.  Four comparisons of
// high words per value, kept as wave masks; a row's counts are population counts of those masks.
// Inlined into the (rolled) rounds.  Its first version, inlined with every loop unrolled, cost the kernel 140 registers and one wave
// per SIMD, so it went out of line -- where the premask variant saved two callee-saved registers on the stack per call (8 bytes
// of scratch).  With the sample loops rolled in groups of four the inlined form fits two waves per SIMD (209-228 registers, no
// scratch) and measures the same (5.13-5.21 against 5.18-5.22 ms per 1e7-sample campaign).
template <int NQ, int S, bool FULL, bool PM>
__device__ __forceinline__ unsigned count_round(unsigned ctx_off, unsigned tile_off, unsigned cnt, int lane, int rows, long long first) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const CountCtx ctx = *reinterpret_cast<const CountCtx*>(smem_raw + ctx_off);
    const uint2* tab = reinterpret_cast<const uint2*>(smem_raw + ctx.tab_off);
    unsigned* below = reinterpret_cast<unsigned*>(smem_raw + ctx.below_off);
    const double* tile = reinterpret_cast<const double*>(smem_raw + tile_off);
    const uint4* pm = reinterpret_cast<const uint4*>(smem_raw + ctx.pm_off);   // [91] {certainly below, possibly below, possibly above, certainly above}
    pem::Record* rec = ctx.rec;
    const unsigned cap = ctx.cap;
    uint8_t* row_certain = PM ? ctx.row_certain + first : nullptr;
    uint8_t* row_uncertain = PM ? ctx.row_uncertain + first : nullptr;
    unsigned bits = 0;           // bit 16 slot + s: value s of the slot's angle lies inside a bracket
    unsigned row_c = 0, row_u = 0;   // lane s: values of row s outside for certain / uncertain
    static_assert(S <= 16, "one bit per sample and slot");
    // Two slots: angles 0..63, one row per wave instruction (lane = angle), and angles 64..90, TWO rows per instruction in full
    // tiles (lanes 0..26 and 32..58: 24 instructions' worth of values per round instead of 32).
    // (Rolled loops on purpose: fully unrolled, the scheduler hoisted every read of the round and the function took 248 registers,
    // or turned every borrow into a 0 / 1 register.  Comparisons are kept as wave masks -- v_cmp into a scalar pair, s_or, and back
    // as a lane condition: written with plain bools every one of them was materialised, 37 instructions per value instead of 19.)
#pragma unroll
    for (int slot = 0; slot < 2; ++slot) {
        const int half = (FULL && slot == 1) ? lane >> 5 : 0;      // which of the instruction's two rows this lane looks at
        const int sub = slot == 1 ? (lane & 31) : lane;
        const int col = 64 * slot + sub;
        const bool on = slot == 0 || (sub < NANG - 64 && (FULL || lane < 32));
        const int cc = on ? col : NANG - 1;           // idle lanes of the second slot repeat the last angle and keep nothing
        uint2 tb[NQ];
        unsigned nb[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            tb[q] = tab[cc * NQ + q];
            nb[q] = 0;
        }
        const int* hw = reinterpret_cast<const int*>(tile) + 2 * cc + 1 + half * 2 * NANG;   // the high words of this lane's values
        uint4 th = make_uint4(0u, 0u, 0u, 0u);
        if constexpr (PM) th = pm[cc];
        constexpr unsigned long long PART = (1ull << (NANG - 64)) - 1;
        const unsigned long long lanes_on = slot == 0 ? ~0ull : (FULL ? (PART | (PART << 32)) : PART);
        unsigned mine = 0;
        // one value per lane: the brackets' below-counts and "inside any" (then `bit` is noted); the premask's two wave masks
        auto one = [&](int row, unsigned bit, unsigned long long& certain, unsigned long long& maybe) {
            const unsigned kh = pem::order_key_high(hw[row * 2 * NANG]);
            unsigned long long in = 0;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                unsigned t;
                nb[q] += __builtin_sub_overflow(kh, tb[q].x, &t) ? 1u : 0u;
                in |= __builtin_amdgcn_uicmp(t, tb[q].y, 37 /* ICMP_ULE */);   // (a borrow leaves t above every `words`)
            }
            mine |= __builtin_amdgcn_inverse_ballot_w64(in) ? bit : 0u;
            if constexpr (PM) {
                certain = (__builtin_amdgcn_uicmp(kh, th.x, 36 /* ULT */) | __builtin_amdgcn_uicmp(kh, th.w, 34 /* UGT */)) & lanes_on;
                maybe = (__builtin_amdgcn_uicmp(kh, th.y, 37 /* ULE */) | __builtin_amdgcn_uicmp(kh, th.z, 35 /* UGE */)) & lanes_on & ~certain;
            }
        };
        if constexpr (FULL) {
            // four rows a turn (explicit groups: the wave-level builtins keep the compiler from unrolling a counted loop with a
            // remainder).  The premask's counts of the four rows -- scalars, at most 64 + 27 each over the two slots -- are packed
            // into one word and kept by lane `turn`: two vector instructions per four rows instead of six per row.
            static_assert(S % 4 == 0, "rows in groups of four");
            const unsigned bit0 = 1u << (16 * slot + half);
#pragma unroll 1
            for (int turn = 0; turn < S / 4; ++turn) {
                unsigned pc = 0, pu = 0;
                if (slot == 0) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        unsigned long long certain = 0, maybe = 0;
                        one(4 * turn + u, bit0 << (4 * turn + u), certain, maybe);
                        if constexpr (PM) {
                            pc |= (unsigned)__popcll(certain) << (8 * u);
                            pu |= (unsigned)__popcll(maybe) << (8 * u);
                        }
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < 2; ++u) {              // rows 4 turn + 2 u (lanes 0..31) and 4 turn + 2 u + 1 (lanes 32..63)
                        unsigned long long certain = 0, maybe = 0;
                        one(4 * turn + 2 * u, bit0 << (4 * turn + 2 * u), certain, maybe);
                        if constexpr (PM) {
                            pc |= ((unsigned)__popc((unsigned)certain) << (16 * u)) | ((unsigned)__popc((unsigned)(certain >> 32)) << (16 * u + 8));
                            pu |= ((unsigned)__popc((unsigned)maybe) << (16 * u)) | ((unsigned)__popc((unsigned)(maybe >> 32)) << (16 * u + 8));
                        }
                    }
                }
                if constexpr (PM) {
                    row_c += lane == turn ? pc : 0u;
                    row_u += lane == turn ? pu : 0u;
                }
            }
        } else {
            for (int r = 0; r < rows; ++r) {          // the ragged last tile of a launch: row by row, one byte per lane
                unsigned long long certain = 0, maybe = 0;
                one(r, 1u << (16 * slot + r), certain, maybe);
                if constexpr (PM) {
                    row_c += lane == r ? (unsigned)__popcll(certain) : 0u;
                    row_u += lane == r ? (unsigned)__popcll(maybe) : 0u;
                }
            }
        }
        bits |= on ? mine : 0u;
        if (on) {
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (nb[q]) atomicAdd(&below[q * NANG + col], nb[q]);
        }
    }
    if constexpr (PM) {
        if constexpr (FULL) {                          // lane `turn` holds the bytes of rows 4 turn .. 4 turn + 3
            if (lane < S / 4) {
                reinterpret_cast<unsigned*>(row_certain)[lane] = row_c;
                reinterpret_cast<unsigned*>(row_uncertain)[lane] = row_u;
            }
        } else if (lane < rows) {
            row_certain[lane] = (uint8_t)row_c;
            row_uncertain[lane] = (uint8_t)row_u;
        }
    }
    // The records: {key, angle} (which of the angle's brackets holds the key is found again by the passes over the records: they
    // see 4 % of the values).  Two per lane and turn -- the reads of the tile, and the stores, of both are in flight together --
    // appended behind the wave's count by however many lanes have one.
    while (__ballot(bits != 0)) {
        const bool has0 = bits != 0;
        const int b0 = has0 ? __builtin_ctz(bits) : 0;
        bits &= bits - 1;                              // (0 stays 0)
        const bool has1 = bits != 0;
        const int b1 = has1 ? __builtin_ctz(bits) : 0;
        bits &= bits - 1;
        const int col0 = (b0 >> 4) ? 64 + (lane & 31) : lane, col1 = (b1 >> 4) ? 64 + (lane & 31) : lane;
        const double x0 = tile[(b0 & 15) * NANG + (has0 ? col0 : 0)], x1 = tile[(b1 & 15) * NANG + (has1 ? col1 : 0)];
        const unsigned long long e0 = __ballot(has0), e1 = __ballot(has1);
        const unsigned at0 = cnt + __builtin_amdgcn_mbcnt_hi((unsigned)(e0 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)e0, 0u));
        const unsigned n0 = (unsigned)__popcll(e0);
        const unsigned at1 = cnt + n0 + __builtin_amdgcn_mbcnt_hi((unsigned)(e1 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)e1, 0u));
        if (has0 && at0 < cap) {
            f64x2 r;
            r.x = __longlong_as_double((long long)pem::order_key(x0));
            r.y = __longlong_as_double((long long)col0);
            *reinterpret_cast<f64x2*>(rec + at0) = r;
        }
        if (has1 && at1 < cap) {
            f64x2 r;
            r.x = __longlong_as_double((long long)pem::order_key(x1));
            r.y = __longlong_as_double((long long)col1);
            *reinterpret_cast<f64x2*>(rec + at1) = r;
        }
        cnt += n0 + (unsigned)__popcll(e1);
    }
    return cnt;
}

// Fused likelihood modes (JMODE 3 / 6): lane c's share -- records c, c+L, ... -- of the n_rec j_ion records {weight, y, 1/std, k}
// of one sample against its staged profile row; the L chunk lanes of the sample are summed by the caller.
// RADII (JMODE 8 / 9): `row` holds the shape g and the record's fourth word k | (ridx << 8); the model value is
// base(r) g + j_cex(r) with the pair {base, j_cex} of radius ridx (clamped into the sample's n_radii pairs).
template <bool RADII>
__device__ __forceinline__ double jion_model(const double4& e, double lo_v, double hi_v, const double2* pairs, int n_radii) {
    const double v = fma(e.x, hi_v - lo_v, lo_v);
    if constexpr (RADII) {
        const double2 p = pairs[min((int)((__double_as_longlong(e.w) >> 8) & 0xff), n_radii - 1)];
        return fma(p.x, v, p.y);
    } else {
        return v;
    }
}

template <int L, typename JT, bool RADII = false>
__device__ __forceinline__ double jion_records_sum(const double4* mt, int n_rec, const JT* row, int c, const double2* pairs = nullptr,
                                                   int n_radii = 0) {
    double acc = 0.0;
    constexpr int MU = PEM_LOGLIK_MU;   // records in flight per lane: the k -> row[k] chain is two LDS latencies deep
    for (int a0 = c; a0 < n_rec; a0 += MU * L) {
        double4 e[MU];
        double lo_v[MU], hi_v[MU];
#pragma unroll
        for (int u = 0; u < MU; ++u) e[u] = mt[a0 + u * L < n_rec ? a0 + u * L : a0];
#pragma unroll
        for (int u = 0; u < MU; ++u) {
            const int k = __double_as_longlong(e[u].w) & 0x7f;
            lo_v[u] = row[k];
            hi_v[u] = row[k + 1];
        }
#pragma unroll
        for (int u = 0; u < MU; ++u) {
            const double model = jion_model<RADII>(e[u], lo_v[u], hi_v[u], pairs, n_radii);
            const double z = (e[u].y - model) * e[u].z;
            if (a0 + u * L < n_rec) acc = fma(-0.5 * z, z, acc);
        }
    }
    return acc;
}

// JMODE 7: lane c's share of the j_ion records of one sample, the model values JMODE 6 compares, stored to out[record]
template <int L, typename JT, bool RADII = false>
__device__ __forceinline__ void jion_records_store(const double4* mt, int n_rec, const JT* row, int c, double* out,
                                                   const double2* pairs = nullptr, int n_radii = 0) {
    constexpr int MU = PEM_LOGLIK_MU;
    for (int a0 = c; a0 < n_rec; a0 += MU * L) {
        double4 e[MU];
        double lo_v[MU], hi_v[MU];
#pragma unroll
        for (int u = 0; u < MU; ++u) e[u] = mt[a0 + u * L < n_rec ? a0 + u * L : a0];
#pragma unroll
        for (int u = 0; u < MU; ++u) {
            const int k = __double_as_longlong(e[u].w) & 0x7f;
            lo_v[u] = row[k];
            hi_v[u] = row[k + 1];
        }
#pragma unroll
        for (int u = 0; u < MU; ++u)
            if (a0 + u * L < n_rec) out[a0 + u * L] = jion_model<RADII>(e[u], lo_v[u], hi_v[u], pairs, n_radii);
    }
}

// JMODE 7: the first record of sample t * 64 + j in pred, u = (t * 64) % n_cond + j: row (t * 64 + j) / n_cond
__device__ __forceinline__ double* pred_row(const WaveLds& m, long long t, unsigned u, int n_cond) {
    return m.pred + ((t * WAVE) / n_cond + (long long)(u / (unsigned)n_cond)) * m.ld_pred;
}


// JMODE 6 epilogue, one lane per sample: the V_cc, thrust and u_ion records of condition `cond` added to `ll` (the sample's j_ion
// sum).  A kind without records adds nothing -- whatever that part of the model is (a NaN v_exh of V_cc > V_a included).
__device__ __forceinline__ double system_epilogue_sum(double ll, const WaveLds& m, unsigned cond, double V_cc,
                                                      double thrust, double v_exh) {
    const double4* rec = reinterpret_cast<const double4*>(m.meas);
    const int2* sp = m.span + 4 * cond;
    const int2 rv = sp[PEM_SYS_VCC], rt = sp[PEM_SYS_T], ru = sp[PEM_SYS_UION];
    for (int i = rv.x; i < rv.x + rv.y; ++i) {   // the clipped cathode coupling voltage
        const double z = (rec[i].y - V_cc) * rec[i].z;
        ll = fma(-0.5 * z, z, ll);
    }
    for (int i = rt.x; i < rt.x + rt.y; ++i) {   // the thruster's thrust T (not the plume's T_c)
        const double z = (rec[i].y - thrust) * rec[i].z;
        ll = fma(-0.5 * z, z, ll);
    }
    const unsigned pmax = (unsigned)(m.n_unode < 2 ? 0 : m.n_unode - 2);
    for (int i = ru.x; i < ru.x + ru.y; ++i) {   // u_ion at nodes p, p+1 of the record, interpolated linearly (np.interp)
        const double4 e = rec[i];
        const unsigned p = min((unsigned)__double_as_longlong(e.w), pmax);
        const double u0 = v_exh / m.unode[p], u1 = v_exh / m.unode[p + 1];
        const double z = (e.y - fma(e.x, u1 - u0, u0)) * e.z;
        ll = fma(-0.5 * z, z, ll);
    }
    return ll;
}

// JMODE 7 epilogue, one lane per sample: the model values system_epilogue_sum compares, stored to out[record]
__device__ __forceinline__ void system_epilogue_store(const WaveLds& m, unsigned cond, double V_cc, double thrust, double v_exh,
                                                      double* out) {
    const double4* rec = reinterpret_cast<const double4*>(m.meas);
    const int2* sp = m.span + 4 * cond;
    const int2 rv = sp[PEM_SYS_VCC], rt = sp[PEM_SYS_T], ru = sp[PEM_SYS_UION];
    for (int i = rv.x; i < rv.x + rv.y; ++i) out[i] = V_cc;
    for (int i = rt.x; i < rt.x + rt.y; ++i) out[i] = thrust;
    const unsigned pmax = (unsigned)(m.n_unode < 2 ? 0 : m.n_unode - 2);
    for (int i = ru.x; i < ru.x + ru.y; ++i) {
        const double4 e = rec[i];
        const unsigned p = min((unsigned)__double_as_longlong(e.w), pmax);
        const double u0 = v_exh / m.unode[p], u1 = v_exh / m.unode[p + 1];
        out[i] = fma(e.x, u1 - u0, u0);
    }
}

// One 64-sample tile.  FULL = every sample of the tile exists (the steady state of the persistent loop:
// no bounds checks and a fixed number of stores, so the compiler can count them); FULL = false is the
// ragged last tile of a batch.
template <int L, bool COUPLED, int JMODE, bool FULL, int NQ = 0, bool PM = false, class QC = NoCount>
__device__ __forceinline__ void process_tile(const PlumeIO& io, const CoupledIO& cio, const WaveLds& m,
                                             const SampleIn<COUPLED>& in, long long t, int lane, double rad,
                                             double inv_r2, double inv_2pi_r2, QC& qc) {
    constexpr int S = WAVE / L;             // samples per round
    constexpr int CH = (NANG + L - 1) / L;  // angles per lane
    constexpr int TILE = S * NANG;          // profile values per round tile
    constexpr bool WRITE_J = JMODE != 0;
    constexpr bool RADII = JMODE == 8 || JMODE == 9;   // several sweep radii: the tile holds the shape g, the radii come in as pairs
    constexpr bool PREDICT = JMODE == 7 || JMODE == 9;
    using JT = typename std::conditional<JMODE == 2, float, double>::type;   // element type of the stored profile
    constexpr int PER16 = 16 / (int)sizeof(JT);                              // values per 16-byte piece
    constexpr int PAIRS = TILE / PER16;     // 16-byte pieces of a full round tile (TILE divides evenly)
    static_assert(TILE % PER16 == 0, "a round tile is a whole number of 16-byte pieces");
    const int s = lane % S, c = lane / S;   // role during the rounds
    const int k0 = c * CH;
    const double2* my_w = m.simpson + k0;   // this lane's folded Simpson weights
    double* params = m.params;
    JT* tile = reinterpret_cast<JT*>(m.tile);
    const long long g = t * WAVE + lane;
    const bool live = FULL || g < io.n;

    // ------------------------------ PRELUDE: one lane per sample ------------------------------
    double I_B0, thrust = 0.0, V_cc = 0.0, v_exh = 0.0;
    bool have_T;
    if constexpr (COUPLED) {
        V_cc = cathode_vcc(in.P_b, in.x0, in.x1, in.x2, in.x3, in.x4, io.torr2pa);
        const ThrusterQoI th = thruster_stage(in.x0, V_cc, in.x5, in.x6);
        I_B0 = th.I_B0;
        thrust = th.T;
        v_exh = th.v_exh;
        have_T = true;
    } else {
        I_B0 = in.x0;
        thrust = in.x1;
        have_T = io.T != nullptr;
    }
    // plume.py:40-61
    const PlumeSetup ps = plume_setup(in.P_b, in.c1, in.c2, in.c3, in.c4, in.c5, io.torr2pa);
    const double n_neutral = ps.n_neutral, a1 = ps.a1, a2 = ps.a2;
    const double u1 = 1.0 / (a1 * a1), u2 = 1.0 / (a2 * a2);
    const double A1 = (1.0 - in.c0) / normaliser(a1, u1, m.poly);  // plume.py:64-73
    const double A2 = in.c0 / normaliser(a2, u2, m.poly);          // plume.py:75-85
    // plume.py:95-100 at the single radius (several radii: the rounds form the pairs {base(r), j_cex(r)}; the loop below runs on
    // the amplitudes A1, A2 alone)
    double j_cex = 0.0, base = 1.0;
    if constexpr (!RADII) {
        const double decay = exp(-rad * n_neutral * in.sigma);
        j_cex = I_B0 * (1.0 - decay) * inv_2pi_r2;
        base = I_B0 * decay * inv_r2;
    }
    const unsigned long long a1_nonpos = __ballot(a1 <= 0.0);  // plume.py:105, first term
    unsigned long long inv_mask = 0;
    double den = 0.0, num = 0.0;
    // Reduced-QoI mode: nothing needs the 91 profile values themselves.  The two Simpson sums are linear in the beam
    // amplitudes and depend on each beam only through its width -> two table look-ups per beam (simpson_functionals).
    // What the loop would still decide is plume.py:105's `any(j_ion <= 0)`; with both amplitudes >= 0 and j_cex > 0 every
    // j_ion[k] >= j_cex > 0, so the flag is `alpha1 <= 0` alone.  Such a "plain" sample takes its sums from the tables,
    // any other one (NaN or denormal amplitudes, negative c0 or 1 - c0, beams narrower than QA_MIN) from the loop: a sample's result
    // depends on that sample alone, however batches and shards cut the design.  The loop is skipped -- a wave-uniform
    // branch -- when all 64 samples of the tile are plain, which under the PEM-v0 priors is every tile.
    bool plain = false, table_tile = false;
    if constexpr (JMODE == 0) {
        // (amplitudes in the denormal range are left to the loop as well: there every w_k f_k underflows to zero and the
        // reference's 0/0 = NaN must come out, where the tabulated sum would still see a few bits)
        const double X1a = base * A1, X2a = base * A2;
        plain = fabs(a1) >= PEM_QA_MIN && fabs(a2) >= PEM_QA_MIN && X1a >= 0.0 && X2a >= 0.0 && j_cex > 0.0 &&
                (fmax(X1a, X2a) >= 1e-280 || (X1a == 0.0 && X2a == 0.0));
        table_tile = __all(plain);
        if (table_tile) inv_mask = a1_nonpos;
    }
    if (!table_tile) {
        // Gaussian recurrences: e_k = exp(-k^2 s), s = (h/a)^2; chunk starts at k = c*CH
        const double s1 = (GRID_H * GRID_H) * u1, s2 = (GRID_H * GRID_H) * u2;
        // a1 == 0: exp(-(0/0)^2) is NaN in the reference; the amplitudes carry it (A1 is NaN there)
        params[0 * WAVE + lane] = base * A1;
        params[1 * WAVE + lane] = base * A2;
        params[2 * WAVE + lane] = j_cex;
        params[3 * WAVE + lane] = exp_nonpos(-s1);
        params[4 * WAVE + lane] = exp_nonpos(-(2.0 * CH) * s1);
        params[5 * WAVE + lane] = exp_nonpos(-(double)(CH * CH) * s1);
        params[6 * WAVE + lane] = exp_nonpos(-s2);
        params[7 * WAVE + lane] = exp_nonpos(-(2.0 * CH) * s2);
        params[8 * WAVE + lane] = exp_nonpos(-(double)(CH * CH) * s2);
        wave_lds_sync();

        // ------------------------------ ROUNDS: L lanes per sample ------------------------------
        // (the counting modes keep the rounds rolled: unrolled four times with count_round inside, the kernel took 340 registers
        // and one wave per SIMD)
        // (the reduced-QoI mode takes this loop for the tiles that hold a sample the tables do not cover -- none under the priors:
        // rolled, with a rolled angle loop, it fits the three waves per SIMD that mode is compiled for; unrolled it spilled there)
        constexpr int ROUND_UNROLL = (NQ > 0 || JMODE == 0) ? 1 : L;
        constexpr int ANGLE_UNROLL = JMODE == 0 ? 1 : CH;
#pragma unroll ROUND_UNROLL
        for (int round = 0; round < L; ++round) {
            const int smp = round * S + s;
            double X1 = params[0 * WAVE + smp], X2 = params[1 * WAVE + smp];
            const double jcex = params[2 * WAVE + smp];
            const double r01 = params[3 * WAVE + smp], G1 = params[4 * WAVE + smp], E1 = params[5 * WAVE + smp];
            const double r02 = params[6 * WAVE + smp], G2 = params[7 * WAVE + smp], E2 = params[8 * WAVE + smp];
            // coarse recurrence to this lane's first angle k0 = c*CH:
            //   e_{k0} = E^(c^2), r_{k0} = exp(-(2 k0 + 1) s) = r0 * G^c
            double rr1 = r01, rr2 = r02, rho1 = E1, rho2 = E2;
            const double E1sq = E1 * E1, E2sq = E2 * E2;
#pragma unroll
            for (int i = 0; i < L - 1; ++i) {
                if (i < c) {
                    X1 *= rho1;
                    rho1 *= E1sq;
                    rr1 *= G1;
                    X2 *= rho2;
                    rho2 *= E2sq;
                    rr2 *= G2;
                }
            }
            const double q1 = r01 * r01, q2 = r02 * r02;
            double den = 0.0, num = 0.0, lo = __builtin_inf();   // this lane's chunk of the round (shadows the tile sums)
            double2* pairs = nullptr;
            if constexpr (RADII) {
                // plume.py:95-98 at every radius, one exp per (sample, radius): lane (s, c) takes radii c, c + L of its sample
                pairs = m.pairs + s * m.n_radii;
                const double nn = __shfl(n_neutral, smp), sg = __shfl(in.sigma, smp), ib = __shfl(I_B0, smp);
                for (int r = c; r < m.n_radii; r += L) {
                    const double decay = exp(-m.rtab[3 * r] * nn * sg);
                    pairs[r] = make_double2(ib * decay * m.rtab[3 * r + 1], ib * (1.0 - decay) * m.rtab[3 * r + 2]);
                }
            }
            // The weight reads are issued PF iterations ahead IN SOURCE ORDER: the tile stores in between are
            // LDS stores the compiler must assume may alias the table, so it cannot hoist the reads itself.
            constexpr int PF = 6;
            double2 wq[CH];
#pragma unroll
            for (int j = 0; WRITE_J && j < PF && j < CH; ++j) wq[j] = my_w[j];
#pragma unroll ANGLE_UNROLL
            for (int j = 0; j < CH; ++j) {
                double2 wj;
                if constexpr (!WRITE_J) {
                    wj = my_w[j];                          // no tile stores in between: the compiler schedules the reads
                } else {
                    if (j + PF < CH) wq[j + PF] = my_w[j + PF];
                    wj = wq[j];
                }
                const double f = X1 + X2;     // j_beam + j_scat
                const double ji = f + jcex;   // plume.py:102
                if ((L - 1) * CH + j < NANG) {  // an angle every chunk has (compile-time after unrolling)
                    if constexpr (WRITE_J) tile[s * NANG + k0 + j] = (JT)ji;
                    lo = fmin(lo, WRITE_J ? ji : f);
                } else {                        // past 90 degrees in the last chunk: store to the sink, skip the min
                    const bool in_range = k0 + j < NANG;
                    if constexpr (WRITE_J) tile[in_range ? s * NANG + k0 + j : TILE] = (JT)ji;
                    lo = fmin(lo, in_range ? (WRITE_J ? ji : f) : __builtin_inf());
                }
                den = fma(wj.x, f, den);
                num = fma(wj.y, f, num);
                X1 *= rr1;
                rr1 *= q1;
                X2 *= rr2;
                rr2 *= q2;
            }
            {
                // deep-underflow or non-positive chunk: the literal evaluation decides (see exact_chunk); rare, and the
                // branch is wave-uniform so that the shuffles inside are executed by every lane
                // (an infinite amplitude -- exp(+x) overflow for a negative density -- must turn into NaN where the
                // reference's exp() is exactly zero.  A class test, not `X - X != 0`: hipcc contracts that with the
                // multiply before it into fma(X', rr, -X), the rounding error of the product, which is never zero.)
                const bool uncertain = (WRITE_J ? lo : lo + jcex) < 1e-290 || !__builtin_isfinite(X1) || !__builtin_isfinite(X2);
                if (__ballot(uncertain)) {
                    const double a1s = __shfl(a1, smp), a2s = __shfl(a2, smp);
                    if (uncertain) {
                        const double X1a = params[0 * WAVE + smp], X2a = params[1 * WAVE + smp];
                        const ChunkSums ex = exact_chunk<JT, WRITE_J>(X1a, X2a, jcex, a1s, a2s, k0, CH, my_w, tile + s * NANG + k0);
                        den = ex.den;
                        num = ex.num;
                        lo = ex.lo;
                    }
                }
            }
            if constexpr (RADII) {
                // div_angle and T_c are those of the last radius: its Simpson sums are the shape's scaled by base(r_last) -- a
                // vanished beam (base = 0) still gives the reference's 0 / 0
                wave_lds_sync();
                const double bl = pairs[m.n_radii - 1].x;
                den *= bl;
                num *= bl;
            }
            // this round has read its nine parameter rows of sample `smp`: rows 2c, 2c+1 now carry the partial sums
            params[(2 * c) * WAVE + smp] = den;
            params[(2 * c + 1) * WAVE + smp] = num;
            // plume.py:105: invalid if alpha1 <= 0 or any j_ion <= 0 (NaN compares false).  Without a stored profile
            // the minimum runs over f and j_cex is added once: rounding is monotonic, min_k fl(f_k + c) = fl(min_k f_k + c).
            unsigned long long bad;
            if constexpr (RADII) {
                // any j_ion(r, alpha_k) <= 0 at ANY radius: with base > 0 the smallest value of a radius is base min_k g + j_cex
                // (rounding is monotonic); any other pair -- never under the priors -- is decided value by value
                bool any = false;
                for (int r = 0; r < m.n_radii; ++r) {
                    const double2 p = pairs[r];
                    if (p.x > 0.0 && __builtin_isfinite(p.x) && __builtin_isfinite(p.y)) {
                        any = any || fma(p.x, lo, p.y) <= 0.0;
                    } else {
                        for (int j = 0; j < CH; ++j)
                            if (k0 + j < NANG) any = any || fma(p.x, (double)tile[s * NANG + k0 + j], p.y) <= 0.0;
                    }
                }
                bad = __ballot(any);
            } else {
                bad = __ballot((WRITE_J ? lo : lo + jcex) <= 0.0);
            }
#pragma unroll
            for (int sh = S; sh < WAVE; sh <<= 1) bad |= bad >> sh;   // fold the L chunk lanes of a sample onto bit s
            bad = (bad | (a1_nonpos >> (round * S))) & ((S == 64) ? ~0ull : ((1ull << S) - 1));
            inv_mask |= bad << (round * S);
            if constexpr (WRITE_J) {
                if ((bad >> s) & 1) {  // plume.py:106: the whole profile of an invalid sample becomes 1e-20 (rare)
                    const JT fill = RADII ? (JT)0.0 : (JT)1e-20;   // (several radii: 0 g + 1e-20 at every radius)
                    for (int j = 0; j < CH; ++j)
                        if (k0 + j < NANG) tile[s * NANG + k0 + j] = fill;
                    if constexpr (RADII) {   // (program order: every lane of the sample has read its pairs above)
                        for (int r = c; r < m.n_radii; r += L) pairs[r] = make_double2(0.0, 1e-20);
                    }
                }
                wave_lds_sync();
                const long long first = t * WAVE + (long long)round * S;
                if constexpr (JMODE == 3 || JMODE == 6 || JMODE == 7 || RADII) {
                    static_assert(2 * L < param_rows<L>(), "row 2L of `params` carries the likelihood sum");
                    // measured current densities against the staged profile: lane (s, c) takes measurements c, c+L, ...
                    // of its sample's condition (sample index mod n_cond); the sample's sum goes to row 2L of `params`
                    const unsigned cond = ((unsigned)((t * WAVE) % io.n_cond) + (unsigned)(round * S + s)) % (unsigned)io.n_cond;
                    const JT* row = tile + s * NANG;
                    if constexpr (PREDICT) {   // the values themselves, to the sample's row of pred
                        const int2 sp = m.span[4 * cond + PEM_SYS_JION];
                        if (FULL || first + s < io.n) {
                            const unsigned u = (unsigned)((t * WAVE) % io.n_cond) + (unsigned)(round * S + s);
                            jion_records_store<L, JT, RADII>(reinterpret_cast<const double4*>(m.meas) + sp.x, sp.y, row, c,
                                                             pred_row(m, t, u, io.n_cond) + sp.x, pairs, m.n_radii);
                        }
                        wave_lds_sync();
                        continue;
                    }
                    double acc;
                    if constexpr (JMODE == 3) {
                        const double4* mt = reinterpret_cast<const double4*>(m.meas) + cond * (io.n_ang | 1);   // {weight, y, 1/std, k}
                        acc = jion_records_sum<L>(mt, io.n_ang, row, c);
                    } else {
                        const int2 sp = m.span[4 * cond + PEM_SYS_JION];
                        acc = jion_records_sum<L, JT, RADII>(reinterpret_cast<const double4*>(m.meas) + sp.x, sp.y, row, c, pairs, m.n_radii);
                    }
#pragma unroll
                    for (int sh = S; sh < WAVE; sh <<= 1) acc += __shfl_xor(acc, sh);   // the L chunk lanes of sample s
                    if (c == 0) params[(2 * L) * WAVE + smp] = acc;
                    wave_lds_sync();
                    continue;
                }
                if constexpr (JMODE == 5) {             // counted, never stored
                    const long long left = io.n - first;
                    qc.cnt = count_round<NQ, S, FULL, PM>(qc.ctx_off, m.tile_off, qc.cnt, lane,
                                                          FULL ? S : (int)(left < S ? (left < 0 ? 0 : left) : S), first);
                    wave_lds_sync();
                    continue;
                }
                // the round's S*91 values are one contiguous, 16-byte aligned block of j_ion
                JT* jbase;
                if constexpr (JMODE == 2) jbase = io.j_ion_f32; else jbase = io.j_ion;
                if constexpr (FULL) {
                    f64x2* dst2 = reinterpret_cast<f64x2*>(jbase + first * NANG);
                    const f64x2* srcv = reinterpret_cast<const f64x2*>(tile);
#pragma unroll
                    for (int it = 0; it < PAIRS / WAVE; ++it) stream_store(srcv[it * WAVE + lane], &dst2[it * WAVE + lane]);
                    if (PAIRS % WAVE != 0 && lane < PAIRS % WAVE)
                        stream_store(srcv[(PAIRS / WAVE) * WAVE + lane], &dst2[(PAIRS / WAVE) * WAVE + lane]);
                } else {
                    long long valid = (io.n - first) * NANG;   // values of this round that exist
                    if (valid > TILE) valid = TILE;
                    if (valid > 0) {
                        JT* dst = jbase + first * NANG;
                        f64x2* dst2 = reinterpret_cast<f64x2*>(dst);
                        const f64x2* srcv = reinterpret_cast<const f64x2*>(tile);
                        const int pieces = (int)(valid / PER16);
                        for (int i = lane; i < pieces; i += WAVE) dst2[i] = srcv[i];
                        const int rest = (int)(valid - (long long)pieces * PER16);
                        if (lane < rest) dst[pieces * PER16 + lane] = tile[pieces * PER16 + lane];
                    }
                }
                if constexpr (JMODE == 4) {             // the stores are on their way (their LDS reads are done): count the tile
                    const long long left = io.n - first;
                    qc.cnt = count_round<NQ, S, FULL, PM>(qc.ctx_off, m.tile_off, qc.cnt, lane,
                                                          FULL ? S : (int)(left < S ? (left < 0 ? 0 : left) : S), first);
                }
                wave_lds_sync();
            }
        }
        wave_lds_sync();
#pragma unroll
        for (int i = 0; i < L; ++i) {
            den += params[(2 * i) * WAVE + lane];
            num += params[(2 * i + 1) * WAVE + lane];
        }
    }   // !table_tile
    if constexpr (JMODE == 0) {   // after the loop, so that nothing of it stays live across the loop's 213 registers
        double d1, n1, d2, n2;
        simpson_functionals(m.qpoly, fabs(a1), u1, d1, n1);
        simpson_functionals(m.qpoly, fabs(a2), u2, d2, n2);
        den = plain ? fma(base * A1, d1, (base * A2) * d2) : den;
        num = plain ? fma(base * A1, n1, (base * A2) * n2) : num;
    }

    // ------------------------------ EPILOGUE: one lane per sample ------------------------------
    double cos_div = num / den;  // plume.py:124-127
    if (cos_div == __builtin_inf()) cos_div = __builtin_nan("");
    if constexpr (JMODE == 4 || JMODE == 5) {
        // A NaN in a column makes its percentiles NaN, and the counting above never looks for one: any non-finite f_k leaves the
        // Simpson sum non-finite (w_k f_k is NaN or infinite, and stays), a non-finite j_cex is seen directly -- such a sample
        // (never under the priors) is reported and the selection falls back to the passes that examine every value.
        if (live && (!__builtin_isfinite(den) || !__builtin_isfinite(j_cex))) atomicOr(io.q.flags + 1, 1);
    }
    if constexpr (JMODE == 3) {
        if (live) io.loglik[g] = params[(2 * L) * WAVE + lane];
    }
    if constexpr (JMODE == 6 || JMODE == 8) {
        if (live) {
            const unsigned cond = ((unsigned)((t * WAVE) % io.n_cond) + (unsigned)lane) % (unsigned)io.n_cond;
            io.loglik[g] = system_epilogue_sum(params[(2 * L) * WAVE + lane], m, cond, V_cc, thrust, v_exh);
        }
    }
    if constexpr (PREDICT) {
        if (live) {
            const unsigned u = (unsigned)((t * WAVE) % io.n_cond) + (unsigned)lane;
            system_epilogue_store(m, u % (unsigned)io.n_cond, V_cc, thrust, v_exh, pred_row(m, t, u, io.n_cond));
        }
    }
    if (live) {
        // (the record predictions take V_cc, div_angle and T_c as optional outputs)
        if (!PREDICT || io.div) io.div[g] = acos(cos_div);
        if (have_T && (!PREDICT || io.Tc)) io.Tc[g] = thrust * cos_div;
        if (io.invalid) io.invalid[g] = (uint8_t)((inv_mask >> lane) & 1);
        if constexpr (COUPLED) {
            if (!PREDICT || cio.V_cc) cio.V_cc[g] = V_cc;
            if (cio.I_B0) cio.I_B0[g] = I_B0;
            if (cio.T) cio.T[g] = thrust;
        }
    }
    wave_lds_sync();  // params are rewritten by the next tile
}

// Minimum waves per SIMD the register allocator must leave room for: 1 (the default for a 4-wave workgroup; every
// instantiation ends up at two anyway) except the fused Monte-Carlo reduced-QoI one, which is bound by Philox's
// quarter-rate 32x32 multiplies and gains a third wave (99 -> 86 us per 1.25e6 samples); unconstrained it takes 171
// registers, three more than three waves allow.
template <int JMODE, bool MC>
constexpr int min_waves_per_simd() { return (MC && JMODE == 0) ? 3 : 1; }

// Only the fused Monte-Carlo instantiations carry the ~340-byte design in their kernel arguments, and only the fused multi-QoI
// likelihood mode its measurement table.
struct NoDesign {};
template <bool MC, int JMODE = 0>
using DesignArg = typename std::conditional<
    MC, McDesign,
    typename std::conditional<JMODE == 6, SystemTable,
                              typename std::conditional<JMODE == 7, SystemPredict,
                                                        typename std::conditional<JMODE >= 8, SystemRadii, NoDesign>::type>::type>::type>::type;

// bytes of LDS the counting modes add per workgroup: brackets' {loh, words} [91][NQ] | below counters [NQ][91] | premask thresholds [91] x 16
template <int NQ, bool PM>
constexpr int count_lds_bytes() { return NANG * NQ * 8 + NQ * NANG * 4 + 8 + (PM ? NANG * 16 + 8 : 0) + WPB * (int)sizeof(CountCtx); }

template <int L, bool COUPLED, int JMODE, bool MC = false, int NQ = 0, bool PM = false>
__global__ __launch_bounds__(WAVE * WPB) __attribute__((amdgpu_waves_per_eu(min_waves_per_simd<JMODE, MC>())))
void plume_r1_kernel(PlumeIO io, CoupledIO cio, long long ntiles, DesignArg<MC, JMODE> mc) {
    static_assert(!MC || COUPLED, "the fused Monte-Carlo mode generates the coupled inputs");
    static_assert((JMODE == 4 || JMODE == 5) == (NQ > 0), "the counting modes, and only they, know their number of brackets");
    static_assert(NQ == 0 || L == 4, "count_round keeps one bit per sample of a 16-sample round");
    static_assert(L == 2 || L == 4 || L == 8, "lanes per sample");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* lds = reinterpret_cast<double*>(smem_raw);
    double2* tab_simpson = reinterpret_cast<double2*>(lds);          // [96] {cden, cnum}, zero past angle 90
    double* tab_poly = lds + 2 * NSIMP;                               // [32*12]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    WaveLds m;
    m.simpson = tab_simpson;
    m.poly = tab_poly;
    m.params = lds + TABLE_DOUBLES + wave * wave_lds_doubles<L, JMODE>();   // [rows][64], private to this wave
    m.tile = m.params + param_rows<L>() * WAVE;                               // [S*91] + sink
    m.tile_off = (unsigned)(reinterpret_cast<unsigned char*>(m.tile) - smem_raw);
    m.qpoly = nullptr;
    if constexpr (JMODE == 0) {   // Simpson-functional tables behind the per-wave regions
        double* q = lds + TABLE_DOUBLES + WPB * wave_lds_doubles<L, JMODE>();
        for (int i = tid; i < QPOLY_DOUBLES; i += WAVE * WPB) q[i] = PEM_QPOLY[i];
        m.qpoly = reinterpret_cast<const double2*>(q);
    }
    double* design = nullptr;
    if constexpr (MC) {   // the Monte-Carlo design behind everything else
        static_assert(!MC || JMODE == 0 || JMODE == 1 || JMODE == 4 || JMODE == 5, "the fused Monte-Carlo mode writes an fp64 profile or none");
        design = lds + TABLE_DOUBLES + WPB * wave_lds_doubles<L, JMODE>() + (JMODE == 0 ? QPOLY_DOUBLES : 0);
        if (tid < 15) {
            design[tid] = mc.a[tid];
            design[15 + tid] = mc.b[tid];
            reinterpret_cast<int*>(design + 32)[tid] = mc.kind[tid];
        }
    }
    m.meas = nullptr;
    if constexpr (JMODE == 3) {   // measurement tables behind the per-wave regions (vmcnt is in order: never global)
        double* meas = lds + TABLE_DOUBLES + WPB * wave_lds_doubles<L, JMODE>();
        const int nent = io.n_cond * io.n_ang;
        // one 32-byte record per measurement; an odd record stride per condition spreads the conditions over the banks
        for (int i = tid; i < nent; i += WAVE * WPB) {
            const int r = 4 * ((i / io.n_ang) * (io.n_ang | 1) + i % io.n_ang);
            meas[r] = io.m_wgt[i];
            meas[r + 1] = io.m_y[i];
            meas[r + 2] = io.m_inv_std[i];
            meas[r + 3] = __longlong_as_double((long long)io.m_kidx[i]);
        }
        m.meas = meas;
    }
    m.span = nullptr;
    m.unode = nullptr;
    m.n_unode = 0;
    m.pred = nullptr;
    m.ld_pred = 0;
    m.rtab = nullptr;
    m.pairs = nullptr;
    m.n_radii = 0;
    if constexpr (JMODE == 6 || JMODE == 7 || JMODE == 8 || JMODE == 9) {   // records | spans | u_ion denominators behind the per-wave regions (system_lds_bytes)
        double* meas = lds + TABLE_DOUBLES + WPB * wave_lds_doubles<L, JMODE>();
        for (int i = tid; i < 4 * mc.n_rec; i += WAVE * WPB) meas[i] = mc.rec[i];
        int2* span = reinterpret_cast<int2*>(meas + 4 * mc.n_rec);
        for (int i = tid; i < 4 * io.n_cond; i += WAVE * WPB) {   // clamped into the table: a span never reads past it
            const int first = min(max(mc.span[2 * i], 0), mc.n_rec);
            span[i] = make_int2(first, min(max(mc.span[2 * i + 1], 0), mc.n_rec - first));
        }
        double* unode = reinterpret_cast<double*>(span + 4 * io.n_cond);
        for (int i = tid; i < (mc.n_node > 2 ? mc.n_node : 2); i += WAVE * WPB)
            unode[i] = i < mc.n_node ? uion_den(uion_z(mc.z0, mc.z1, mc.ncells, min(max(mc.node[i], 0), mc.ncells - 1)))
                                     : __builtin_nan("");
        m.meas = meas;
        m.span = span;
        m.unode = unode;
        m.n_unode = mc.n_node;
        if constexpr (JMODE == 7 || JMODE == 9) {
            m.pred = mc.pred;
            m.ld_pred = mc.ld_pred;
        }
        if constexpr (JMODE == 8 || JMODE == 9) {   // behind them: the radii's constants | every wave's pairs of a round (radii_lds_bytes)
            const int nr = min(max(mc.n_radii, 1), SYS_RADII_MAX);
            double* rtab = unode + (((mc.n_node > 2 ? mc.n_node : 2) + 1) & ~1);
            if (tid < nr) {
                const double r = mc.radii[tid];
                rtab[3 * tid] = r;
                rtab[3 * tid + 1] = 1.0 / (r * r);
                rtab[3 * tid + 2] = 1.0 / (2.0 * PEM_PI * (r * r));
            }
            m.rtab = rtab;
            m.pairs = reinterpret_cast<double2*>(rtab + ((3 * nr + 1) & ~1)) + wave * (WAVE / L) * nr;
            m.n_radii = nr;
        }
    }

    using QC = typename std::conditional<(NQ > 0), QCount, NoCount>::type;
    QC qc;
    if constexpr (NQ > 0) {   // the brackets and the below counters behind everything else
        double* qbase = lds + TABLE_DOUBLES + WPB * wave_lds_doubles<L, JMODE>() + (MC ? MC_LDS_DOUBLES : 0);
        uint2* qtab = reinterpret_cast<uint2*>(qbase);
        unsigned* qbelow = reinterpret_cast<unsigned*>(qtab + NANG * NQ);
        for (int i = tid; i < NANG * NQ; i += WAVE * WPB) {
            // (a selection of fewer than NQ quantiles leaves the other brackets empty: loh = 2^32 - 1, no words)
            const int c = i / NQ, q = i - c * NQ;
            qtab[i] = q < io.q.nq ? make_uint2(io.q.br[c * io.q.nq + q].loh, io.q.br[c * io.q.nq + q].words) : make_uint2(0xffffffffu, 0u);
            qbelow[i] = 0;
        }
        const unsigned gw = blockIdx.x * WPB + wave;
        unsigned char* after = reinterpret_cast<unsigned char*>(qbelow + NQ * NANG);
        after = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(after) + 15) & ~uintptr_t(15));
        unsigned pm_off = 0;
        if constexpr (PM) {
            uint4* pmt = reinterpret_cast<uint4*>(after);
            for (int i = tid; i < NANG; i += WAVE * WPB) pmt[i] = io.q.premask[i];
            pm_off = (unsigned)(after - smem_raw);
            after += NANG * sizeof(uint4);
        }
        CountCtx* ctx = reinterpret_cast<CountCtx*>(after) + wave;
        if (lane == 0) {
            ctx->rec = io.q.rec + (size_t)gw * io.q.cap;
            ctx->row_certain = io.q.row_certain;
            ctx->row_uncertain = io.q.row_uncertain;
            ctx->cap = io.q.cap;
            ctx->tab_off = (unsigned)(reinterpret_cast<unsigned char*>(qtab) - smem_raw);
            ctx->below_off = (unsigned)(reinterpret_cast<unsigned char*>(qbelow) - smem_raw);
            ctx->pm_off = pm_off;
        }
        qc.ctx_off = (unsigned)(reinterpret_cast<unsigned char*>(ctx) - smem_raw);
        qc.below_off = (unsigned)(reinterpret_cast<unsigned char*>(qbelow) - smem_raw);
        qc.cap = io.q.cap;
        qc.cnt = 0;
    }
    for (int i = tid; i < NSIMP; i += WAVE * WPB)
        tab_simpson[i] = i < NANG ? make_double2(PEM_SIMPSON_CDEN[i], PEM_SIMPSON_CNUM[i]) : make_double2(0.0, 0.0);
    for (int i = tid; i < PEM_NDI * PEM_NDC; i += WAVE * WPB) tab_poly[i] = PEM_DPOLY[i];
    __syncthreads();   // the only workgroup barrier of the evaluation: from here on the waves are independent

    const double rad = io.radius;
    const double inv_r2 = 1.0 / (rad * rad);
    const double inv_2pi_r2 = 1.0 / (2.0 * PEM_PI * (rad * rad));

    // persistent loop over the tiles whose 64 samples all exist; inputs are prefetched one tile ahead
    const long long nfull = io.n / WAVE;
    // XCD-aware tile order.  Workgroups are dealt round-robin over the 8 XCDs (b and b + 8 share one), so with tile = workgroup
    // index every XCD writes every eighth 186-KB piece of j_ion; with the bijective remap below (cdna_hip_programming.md, "XCD
    // swizzle must be bijective") the workgroups that share an XCD take one CONTIGUOUS eighth of the tiles, and each XCD's L2 hands
    // the memory system one sequential stream instead of a comb.  There is no inter-workgroup reuse here -- the gain is in how the
    // writes arrive at HBM: 210 -> 204 us per 1.25e6-sample launch, 204 -> 195 us per step on two streams (interleaved A/B,
    // the same on four leases; a first box showed 202 -> 184: profiles/grid_modes_r03.txt).  The remap itself: pem_common.h.
    // Where it pays: the modes that write a profile (without one -- reduced QoIs, VALU-bound -- it measured 2 % slower: 48.4 against
    // 47.2 us), and one-shot grids only -- a persistent grid of a few rounds (312 512-sample pieces) ran at 249 against 215 us per
    // 1.25e6 samples with it.
    const bool one_tile_per_wave = (long long)gridDim.x * WPB >= ntiles;
    const long long vblock = ((JMODE == 1 || JMODE == 2) && one_tile_per_wave) ? (long long)pem::xcd_contiguous_block() : (long long)blockIdx.x;
    const long long me = vblock * WPB + wave, nwaves = (long long)gridDim.x * WPB;
    long long t = me;
    if constexpr (MC) {
        for (; t < nfull; t += nwaves) {
            const SampleIn<COUPLED> in = generate_sample(mc, design, t * WAVE + lane);
            process_tile<L, COUPLED, JMODE, true, NQ, PM>(io, cio, m, in, t, lane, rad, inv_r2, inv_2pi_r2, qc);
        }
        if (nfull < ntiles && (nfull % nwaves) == me) {
            const long long g = nfull * WAVE + lane;
            McDesign quiet = mc;
            if (g >= io.n) quiet.x_out = nullptr;       // dead lanes recompute the last sample and store nothing
            const SampleIn<COUPLED> in = generate_sample(quiet, design, g < io.n ? g : io.n - 1);
            process_tile<L, COUPLED, JMODE, false, NQ, PM>(io, cio, m, in, nfull, lane, rad, inv_r2, inv_2pi_r2, qc);
        }
    } else {
        if (t < nfull) {
            SampleIn<COUPLED> nxt = load_sample<COUPLED>(io, cio, t * WAVE + lane);
            for (; t < nfull; t += nwaves) {
                const SampleIn<COUPLED> in = nxt;
                if (t + nwaves < nfull) nxt = load_sample<COUPLED>(io, cio, (t + nwaves) * WAVE + lane);
                process_tile<L, COUPLED, JMODE, true, NQ, PM>(io, cio, m, in, t, lane, rad, inv_r2, inv_2pi_r2, qc);
            }
        }
        // the ragged last tile (n % 64 samples) goes to the wave that would have been next in line for it
        if (nfull < ntiles && (nfull % nwaves) == me) {
            const long long g = nfull * WAVE + lane;
            const SampleIn<COUPLED> in = load_sample<COUPLED>(io, cio, g < io.n ? g : io.n - 1);
            process_tile<L, COUPLED, JMODE, false, NQ, PM>(io, cio, m, in, nfull, lane, rad, inv_r2, inv_2pi_r2, qc);
        }
    }
    if constexpr (NQ > 0) {
        // every wave reaches this barrier (no path above returns): the workgroup's counters are complete, one atomic each
        if (lane == 0) {
            io.q.rec_count[blockIdx.x * WPB + wave] = qc.cnt;
            if (qc.cnt > qc.cap) atomicOr(io.q.flags, 1);
        }
        __syncthreads();
        for (int i = tid; i < NQ * NANG; i += WAVE * WPB) {
            const int q = i / NANG, c = i - q * NANG;
            const unsigned v = reinterpret_cast<const unsigned*>(smem_raw + qc.below_off)[i];
            if (v && q < io.q.nq) atomicAdd(&io.q.below[c * io.q.nq + q], (unsigned long long)v);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
std::atomic<int> g_lanes{4};
double g_angle_grid[NANG];
std::once_flag g_grid_once;

// persistent grid of the fast kernel: workgroups of WPB waves, `per_cu` of them resident on every CU (balanced rounds:
// balanced_grid, csrc/pem_common.h)
// The grid of the R = 1 kernel, apart from the device query so that the host side can plan range launches with it
// (pem_persistent_grid).  Two regimes for the HBM-bound modes (profile written), measured interleaved on one box in the
// streaming regime (tools/grid_mode_ab.py, tools/launch_size_probe.py --walk; profiles/grid_modes_r03.txt):
//   * more than ONE_SHOT_ROUNDS rounds of work: a ONE-SHOT grid, one tile per wave, every workgroup handed to whichever CU has
//     room.  With the static walk (tile me, me + nwaves, ...) the launch ends when the slowest wave has done its share while
//     the others idle -- a tile's duration depends on where its wave sits; the dispatcher deals tiles out as slots free up
//     instead: 206-208 against 214-219 us for the 1.25e6-sample shard (9.5 rounds), 213-215 against 222-226 for half of it.
//     (A tile counter drawn from with atomics inside a persistent loop cost 36 registers, one wave per SIMD, 265 us; removed.)
//   * fewer rounds: the persistent loop with balanced rounds -- the next tile's inputs are in flight while a tile is worked on
//     and the tables are loaded once per wave, which is worth more than the dealing when a wave sees two or three tiles
//     (312 512 samples, 2.4 rounds: 214-217 against 224-225 us per 1.25e6).
constexpr long long ONE_SHOT_ROUNDS = 3;
long long persistent_grid(long long ntiles, long long cus, long long per_cu, bool memory_bound) {
    if (per_cu < 1) per_cu = 1;
    long long g = cus * per_cu;
    const long long need = (ntiles + WPB - 1) / WPB;
    if (g > need) g = need;
    if (!memory_bound) return g;
    // (the modes bound by instruction issue want every slot: balanced, the reduced-QoI launch takes 45.3 instead of 44.4 us and
    // the fused Monte-Carlo one 88 instead of 82 us; tools/grid_ab_probe.py)
    if (need > ONE_SHOT_ROUNDS * g) return need;
    return (long long)balanced_grid((size_t)need, (size_t)g);
}

int fast_grid(long long per_cu, long long ntiles, bool memory_bound, unsigned* grid) {
    int cus = 0;
    HIP_TRY(pem::device_cus(&cus));
    if (const char* e = getenv("PEM_WAVES_PER_CU")) {          // tuning/experiments only
        const long long v = atoll(e) / WPB;
        if (v >= 1 && v < per_cu) per_cu = v;
    }
    *grid = (unsigned)persistent_grid(ntiles, cus, per_cu, memory_bound);
    if (const char* e = getenv("PEM_GRID_MULT")) {             // experiments: a grid of m x the resident slots (0 = one tile per wave)
        const long long m = atoll(e), need = (ntiles + WPB - 1) / WPB, cap = (long long)cus * (per_cu < 1 ? 1 : per_cu);
        *grid = (unsigned)((m <= 0 || m * cap > need) ? need : m * cap);
    }
    return PEM_OK;
}

// JMODE 6's table in LDS: records [n_rec][4] doubles | spans [n_cond][4] int2 | u_ion denominators [max(n_node, 2)] doubles
size_t system_lds_bytes(int n_cond, const SystemTable& tab) {
    return (size_t)tab.n_rec * 32 + (size_t)n_cond * 32 + (size_t)(tab.n_node > 2 ? tab.n_node : 2) * 8;
}

// JMODE 8 / 9 behind that table (padded to 16 bytes): {r, 1 / r^2, 1 / (2 pi r^2)} [n_radii] | pairs [WPB][samples of a round][n_radii] double2
size_t radii_lds_bytes(int n_cond, const SystemRadii& tab, int samples_per_round) {
    return ((system_lds_bytes(n_cond, tab) + 15) & ~(size_t)15) + (size_t)((3 * tab.n_radii + 1) & ~1) * 8 +
           (size_t)WPB * samples_per_round * tab.n_radii * 16;
}

template <int L, int JMODE, bool MC, int NQ = 0, bool PM = false>
size_t r1_lds_bytes(const PlumeIO& io) {
    size_t lds = (size_t)fast_lds_doubles<L, JMODE>() * 8;
    if (NQ > 0) lds += (size_t)count_lds_bytes<(NQ > 0 ? NQ : 1), PM>();
    if (JMODE == 3) lds += (size_t)io.n_cond * (io.n_ang | 1) * 32;
    if (JMODE == 0) lds += (size_t)QPOLY_DOUBLES * 8;
    if (MC) lds += (size_t)MC_LDS_DOUBLES * 8;
    return lds;
}

// Workgroups resident per CU: bounded by the LDS (160 KB) and by the registers this instantiation was compiled to
// (hipFuncGetAttributes; 512 per SIMD lane) -- the persistent loop must launch exactly as many as fit, a workgroup that
// waits for a slot turns the tile split into a two-pass schedule -- and capped at two waves per SIMD, which measured
// best for the HBM-bound modes, three for the profile-less ones: the fused Monte-Carlo kernel uses a third wave to
// hide Philox's quarter-rate multiplies whenever its register count allows one (<= 168).
template <int L, bool COUPLED, int JMODE, bool MC, int NQ = 0, bool PM = false>
int r1_per_cu(size_t lds, long long* per_cu) {
    auto kern = plume_r1_kernel<L, COUPLED, JMODE, MC, NQ, PM>;
    // the register count belongs to the code object (one architecture): once per process
    static std::once_flag once;
    static int by_regs = 0;
    static hipError_t err = hipSuccess;
    std::call_once(once, [&] {
        hipFuncAttributes fa;
        err = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kern));
        if (err != hipSuccess) return;
        const int regs = fa.numRegs > 0 ? ((fa.numRegs + 7) & ~7) : 256;
        by_regs = (512 / regs) * 4 / WPB;
    });
    HIP_TRY(err);
    long long v = (long long)(160 * 1024 / lds);
    const int cap = (JMODE == 0 ? 12 : 8) / WPB;
    if (v > by_regs) v = by_regs;
    if (v > cap) v = cap;
    *per_cu = v;
    return PEM_OK;
}

// `grid_only`: report the grid the launch would use (the counting modes size their record buffer by it) and launch nothing
template <int L, bool COUPLED, int JMODE, bool MC = false, int NQ = 0, bool PM = false>
int launch_r1(const PlumeIO& io, const CoupledIO& cio, hipStream_t st, const McDesign& mc = McDesign{}, unsigned* grid_only = nullptr,
              const SystemTable* sys = nullptr, const SystemPredict* pr = nullptr, const SystemRadii* rd = nullptr) {
    size_t lds = r1_lds_bytes<L, JMODE, MC, NQ, PM>(io);
    if constexpr (JMODE == 6) lds += system_lds_bytes(io.n_cond, *sys);
    if constexpr (JMODE == 7) lds += system_lds_bytes(io.n_cond, *pr);
    if constexpr (JMODE == 8 || JMODE == 9) lds += radii_lds_bytes(io.n_cond, *rd, WAVE / L);
    const long long ntiles = (io.n + WAVE - 1) / WAVE;
    unsigned grid = 0;
    auto kern = plume_r1_kernel<L, COUPLED, JMODE, MC, NQ, PM>;
    if (lds > 64 * 1024) {
        static pem::LdsAttrOnce attr;
        HIP_TRY(attr.ensure(reinterpret_cast<const void*>(kern)));
    }
    long long per_cu = 0;
    if (int rc = r1_per_cu<L, COUPLED, JMODE, MC, NQ, PM>(lds, &per_cu)) return rc;
    // (the counting modes: a persistent grid of resident waves, each with its own region of the record buffer)
    if (int rc = fast_grid(per_cu, ntiles, JMODE == 1 || JMODE == 2, &grid)) return rc;
    if (grid_only) {
        *grid_only = grid;
        return PEM_OK;
    }
    if constexpr (MC) hipLaunchKernelGGL(kern, dim3(grid), dim3(WAVE * WPB), lds, st, io, cio, ntiles, mc);
    else if constexpr (JMODE == 6) hipLaunchKernelGGL(kern, dim3(grid), dim3(WAVE * WPB), lds, st, io, cio, ntiles, *sys);
    else if constexpr (JMODE == 7) hipLaunchKernelGGL(kern, dim3(grid), dim3(WAVE * WPB), lds, st, io, cio, ntiles, *pr);
    else if constexpr (JMODE == 8 || JMODE == 9) hipLaunchKernelGGL(kern, dim3(grid), dim3(WAVE * WPB), lds, st, io, cio, ntiles, *rd);
    else hipLaunchKernelGGL(kern, dim3(grid), dim3(WAVE * WPB), lds, st, io, cio, ntiles, NoDesign{});
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

template <bool COUPLED, int JMODE>
int dispatch_lanes(const PlumeIO& io, const CoupledIO& cio, hipStream_t st) {
    switch (g_lanes.load(std::memory_order_relaxed)) {
        case 2: return launch_r1<2, COUPLED, JMODE>(io, cio, st);
        case 8: return launch_r1<8, COUPLED, JMODE>(io, cio, st);
        default: return launch_r1<4, COUPLED, JMODE>(io, cio, st);
    }
}

}  // namespace

namespace pem {
char* error_buffer() {
    thread_local char buf[512] = "";
    return buf;
}
}  // namespace pem

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

const char* pem_last_error(void) { return pem::error_buffer(); }

int pem_set_lanes_per_sample(int lanes) {
    if (lanes == 0) lanes = 4;
    if (lanes == 2 || lanes == 4 || lanes == 8) g_lanes = lanes;
    return g_lanes;
}

int pem_persistent_grid(size_t n, int cus, int wg_per_cu, int memory_bound, size_t* workgroups, size_t* samples_per_round) {
    if (!workgroups || !samples_per_round) return fail(PEM_ERR_INVALID_ARG, "pem_persistent_grid: NULL result pointer");
    if (cus < 1 || wg_per_cu < 1) return fail(PEM_ERR_INVALID_ARG, "pem_persistent_grid: cus and wg_per_cu must be positive");
    const long long ntiles = (long long)((n + WAVE - 1) / WAVE);
    const long long g = persistent_grid(ntiles, cus, wg_per_cu, memory_bound != 0);
    const long long resident = g < (long long)cus * wg_per_cu ? g : (long long)cus * wg_per_cu;   // a one-shot grid is longer than that
    *workgroups = (size_t)g;
    *samples_per_round = (size_t)resident * WPB * WAVE;
    return PEM_OK;
}

int pem_coupled_occupancy(int profile_mode, int* cus, int* wg_per_cu) {
    if (!cus || !wg_per_cu) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_occupancy: NULL result pointer");
    if (int rc = check_device()) return rc;
    HIP_TRY(pem::device_cus(cus));
    PlumeIO io{};
    long long v = 0;
    int rc;
    // the instantiations pem_coupled_f64_dev / pem_coupled_mixed_dev launch at the current lanes-per-sample setting
#define PEM_OCC(L_)                                                                                      \
    (profile_mode == 0   ? r1_per_cu<L_, true, 0, false>(r1_lds_bytes<L_, 0, false>(io), &v)               \
     : profile_mode == 1 ? r1_per_cu<L_, true, 1, false>(r1_lds_bytes<L_, 1, false>(io), &v)               \
                         : r1_per_cu<L_, true, 2, false>(r1_lds_bytes<L_, 2, false>(io), &v))
    if (profile_mode < 0 || profile_mode > 2) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_occupancy: profile_mode must be 0, 1 or 2");
    switch (g_lanes.load(std::memory_order_relaxed)) {
        case 2: rc = PEM_OCC(2); break;
        case 8: rc = PEM_OCC(8); break;
        default: rc = PEM_OCC(4); break;
    }
#undef PEM_OCC
    if (rc) return rc;
    if (const char* e = getenv("PEM_WAVES_PER_CU")) {          // as fast_grid
        const long long w = atoll(e) / WPB;
        if (w >= 1 && w < v) v = w;
    }
    *wg_per_cu = (int)v;
    return PEM_OK;
}

const double* pem_angle_grid(void) {
    std::call_once(g_grid_once, [] {
        // np.linspace(0, pi/2, 91): k * ((pi/2) / 90), last point exactly pi/2 (plume.py:53)
        const double step = HALF_PI / 90.0;
        for (int k = 0; k < NANG; ++k) g_angle_grid[k] = (double)k * step;
        g_angle_grid[NANG - 1] = HALF_PI;
    });
    return g_angle_grid;
}

// ---- plume -------------------------------------------------------------------------------------
int pem_plume_f64_dev(size_t n, int n_radii, const double* radii, double torr2pa, const double* P_b, const double* c0,
                      const double* c1, const double* c2, const double* c3, const double* c4, const double* c5,
                      const double* sigma_cex, const double* I_B0, const double* T, double* j_ion, double* div_angle,
                      double* T_c, uint8_t* invalid, pem_stream_t stream) {
    if (n_radii < 1 || !radii) return fail(PEM_ERR_INVALID_ARG, "pem_plume: need at least one sweep radius");
    if (n == 0) return PEM_OK;
    if (!P_b || !c0 || !c1 || !c2 || !c3 || !c4 || !c5 || !sigma_cex || !I_B0 || !j_ion || !div_angle)
        return fail(PEM_ERR_INVALID_ARG, "pem_plume: NULL array");
    if ((T == nullptr) != (T_c == nullptr)) return fail(PEM_ERR_INVALID_ARG, "pem_plume: T and T_c go together");
    if (int rc = check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    PlumeIO io{(long long)n, torr2pa, radii[0], P_b, c0, c1, c2, c3, c4, c5, sigma_cex, I_B0, T, j_ion, div_angle, T_c, invalid};
    if (n_radii == 1 && aligned16(j_ion)) return dispatch_lanes<false, 1>(io, CoupledIO{}, st);
    return pem::launch_plume_radii(n, n_radii, radii, io, st);
}

// ---- coupled -----------------------------------------------------------------------------------
int pem_coupled_f64_dev(size_t n, double torr2pa, double radius, const double* P_b, const double* V_a, const double* T_e,
                        const double* V_vac, const double* Pstar, const double* P_T, const double* mdot_a,
                        const double* a_1, const double* c0, const double* c1, const double* c2, const double* c3,
                        const double* c4, const double* c5, const double* sigma_cex, double* V_cc, double* I_B0,
                        double* T, double* j_ion, double* div_angle, double* T_c, uint8_t* invalid, pem_stream_t stream) {
    if (n == 0) return PEM_OK;
    if (!P_b || !V_a || !T_e || !V_vac || !Pstar || !P_T || !mdot_a || !a_1 || !c0 || !c1 || !c2 || !c3 || !c4 || !c5 ||
        !sigma_cex || !V_cc || !div_angle || !T_c)
        return fail(PEM_ERR_INVALID_ARG, "pem_coupled: NULL array");
    if (j_ion && !aligned16(j_ion)) return fail(PEM_ERR_INVALID_ARG, "pem_coupled: j_ion must be 16-byte aligned");
    if (int rc = check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    PlumeIO io{(long long)n, torr2pa, radius, P_b, c0, c1, c2, c3, c4, c5, sigma_cex, nullptr, nullptr, j_ion, div_angle, T_c, invalid};
    CoupledIO cio{V_a, T_e, V_vac, Pstar, P_T, mdot_a, a_1, V_cc, I_B0, T};
    return j_ion ? dispatch_lanes<true, 1>(io, cio, st) : dispatch_lanes<true, 0>(io, cio, st);
}

// ---- coupled, inputs tile-interleaved: [ceil(n / 64)][15][64], one contiguous 7.5 KB block per 64-sample tile ----
int pem_coupled_tiled_f64_dev(size_t n, double torr2pa, double radius, const double* x_tiled, double* V_cc, double* I_B0,
                              double* T, double* j_ion, double* div_angle, double* T_c, uint8_t* invalid, pem_stream_t stream) {
    if (n == 0) return PEM_OK;
    if (!x_tiled || !V_cc || !div_angle || !T_c) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_tiled: NULL array");
    if (j_ion && !aligned16(j_ion)) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_tiled: j_ion must be 16-byte aligned");
    if (int rc = check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double* x = x_tiled;   // rows in the order of pem_coupled_f64_dev's arguments: P_b V_a T_e V_vac Pstar P_T mdot_a a_1 c0..c5 sigma_cex
    PlumeIO io{(long long)n, torr2pa, radius, x, x + 8 * WAVE, x + 9 * WAVE, x + 10 * WAVE, x + 11 * WAVE, x + 12 * WAVE, x + 13 * WAVE,
               x + 14 * WAVE, nullptr, nullptr, j_ion, div_angle, T_c, invalid};
    io.in_tile_stride = 15 * WAVE;
    CoupledIO cio{x + 1 * WAVE, x + 2 * WAVE, x + 3 * WAVE, x + 4 * WAVE, x + 5 * WAVE, x + 6 * WAVE, x + 7 * WAVE, V_cc, I_B0, T};
    return j_ion ? dispatch_lanes<true, 1>(io, cio, st) : dispatch_lanes<true, 0>(io, cio, st);
}

// ---- coupled, fused Monte-Carlo: inputs generated from the counter-based design inside the kernel ------------
int pem_coupled_mc_f64_dev(size_t n, uint64_t first_index, uint64_t seed, uint32_t stream_id, int swap_dim,
                           const int32_t* kind, const double* a, const double* b, double torr2pa, double radius,
                           double* x_out, size_t ld,
                           double* V_cc, double* I_B0, double* T, double* j_ion, double* div_angle, double* T_c,
                           uint8_t* invalid, pem_stream_t stream) {
    if (n == 0) return PEM_OK;
    if (!kind || !a || !b || !V_cc || !div_angle || !T_c) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_mc: NULL array");
    if (j_ion && !aligned16(j_ion)) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_mc: j_ion must be 16-byte aligned");
    if (x_out && ld < n) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_mc: leading dimension smaller than n");
    if (swap_dim < -2 || swap_dim >= 15) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_mc: swap_dim out of range");
    if (int rc = check_device()) return rc;
    McDesign mc{};
    mc.seed = seed;
    mc.first = first_index;
    mc.stream = stream_id;
    mc.swap_dim = swap_dim;
    for (int d = 0; d < 15; ++d) {
        if (kind[d] < PEM_DIST_UNIFORM || kind[d] > PEM_DIST_NORMAL)
            return fail(PEM_ERR_INVALID_ARG, "pem_coupled_mc: unknown distribution kind %d for input %d", kind[d], d);
        mc.kind[d] = kind[d];
        mc.a[d] = a[d];
        mc.b[d] = b[d];
    }
    mc.x_out = x_out;
    mc.ld = ld;
    PlumeIO io{(long long)n, torr2pa, radius, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, j_ion, div_angle, T_c, invalid, nullptr};
    CoupledIO cio{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, V_cc, I_B0, T};
    hipStream_t st = static_cast<hipStream_t>(stream);
    return j_ion ? launch_r1<4, true, 1, true>(io, cio, st, mc) : launch_r1<4, true, 0, true>(io, cio, st, mc);
}

}  // extern "C"

// ---- coupled, fused Monte-Carlo + campaign statistics: what csrc/pem_campaign.hip (pem_coupled_mc_stats_f64_dev) launches through
// csrc/pem_qfused.h

namespace {

int mc_design_of(const pem::McLaunch& a, McDesign* mc) {
    mc->seed = a.seed;
    mc->first = a.first_index;
    mc->stream = a.stream_id;
    mc->swap_dim = -1;
    for (int d = 0; d < 15; ++d) {
        if (a.kind[d] < PEM_DIST_UNIFORM || a.kind[d] > PEM_DIST_NORMAL)
            return fail(PEM_ERR_INVALID_ARG, "pem_coupled_mc: unknown distribution kind %d for input %d", a.kind[d], d);
        mc->kind[d] = a.kind[d];
        mc->a[d] = a.a[d];
        mc->b[d] = a.b[d];
    }
    mc->x_out = a.x_out;
    mc->ld = a.ld;
    return PEM_OK;
}

// the counting launch for nq quantiles: instantiated for 3, 5 and 6 brackets per angle (fewer are padded with empty ones)
template <int JMODE>
int launch_count(const PlumeIO& io, const CoupledIO& cio, const McDesign& mc, int nq, hipStream_t st, unsigned* grid_only) {
    // (the premask rides with up to five brackets: six leave no LDS for its thresholds beside two workgroups per CU)
    if (io.q.premask && nq <= 5) return launch_r1<4, true, JMODE, true, 5, true>(io, cio, st, mc, grid_only);
    if (nq <= 3) return launch_r1<4, true, JMODE, true, 3>(io, cio, st, mc, grid_only);
    if (nq <= 5) return launch_r1<4, true, JMODE, true, 5>(io, cio, st, mc, grid_only);
    return launch_r1<4, true, JMODE, true, 6>(io, cio, st, mc, grid_only);
}

}  // namespace

namespace pem {

int launch_coupled_mc(const McLaunch& a, hipStream_t st) {
    if (a.n == 0) return PEM_OK;
    McDesign mc{};
    if (int rc = mc_design_of(a, &mc)) return rc;
    PlumeIO io{(long long)a.n, a.torr2pa, a.radius, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, a.j_ion, a.div_angle, a.T_c, a.invalid, nullptr};
    CoupledIO cio{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, a.V_cc, a.I_B0, a.T};
    return a.j_ion ? launch_r1<4, true, 1, true>(io, cio, st, mc) : launch_r1<4, true, 0, true>(io, cio, st, mc);
}

static int count_launch(const McLaunch& a, const CountIO& c, bool store_profile, hipStream_t st, unsigned* grid_only) {
    McDesign mc{};
    if (int rc = mc_design_of(a, &mc)) return rc;
    PlumeIO io{(long long)a.n, a.torr2pa, a.radius, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, a.j_ion, a.div_angle, a.T_c, a.invalid, nullptr};
    io.q = c;
    CoupledIO cio{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, a.V_cc, a.I_B0, a.T};
    return store_profile ? launch_count<4>(io, cio, mc, c.nq, st, grid_only) : launch_count<5>(io, cio, mc, c.nq, st, grid_only);
}

int coupled_count_waves(size_t n, int nq, bool store_profile, unsigned* waves) {
    McLaunch a{};
    a.n = n;
    for (int d = 0; d < 15; ++d) a.kind[d] = PEM_DIST_UNIFORM;
    CountIO c{};
    c.nq = nq;
    unsigned grid = 0;
    if (int rc = count_launch(a, c, store_profile, nullptr, &grid)) return rc;
    *waves = grid * WPB;
    return PEM_OK;
}

int launch_coupled_mc_count(const McLaunch& a, const CountIO& c, bool store_profile, hipStream_t st) {
    if (a.n == 0) return PEM_OK;
    if (c.nq < 1 || c.nq > 6 || !c.br || !c.below || !c.rec || !c.rec_count || !c.flags || c.cap == 0)
        return fail(PEM_ERR_INVALID_ARG, "counting launch: incomplete arguments");
    if (store_profile && !a.j_ion) return fail(PEM_ERR_INVALID_ARG, "counting launch: no profile array to store into");
    return count_launch(a, c, store_profile, st, nullptr);
}

}  // namespace pem

extern "C" {

// ---- coupled + likelihood fused: the profile never leaves the chip ------------------------------------------------
int pem_coupled_loglik_f64_dev(size_t n, double torr2pa, double radius, const double* P_b, const double* V_a,
                               const double* T_e, const double* V_vac, const double* Pstar, const double* P_T,
                               const double* mdot_a, const double* a_1, const double* c0, const double* c1, const double* c2,
                               const double* c3, const double* c4, const double* c5, const double* sigma_cex, int n_cond,
                               int n_ang, const int32_t* kidx, const double* weight, const double* y, const double* inv_std,
                               double* V_cc, double* div_angle, double* T_c, double* loglik, uint8_t* invalid,
                               pem_stream_t stream) {
    if (n_cond < 1 || n_ang < 1 || (long long)n_cond * (n_ang | 1) > PEM_FUSED_LOGLIK_MAX_MEASUREMENTS)
        return fail(PEM_ERR_INVALID_ARG, "pem_coupled_loglik: 1 <= n_cond * (n_ang | 1) <= %d", PEM_FUSED_LOGLIK_MAX_MEASUREMENTS);
    if (n == 0) return PEM_OK;
    if (!P_b || !V_a || !T_e || !V_vac || !Pstar || !P_T || !mdot_a || !a_1 || !c0 || !c1 || !c2 || !c3 || !c4 || !c5 ||
        !sigma_cex || !kidx || !weight || !y || !inv_std || !V_cc || !div_angle || !T_c || !loglik)
        return fail(PEM_ERR_INVALID_ARG, "pem_coupled_loglik: NULL array");
    if (int rc = check_device()) return rc;
    PlumeIO io{(long long)n, torr2pa, radius, P_b, c0, c1, c2, c3, c4, c5, sigma_cex, nullptr, nullptr, nullptr, div_angle, T_c, invalid, nullptr,
               kidx, weight, y, inv_std, loglik, n_cond, n_ang};
    CoupledIO cio{V_a, T_e, V_vac, Pstar, P_T, mdot_a, a_1, V_cc, nullptr, nullptr};
    return launch_r1<4, true, 3>(io, cio, static_cast<hipStream_t>(stream));
}

// ---- coupled + multi-QoI likelihood fused: j_ion against the staged profile, V_cc / T / u_ion in the epilogue ----------
int pem_coupled_system_loglik_f64_dev(size_t n, double torr2pa, double radius, const double* P_b, const double* V_a,
                                      const double* T_e, const double* V_vac, const double* Pstar, const double* P_T,
                                      const double* mdot_a, const double* a_1, const double* c0, const double* c1, const double* c2,
                                      const double* c3, const double* c4, const double* c5, const double* sigma_cex, int n_cond,
                                      int n_rec, const double* rec, const int32_t* span, int n_node, const int32_t* node, double z0,
                                      double z1, int ncells, double* V_cc, double* div_angle, double* T_c, double* loglik,
                                      uint8_t* invalid, pem_stream_t stream) {
    if (n_cond < 1 || n_cond > PEM_FUSED_SYSTEM_MAX_RECORDS || n_rec < 0 || n_rec > PEM_FUSED_SYSTEM_MAX_RECORDS || n_node < 0 ||
        n_node > 2 * PEM_FUSED_SYSTEM_MAX_RECORDS)
        return fail(PEM_ERR_INVALID_ARG, "pem_coupled_system_loglik: 1 <= n_cond <= %d, 0 <= n_rec <= %d, 0 <= n_node <= %d "
                    "(PEM_FUSED_SYSTEM_MAX_RECORDS)", PEM_FUSED_SYSTEM_MAX_RECORDS, PEM_FUSED_SYSTEM_MAX_RECORDS,
                    2 * PEM_FUSED_SYSTEM_MAX_RECORDS);
    if (n_node > 0 && ncells < 2) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_system_loglik: need at least 2 u_ion grid points");
    if (n == 0) return PEM_OK;
    if (!P_b || !V_a || !T_e || !V_vac || !Pstar || !P_T || !mdot_a || !a_1 || !c0 || !c1 || !c2 || !c3 || !c4 || !c5 ||
        !sigma_cex || (n_rec > 0 && !rec) || !span || (n_node > 0 && !node) || !V_cc || !div_angle || !T_c || !loglik)
        return fail(PEM_ERR_INVALID_ARG, "pem_coupled_system_loglik: NULL array");
    if (int rc = check_device()) return rc;
    PlumeIO io{(long long)n, torr2pa, radius, P_b, c0, c1, c2, c3, c4, c5, sigma_cex, nullptr, nullptr, nullptr, div_angle, T_c, invalid, nullptr,
               nullptr, nullptr, nullptr, nullptr, loglik, n_cond, 0};
    CoupledIO cio{V_a, T_e, V_vac, Pstar, P_T, mdot_a, a_1, V_cc, nullptr, nullptr};
    const SystemTable tab{rec, span, node, n_rec, n_node, z0, z1, ncells};
    return launch_r1<4, true, 6>(io, cio, static_cast<hipStream_t>(stream), McDesign{}, nullptr, &tab);
}

// ---- coupled + the model value at every record of the multi-QoI table (JMODE 6's table, stored instead of compared) --------
int pem_coupled_system_predict_f64_dev(size_t n, double torr2pa, double radius, const double* P_b, const double* V_a,
                                       const double* T_e, const double* V_vac, const double* Pstar, const double* P_T,
                                       const double* mdot_a, const double* a_1, const double* c0, const double* c1, const double* c2,
                                       const double* c3, const double* c4, const double* c5, const double* sigma_cex, int n_cond,
                                       int n_rec, const double* rec, const int32_t* span, int n_node, const int32_t* node, double z0,
                                       double z1, int ncells, double* V_cc, double* div_angle, double* T_c, double* pred,
                                       size_t ld_pred, uint8_t* invalid, pem_stream_t stream) {
    if (n_cond < 1 || n_cond > PEM_FUSED_SYSTEM_MAX_RECORDS || n_rec < 0 || n_rec > PEM_FUSED_SYSTEM_MAX_RECORDS || n_node < 0 ||
        n_node > 2 * PEM_FUSED_SYSTEM_MAX_RECORDS)
        return fail(PEM_ERR_INVALID_ARG, "pem_coupled_system_predict: 1 <= n_cond <= %d, 0 <= n_rec <= %d, 0 <= n_node <= %d "
                    "(PEM_FUSED_SYSTEM_MAX_RECORDS)", PEM_FUSED_SYSTEM_MAX_RECORDS, PEM_FUSED_SYSTEM_MAX_RECORDS,
                    2 * PEM_FUSED_SYSTEM_MAX_RECORDS);
    if (n_node > 0 && ncells < 2) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_system_predict: need at least 2 u_ion grid points");
    if (ld_pred < (size_t)n_rec) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_system_predict: ld_pred < n_rec");
    if (n == 0) return PEM_OK;
    if (!P_b || !V_a || !T_e || !V_vac || !Pstar || !P_T || !mdot_a || !a_1 || !c0 || !c1 || !c2 || !c3 || !c4 || !c5 ||
        !sigma_cex || (n_rec > 0 && !rec) || !span || (n_node > 0 && !node) || !pred)
        return fail(PEM_ERR_INVALID_ARG, "pem_coupled_system_predict: NULL array");
    if (int rc = check_device()) return rc;
    PlumeIO io{(long long)n, torr2pa, radius, P_b, c0, c1, c2, c3, c4, c5, sigma_cex, nullptr, nullptr, nullptr, div_angle, T_c, invalid, nullptr,
               nullptr, nullptr, nullptr, nullptr, nullptr, n_cond, 0};
    CoupledIO cio{V_a, T_e, V_vac, Pstar, P_T, mdot_a, a_1, V_cc, nullptr, nullptr};
    SystemPredict pr;
    static_cast<SystemTable&>(pr) = SystemTable{rec, span, node, n_rec, n_node, z0, z1, ncells};
    pr.pred = pred;
    pr.ld_pred = (long long)ld_pred;
    return launch_r1<4, true, 7>(io, cio, static_cast<hipStream_t>(stream), McDesign{}, nullptr, nullptr, &pr);
}

// ---- the same two launches against j_ion measured at several sweep radii: one model evaluation per sample (JMODE 8 / 9) ------
// every check of the two entry points that needs no device; `who` names the entry point in the message
static int check_system_radii(const char* who, int n_radii, const double* radii, int n_cond, int n_rec, int n_node, int ncells) {
    if (n_radii < 2 || n_radii > PEM_FUSED_SYSTEM_MAX_RADII)
        return fail(PEM_ERR_INVALID_ARG, "%s: 2 <= n_radii <= %d (PEM_FUSED_SYSTEM_MAX_RADII), got %d", who, PEM_FUSED_SYSTEM_MAX_RADII, n_radii);
    if (!radii) return fail(PEM_ERR_INVALID_ARG, "%s: NULL radii", who);
    for (int r = 0; r < n_radii; ++r) {
        if (!(std::isfinite(radii[r]) && radii[r] > 0.0)) return fail(PEM_ERR_INVALID_ARG, "%s: radii must be finite and positive, radii[%d] = %g", who, r, radii[r]);
        if (r > 0 && !(radii[r] > radii[r - 1])) return fail(PEM_ERR_INVALID_ARG, "%s: radii must be strictly ascending, radii[%d] = %g after %g", who, r, radii[r], radii[r - 1]);
    }
    if (n_cond < 1 || n_cond > PEM_FUSED_SYSTEM_MAX_RECORDS || n_rec < 0 || n_rec > PEM_FUSED_SYSTEM_MAX_RECORDS || n_node < 0 ||
        n_node > 2 * PEM_FUSED_SYSTEM_MAX_RECORDS)
        return fail(PEM_ERR_INVALID_ARG, "%s: 1 <= n_cond <= %d, 0 <= n_rec <= %d, 0 <= n_node <= %d (PEM_FUSED_SYSTEM_MAX_RECORDS)", who,
                    PEM_FUSED_SYSTEM_MAX_RECORDS, PEM_FUSED_SYSTEM_MAX_RECORDS, 2 * PEM_FUSED_SYSTEM_MAX_RECORDS);
    if (n_node > 0 && ncells < 2) return fail(PEM_ERR_INVALID_ARG, "%s: need at least 2 u_ion grid points", who);
    return PEM_OK;
}

static SystemRadii system_radii_arg(int n_radii, const double* radii, int n_rec, const double* rec, const int32_t* span, int n_node,
                                    const int32_t* node, double z0, double z1, int ncells, double* pred, size_t ld_pred) {
    SystemRadii rd;
    static_cast<SystemTable&>(rd) = SystemTable{rec, span, node, n_rec, n_node, z0, z1, ncells};
    rd.pred = pred;
    rd.ld_pred = (long long)ld_pred;
    rd.n_radii = n_radii;
    for (int r = 0; r < SYS_RADII_MAX; ++r) rd.radii[r] = radii[r < n_radii ? r : n_radii - 1];
    return rd;
}

int pem_coupled_system_loglik_radii_f64_dev(size_t n, double torr2pa, int n_radii, const double* radii, const double* P_b,
                                            const double* V_a, const double* T_e, const double* V_vac, const double* Pstar,
                                            const double* P_T, const double* mdot_a, const double* a_1, const double* c0,
                                            const double* c1, const double* c2, const double* c3, const double* c4, const double* c5,
                                            const double* sigma_cex, int n_cond, int n_rec, const double* rec, const int32_t* span,
                                            int n_node, const int32_t* node, double z0, double z1, int ncells, double* V_cc,
                                            double* div_angle, double* T_c, double* loglik, uint8_t* invalid, pem_stream_t stream) {
    if (int rc = check_system_radii("pem_coupled_system_loglik_radii", n_radii, radii, n_cond, n_rec, n_node, ncells)) return rc;
    if (n == 0) return PEM_OK;
    if (!P_b || !V_a || !T_e || !V_vac || !Pstar || !P_T || !mdot_a || !a_1 || !c0 || !c1 || !c2 || !c3 || !c4 || !c5 ||
        !sigma_cex || (n_rec > 0 && !rec) || !span || (n_node > 0 && !node) || !V_cc || !div_angle || !T_c || !loglik)
        return fail(PEM_ERR_INVALID_ARG, "pem_coupled_system_loglik_radii: NULL array");
    if (int rc = check_device()) return rc;
    PlumeIO io{(long long)n, torr2pa, radii[n_radii - 1], P_b, c0, c1, c2, c3, c4, c5, sigma_cex, nullptr, nullptr, nullptr, div_angle, T_c, invalid, nullptr,
               nullptr, nullptr, nullptr, nullptr, loglik, n_cond, 0};
    CoupledIO cio{V_a, T_e, V_vac, Pstar, P_T, mdot_a, a_1, V_cc, nullptr, nullptr};
    const SystemRadii rd = system_radii_arg(n_radii, radii, n_rec, rec, span, n_node, node, z0, z1, ncells, nullptr, 0);
    return launch_r1<4, true, 8>(io, cio, static_cast<hipStream_t>(stream), McDesign{}, nullptr, nullptr, nullptr, &rd);
}

int pem_coupled_system_predict_radii_f64_dev(size_t n, double torr2pa, int n_radii, const double* radii, const double* P_b,
                                             const double* V_a, const double* T_e, const double* V_vac, const double* Pstar,
                                             const double* P_T, const double* mdot_a, const double* a_1, const double* c0,
                                             const double* c1, const double* c2, const double* c3, const double* c4, const double* c5,
                                             const double* sigma_cex, int n_cond, int n_rec, const double* rec, const int32_t* span,
                                             int n_node, const int32_t* node, double z0, double z1, int ncells, double* V_cc,
                                             double* div_angle, double* T_c, double* pred, size_t ld_pred, uint8_t* invalid,
                                             pem_stream_t stream) {
    if (int rc = check_system_radii("pem_coupled_system_predict_radii", n_radii, radii, n_cond, n_rec, n_node, ncells)) return rc;
    if (ld_pred < (size_t)n_rec) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_system_predict_radii: ld_pred < n_rec");
    if (n == 0) return PEM_OK;
    if (!P_b || !V_a || !T_e || !V_vac || !Pstar || !P_T || !mdot_a || !a_1 || !c0 || !c1 || !c2 || !c3 || !c4 || !c5 ||
        !sigma_cex || (n_rec > 0 && !rec) || !span || (n_node > 0 && !node) || !pred)
        return fail(PEM_ERR_INVALID_ARG, "pem_coupled_system_predict_radii: NULL array");
    if (int rc = check_device()) return rc;
    PlumeIO io{(long long)n, torr2pa, radii[n_radii - 1], P_b, c0, c1, c2, c3, c4, c5, sigma_cex, nullptr, nullptr, nullptr, div_angle, T_c, invalid, nullptr,
               nullptr, nullptr, nullptr, nullptr, nullptr, n_cond, 0};
    CoupledIO cio{V_a, T_e, V_vac, Pstar, P_T, mdot_a, a_1, V_cc, nullptr, nullptr};
    const SystemRadii rd = system_radii_arg(n_radii, radii, n_rec, rec, span, n_node, node, z0, z1, ncells, pred, ld_pred);
    return launch_r1<4, true, 9>(io, cio, static_cast<hipStream_t>(stream), McDesign{}, nullptr, nullptr, nullptr, &rd);
}

// ---- coupled, mixed precision: fp64 arithmetic, the 91-point profile stored as fp32 -----------------
int pem_coupled_mixed_dev(size_t n, double torr2pa, double radius, const double* P_b, const double* V_a, const double* T_e,
                          const double* V_vac, const double* Pstar, const double* P_T, const double* mdot_a,
                          const double* a_1, const double* c0, const double* c1, const double* c2, const double* c3,
                          const double* c4, const double* c5, const double* sigma_cex, double* V_cc, double* I_B0,
                          double* T, float* j_ion_f32, double* div_angle, double* T_c, uint8_t* invalid,
                          pem_stream_t stream) {
    if (n == 0) return PEM_OK;
    if (!P_b || !V_a || !T_e || !V_vac || !Pstar || !P_T || !mdot_a || !a_1 || !c0 || !c1 || !c2 || !c3 || !c4 || !c5 ||
        !sigma_cex || !V_cc || !div_angle || !T_c || !j_ion_f32)
        return fail(PEM_ERR_INVALID_ARG, "pem_coupled_mixed: NULL array");
    if (!aligned16(j_ion_f32)) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_mixed: j_ion_f32 must be 16-byte aligned");
    if (int rc = check_device()) return rc;
    PlumeIO io{(long long)n, torr2pa, radius, P_b, c0, c1, c2, c3, c4, c5, sigma_cex, nullptr, nullptr, nullptr, div_angle, T_c, invalid, j_ion_f32};
    CoupledIO cio{V_a, T_e, V_vac, Pstar, P_T, mdot_a, a_1, V_cc, I_B0, T};
    return dispatch_lanes<true, 2>(io, cio, static_cast<hipStream_t>(stream));
}

}  // extern "C"
