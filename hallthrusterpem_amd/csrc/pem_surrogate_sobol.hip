// pem_surrogate_sobol.hip -- the Sobol' study over a pressure sweep through the chained surrogate (gfx950).
//
// scripts/pem_v0/sobol.py:70-98: the reference's model() obtains V_cc, T and u_ion(z = L_ch) from `SURR.predict` of the component
// chain; only j_ion goes to the true plume model (:82-90).  pem_sobol_sweep.hip evaluates the analytic stages; this unit puts the
// chain's cathode and thruster tables in their place.  One launch covers one group at EVERY pressure (blockIdx.y = pressure), one lane
// per base sample: the lane draws rows A and B of pem_sobol_sweep_f64_dev's design (pem_sobol_design.h: the same streams, tables and
// Philox numbers), maps them to the chain's coordinates, runs the cathode stage and, for the Thruster group, the coupling map and the
// thruster stage -- never the plume stage, which no index of V_cc, T or u_ion reads -- rebuilds the one u_ion cell the study looks at
// from the latents, and adds the estimator terms to per-wave fp64 accumulators (pem_wave.h).  Only one partial per workgroup reaches
// HBM.  The stages, the coupling map and the field expression are pem_surrogate.hip's and pem_surrogate_fields.hip's device code,
// compiled here once more (that file is included below with its entry points left out).
#define PEM_SURROGATE_SOBOL_UNIT
#include "pem_surrogate_fields.hip"
#include "pem_sobol_design.h"
#include "pem_wave.h"

namespace {

constexpr int CFLAG = 2;      // non-physical thruster values, V_cc coupling coordinates outside [-1, 1]

struct SobolArg {
    unsigned long long seed, first;
    long long n;
    int n_p, n_dim, vcc_slot, basis_words;
    int u_rank, u_norm;
    double vcc_lo, vcc_w, u_scale;
};

// per input row c of the design: the coordinate slot it feeds (-1: the chain does not carry it) and that slot's map
struct SlotMap {
    int slot[NIN], is_log[NIN];
    double a[NIN], w[NIN];
};

// The head of the dynamic LDS, in doubles: the accumulators [4][NV + 1][8], the counts [4][8], the prior table's a and b and the
// slot map's a and w (16 each), then 64 ints (kind, slot, is_log of 16 each, the slots the cathode table reads).  The stages' bases
// and the coordinates follow.  All of it is dynamic so that one figure, the launch's, is held against the 160 KB.
__host__ __device__ constexpr int head_doubles(int g) { return 4 * (n_varied(g) + 1) * 8 + 32 + 4 * 16 + 32; }

// an input x -> its normalised coordinate over the chain's box: SurrogatePosterior.assemble_inputs' expression, left to right, no
// contraction.  Out of line, as transform_call: one body of log10 for every input.
__device__ __attribute__((noinline)) double slot_coord_call(double x, int is_log, double a, double w) {
#pragma clang fp contract(off)
    const double u = is_log ? log10(x) : x;
    return 2.0 * (u - a) / w - 1.0;
}

// f_out: [n_p][NV + 2][NQ][n]; partial: [n_p][gridDim.x][2 + 4 NV][NQ]; flags: [n_p][gridDim.x][2]
template <int G, int UW, bool UEXACT>
__global__ __launch_bounds__(BLOCK) void chain_sobol_sweep_kernel(SobolArg s, SlotMap sm, ChainStage cat, ChainStage thr,
                                                                  const int* __restrict__ kind_t, const double* __restrict__ a_t,
                                                                  const double* __restrict__ b_t, const double* __restrict__ ub,
                                                                  double* __restrict__ f_out, double* __restrict__ partial,
                                                                  uint64_t* __restrict__ flags) {
    static_assert(G == PEM_SWEEP_CATHODE || G == PEM_SWEEP_THRUSTER, "the Plume group stays on the model");
    constexpr int NV = n_varied(G), NQ = n_qoi(G), ROWS = 2 + 4 * NV;
    constexpr bool THRUSTER = G == PEM_SWEEP_THRUSTER;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double (*acc)[NV + 1][8] = reinterpret_cast<double (*)[NV + 1][8]>(lds);      // [wave][0: the A/B statistics, 1 + j: varied input j][value]
    double (*cnt)[8] = reinterpret_cast<double (*)[8]>(lds + 4 * (NV + 1) * 8);   // [wave][flag]
    double* lds_a = lds + 4 * (NV + 1) * 8 + 32;
    double* lds_b = lds_a + 16;
    double* lds_ca = lds_b + 16;
    double* lds_cw = lds_ca + 16;
    int* lds_kind = reinterpret_cast<int*>(lds_cw + 16);
    int* lds_slot = lds_kind + 16;
    int* lds_log = lds_slot + 16;
    unsigned* cat_reads = reinterpret_cast<unsigned*>(lds_log + 16);
    double* basis = lds + head_doubles(G);                   // a stage's outer bases
    double* coord = basis + (size_t)s.basis_words * BLOCK;   // [n_dim][BLOCK]: the external coordinates and the V_cc slot
    const int p = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int c = 0; c < NIN; ++c)
        if (tid == c) {
            lds_kind[c] = kind_t[p * NIN + c];
            lds_a[c] = a_t[p * NIN + c];
            lds_b[c] = b_t[p * NIN + c];
            lds_slot[c] = sm.slot[c];
            lds_log[c] = sm.is_log[c];
            lds_ca[c] = sm.a[c];
            lds_cw[c] = sm.w[c];
        }
    if (tid == 0) *cat_reads = 0u;
    for (int i = tid; i < 4 * (NV + 1) * 8; i += BLOCK) (&acc[0][0][0])[i] = 0.0;
    __syncthreads();
    // the slots the cathode table reads: an AB evaluation whose swapped input is none of them has row A's V_cc
    if constexpr (THRUSTER) {
        unsigned m = 0u;
        for (int bi = tid; bi < cat.n_beta; bi += BLOCK) {
            const int32_t* e = cat.index + (size_t)bi * IDX_STRIDE;
            for (int k = 0; k < min(e[0], MAXA); ++k) m |= 1u << (e[2 + k] & 31);
        }
        if (m) atomicOr(cat_reads, m);
        __syncthreads();
    }
    // the pinned inputs the chain carries: their coordinates, once (the slots are this thread's own)
#pragma nounroll
    for (int c = 0; c < NIN; ++c) {
        const int d = lds_slot[c];
        if (is_varied(G, c) || d < 0) continue;
        coord[d * BLOCK + tid] = slot_coord_call(lds_a[c], __builtin_amdgcn_readfirstlane(lds_log[c]), lds_ca[c], lds_cw[c]);
    }
    const int n_thr = UEXACT ? UW : thr.n_out;
    const unsigned reads = THRUSTER ? *cat_reads : 0u;
    const int my_slot = pem::wave_sum8_slot(lane);
    unsigned int bad_thruster = 0, outside = 0;
    // every wave runs the same number of iterations (the reductions need all 64 lanes): lanes past n evaluate the last
    // sample and contribute zeros
    const long long n = s.n;
    const long long stride = (long long)gridDim.x * BLOCK;
    const long long iters = (n + stride - 1) / stride;
    for (long long it = 0; it < iters; ++it) {
        const long long i = it * stride + (long long)blockIdx.x * BLOCK + tid;
        const bool live = i < n;
        const unsigned long long g = s.first + (unsigned long long)(live ? i : n - 1);
        double ta[NV], tb[NV], fa[2], fb[2], tva = 0.0;
        // ONE body of the stages, a rolled loop over the evaluations of a base sample: 0 = row A, 1 = row B, 2 + j = A with
        // column varied_input(j) from B.  The rows live as coordinates: nothing else of them is read.
        for (int e = 0; e < NV + 2; ++e) {
            double tc[NV];
            if (e < 2) {
                double x[NIN];
                design_row<G>(s.seed, lds_kind, lds_a, lds_b, g, row_stream(G, s.n_p, p, 0, e), x);
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const int c = varied_input(G, j);
                    tc[j] = slot_coord_call(x[c], __builtin_amdgcn_readfirstlane(lds_log[c]), lds_ca[c], lds_cw[c]);
                    ta[j] = e == 0 ? tc[j] : ta[j];
                    tb[j] = e == 1 ? tc[j] : tb[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < NV; ++j) tc[j] = j == e - 2 ? tb[j] : ta[j];
            }
            int swapped = 0;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int d = lds_slot[varied_input(G, j)];
                coord[d * BLOCK + tid] = tc[j];
                if (j == e - 2) swapped = d;
            }
            // (each stage reads and writes this thread's own slots only: no barrier between the stages)
            double vcc[1] = {0.0}, tv;
            if (THRUSTER && e >= 2 && !((reads >> swapped) & 1u)) {
                tv = tva;
            } else {
                stage_predict<1, true>(cat, coord, basis, tid, vcc);
                tv = coupling_coord(vcc[0], s.vcc_lo, s.vcc_w);
                if (e == 0) tva = tv;
            }
            if (live) outside += !(tv >= -1.0 && tv <= 1.0);
            double f[2] = {vcc[0], 0.0};
            if constexpr (THRUSTER) {
                coord[s.vcc_slot * BLOCK + tid] = tv;
                double thrust[UW];
                stage_predict<UW, UEXACT>(thr, coord, basis, tid, thrust);
                if (live) bad_thruster += thrust[1] < 0.0 || thrust[0] < 0.0;
                f[0] = thrust[1];
                // the cell's value: rebuild_field's sum over the latents and its denormalisation
                double v = 0.0;
#pragma unroll
                for (int o = 2; o < UW; ++o)
                    if (UEXACT || o < n_thr) v = fma(thrust[o], ub[o - 2], v);
                if (s.u_norm == PEM_NORM_LOG10) v = exp10(v);
                else if (s.u_norm == PEM_NORM_LINEAR) v = v / s.u_scale;
                f[1] = UW > 2 ? v : __builtin_nan("");       // a chain without u_ion latents: made visible
            }
            if (f_out && live) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) f_out[(((size_t)p * (NV + 2) + e) * NQ + q) * (size_t)n + i] = f[q];
            }
            if (e == 0) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) fa[q] = f[q];
                continue;
            }
            double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (e == 1) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    fb[q] = f[q];
                    v[q] = fa[q] + f[q];
                    v[NQ + q] = fma(fa[q], fa[q], f[q] * f[q]);
                }
            } else {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const double t1 = fb[q] * (f[q] - fa[q]), t2 = (fa[q] - f[q]) * (fa[q] - f[q]);
                    v[q] = t1;
                    v[NQ + q] = t1 * t1;
                    v[2 * NQ + q] = t2;
                    v[3 * NQ + q] = t2 * t2;
                }
            }
            if (!live) {
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = 0.0;
            }
            const double tot = pem::wave_sum8(v, lane);
            if (lane < 8) acc[wave][e - 1][my_slot] += tot;
        }
    }
    {
        double v[8] = {(double)bad_thruster, (double)outside, 0, 0, 0, 0, 0, 0};
        const double tot = pem::wave_sum8(v, lane);
        if (lane < 8) cnt[wave][my_slot] = tot;
    }
    __syncthreads();
    // one partial per workgroup, in a fixed order (deterministic).  Row 0, 1 <- acc[.][0][{0, 1} NQ + q];
    // row 2 + 4 j + w <- acc[.][1 + j][w NQ + q]
    const size_t blk = (size_t)p * gridDim.x + blockIdx.x;
    if (tid < ROWS * NQ) {
        const int row = tid / NQ, q = tid - row * NQ;
        const int e = row < 2 ? 0 : 1 + (row - 2) / 4, w = row < 2 ? row : (row - 2) % 4;
        partial[blk * ROWS * NQ + tid] = acc[0][e][w * NQ + q] + acc[1][e][w * NQ + q] + acc[2][e][w * NQ + q] + acc[3][e][w * NQ + q];
    }
    if (tid < CFLAG) flags[blk * CFLAG + tid] = (uint64_t)cnt[0][tid] + (uint64_t)cnt[1][tid] + (uint64_t)cnt[2][tid] + (uint64_t)cnt[3][tid];
}

template <int G, int UW, bool UEXACT>
void launch_chain_sobol(dim3 grid, size_t lds, hipStream_t st, const SobolArg& s, const SlotMap& sm, const ChainStage (&cs)[3],
                        const int32_t* kind, const double* a, const double* b, const double* ub, double* f_out, double* partial,
                        uint64_t* flags) {
    if (lds > 64 * 1024) {
        static pem::LdsAttrOnce attr;
        (void)attr.ensure(reinterpret_cast<const void*>(chain_sobol_sweep_kernel<G, UW, UEXACT>));      // a refusal shows as a launch error below
    }
    hipLaunchKernelGGL((chain_sobol_sweep_kernel<G, UW, UEXACT>), grid, dim3(BLOCK), lds, st, s, sm, cs[0], cs[1], kind, a, b, ub, f_out,
                       partial, flags);
}

}  // namespace

extern "C" int pem_chain_sobol_sweep_f64_dev(int group, size_t n_base, uint64_t first_index, uint64_t seed, int n_p, const int32_t* kind,
                                             const double* a, const double* b, int n_dim, int vcc_slot, int ib0_slot,
                                             const pem_surr_stage* stages, double vcc_lo, double vcc_w, const int32_t* slot_row,
                                             const int32_t* slot_log, const double* slot_a, const double* slot_w, int u_rank, int u_dof,
                                             int u_norm, double u_scale, const double* u_basis, int u_cell, double* f_out,
                                             double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream) {
    const char* who = "pem_chain_sobol_sweep_f64";
    if (group == PEM_SWEEP_PLUME)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: the Plume group stays on the model (pem_sobol_sweep_f64_dev): the chain serves V_cc, T and u_ion", who);
    if (group != PEM_SWEEP_CATHODE && group != PEM_SWEEP_THRUSTER) return pem::fail(PEM_ERR_INVALID_ARG, "%s: unknown group %d", who, group);
    if (n_p < 1 || n_p > PEM_SWEEP_MAX_PRESSURES)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: 1 <= n_p <= %d pressures, got %d", who, PEM_SWEEP_MAX_PRESSURES, n_p);
    if (n_blocks < 1) return pem::fail(PEM_ERR_INVALID_ARG, "%s: n_blocks must be positive", who);
    if (n_base < 1 || n_base > (size_t)1 << 40) return pem::fail(PEM_ERR_INVALID_ARG, "%s: 1 <= n_base <= 2^40", who);
    if (!kind || !a || !b || !partial || !flags) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL array", who);
    if (int rc0 = check_uion(who, 2, u_rank, u_dof, u_norm, u_scale, u_basis)) return rc0;
    if (u_rank > 0 && (u_cell < 0 || u_cell >= u_dof))
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: cell %d is outside the u_ion grid of %d cells", who, u_cell, u_dof);
    ChainStage cs[3];
    int basis_words = 0;
    // (the plume table is checked as the parents check it and never read; its coupling domain is not asked for)
    if (int rc0 = check_chain(who, n_dim, vcc_slot, ib0_slot, stages, vcc_lo, vcc_w, 0.0, 1.0, cs, basis_words, 2 + u_rank)) return rc0;
    const bool thruster = group == PEM_SWEEP_THRUSTER;
    basis_words = cs[0].max_outer * cs[0].max_m;
    if (thruster && cs[1].max_outer * cs[1].max_m > basis_words) basis_words = cs[1].max_outer * cs[1].max_m;
    const size_t lds = ((size_t)(basis_words + n_dim) * BLOCK + head_doubles(group)) * sizeof(double);
    if (lds > 160 * 1024)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: the largest stage's outer bases, %d coordinates and the accumulators do not fit the LDS", who, n_dim);
    // the slot table: entry k is the k-th external coordinate (the slots other than V_cc's and I_B0's, in order)
    const int n_ext = n_dim - 2;
    if (n_ext > 0 && (!slot_row || !slot_log || !slot_a || !slot_w)) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL slot table", who);
    SlotMap sm;
    for (int c = 0; c < NIN; ++c) {
        sm.slot[c] = -1;
        sm.is_log[c] = 0;
        sm.a[c] = 0.0;
        sm.w[c] = 1.0;
    }
    for (int k = 0, d = 0; k < n_ext; ++k, ++d) {
        while (d == vcc_slot || d == ib0_slot) ++d;
        const int c = slot_row[k];
        if (c < 0 || c >= NIN || sm.slot[c] >= 0)
            return pem::fail(PEM_ERR_INVALID_ARG, "%s: slot_row[%d] = %d: the external slots read distinct input rows 0 .. %d", who, k, c, NIN - 1);
        if (!std::isfinite(slot_a[k]) || !std::isfinite(slot_w[k]) || !(slot_w[k] > 0.0))
            return pem::fail(PEM_ERR_INVALID_ARG, "%s: slot %d needs a finite a and a finite width w > 0", who, k);
        sm.slot[c] = d;
        sm.is_log[c] = slot_log[k] != 0;
        sm.a[c] = slot_a[k];
        sm.w[c] = slot_w[k];
    }
    for (int j = 0; j < n_varied(group); ++j)
        if (sm.slot[varied_input(group, j)] < 0)
            return pem::fail(PEM_ERR_INVALID_ARG, "%s: no slot reads input row %d, which the group varies", who, varied_input(group, j));
    if (int rc0 = pem::check_device()) return rc0;
    SobolArg s{};
    s.seed = seed;
    s.first = first_index;
    s.n = (long long)n_base;
    s.n_p = n_p;
    s.n_dim = n_dim;
    s.vcc_slot = vcc_slot;
    s.basis_words = basis_words;
    s.u_rank = u_rank;
    s.u_norm = u_norm;
    s.vcc_lo = vcc_lo;
    s.vcc_w = vcc_w;
    s.u_scale = u_scale;
    const double* ub = u_rank > 0 ? u_basis + (size_t)u_cell * u_rank : nullptr;
    const dim3 grid((unsigned)n_blocks, (unsigned)n_p);
    const hipStream_t st = static_cast<hipStream_t>(stream);
#define PEM_CSOBOL(G_, UW_, UE_) launch_chain_sobol<G_, UW_, UE_>(grid, lds, st, s, sm, cs, kind, a, b, ub, f_out, partial, flags)
    // thruster widths: 2 (no u_ion: its column is NaN), 3 exact (the test double's rank 1), 16 guarded (2 .. 14 latents): a stage's
    // columns are summed independently of each other, so the width changes no bit
    if (!thruster) PEM_CSOBOL(PEM_SWEEP_CATHODE, 2, true);
    else if (u_rank == 0) PEM_CSOBOL(PEM_SWEEP_THRUSTER, 2, true);
    else if (u_rank == 1) PEM_CSOBOL(PEM_SWEEP_THRUSTER, 3, true);
    else PEM_CSOBOL(PEM_SWEEP_THRUSTER, 16, false);
#undef PEM_CSOBOL
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}
