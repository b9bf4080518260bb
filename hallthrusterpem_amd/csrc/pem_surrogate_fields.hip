// pem_surrogate_fields.hip -- the component chain with the ion velocity carried through the thruster stage.
//
// A unit of its own so that pem_surrogate.hip's kernels and its compile time stay what they are: the stages, the coupling maps, the
// field rebuild and the j_ion node expression are THAT file's device code, compiled here a second time (it is included below with
// its own entry points left out; its node tables stay in one place), and only the kernels of this file are instantiated here.
#define PEM_SURROGATE_FIELDS_UNIT
#include "pem_surrogate.hip"

namespace {

// ---- u_ion through the chain: the thruster stage carries the SVD latents of its axial ion-velocity profile ------------------------
// scripts/pem_v0/pem_v0_SPT-100.yml:207-214 (`u_ion`: svd, linear(1e-3) norm, reconstruction_tol 0.01), train-shim.sh:9-11 (trained
// with the thruster component), mcmc.py:88-89 (`uion_reconstruct` inside the likelihood).  The thruster table has 2 + rank outputs:
// I_B0, T, then the latents.  Everything about u_ion happens between the thruster and the plume stage, so that the latents are dead
// when the widest stage starts: only the partial sum, V_cc, I_B0 and T stay live across it.  The stages, the coupling maps, the j_ion
// epilogue and the field rebuild are the parents' own helpers: a column of a stage is summed independently of the others, so that
// V_cc, I_B0, T and everything of the plume equal the parents' bits on the same tables.
struct ChainU {
    const double* basis;     // [dof][rank]
    const int32_t* node;     // likelihood: [n_node] grid indices, PEM_SYS_UION record p reads node[p], node[p + 1]
    double* field;           // predict: NULL or [n][dof]
    int rank, dof, norm, n_node;
    double scale;
};

// the u_basis row of node-table entry p: gathered once per workgroup (`rows`, [n_node][rank]) or through the cache; an entry is clamped
// into the grid (the entry point refuses the caller's host copy of a table that needs it)
__device__ __forceinline__ const double* uion_row(const ChainU& u, const double* rows, unsigned p) {
    if (rows) return rows + (size_t)p * u.rank;
    return u.basis + (size_t)min(max(u.node[p], 0), u.dof - 1) * u.rank;
}

// The u_ion records of sample i against the thruster stage's latents (`lat`: this thread's LDS slots, latent q at q * BLOCK): node
// values by jion_node's expression, m = fma(w, u[b] - u[a], u[a]) as system_epilogue_sum of the coupled kernel, p clamped as there.
// Returns the sum of the terms in record order, from 0: what chain_fields_epilogue goes on from.
__device__ __forceinline__ double chain_uion_sum(const ChainLik& lk, const ChainU& u, const double* rec, const int32_t* span,
                                                 const double* rows, const double* lat, long long i, bool store) {
#pragma clang fp contract(off)
    const long long d = i / lk.n_cond;
    const int c = (int)(i - d * lk.n_cond);
    const double4* r4 = reinterpret_cast<const double4*>(rec);
    const int2 ru = (reinterpret_cast<const int2*>(span) + 4 * c)[PEM_SYS_UION];
    double* prow = (lk.pred && store) ? lk.pred + (size_t)d * lk.ld_pred : nullptr;
    double ll = 0.0;
    if (u.n_node < 2) return ru.y > 0 ? __builtin_nan("") : ll;      // records without a node table (the host cannot see the spans)
    const unsigned pmax = (unsigned)(u.n_node - 2);
    for (int r = max(ru.x, 0); r < min(ru.x + ru.y, lk.n_rec); ++r) {
        const double4 e = r4[r];
        const unsigned p = min((unsigned)__double_as_longlong(e.w), pmax);
        const double ua = jion_node(lat, uion_row(u, rows, p), 0, u.rank, u.norm, u.scale);
        const double ub = jion_node(lat, uion_row(u, rows, p + 1), 0, u.rank, u.norm, u.scale);
        const double m = fma(e.x, ub - ua, ua);
        if (prow) prow[r] = m;
        const double z = (e.y - m) * e.z;
        ll = fma(-0.5 * z, z, ll);
    }
    return ll;
}

// twin of chain_loglik_epilogue (pem_surrogate.hip: a change there is made here too; the parent keeps its own copy so that none of
// its instantiations changes): the sum goes on from `ll`, the u_ion terms, and u_ion records are no longer something the chain cannot
// give.  Everything else -- the order j_ion, V_cc, T, discharge, the node reuse, pred -- is the parent's, expression for expression.
__device__ __forceinline__ void chain_fields_epilogue(const ChainLik& lk, const double* rec, const int32_t* span, const double* jb,
                                                      const double* lat, long long i, bool store, double V_cc, double I_B0, double T,
                                                      double ll) {
#pragma clang fp contract(off)
    const long long d = i / lk.n_cond;
    const int c = (int)(i - d * lk.n_cond);
    const double4* r4 = reinterpret_cast<const double4*>(rec);
    const int2* sp = reinterpret_cast<const int2*>(span) + 4 * c;
    const int2 rj = sp[PEM_SYS_JION], rv = sp[PEM_SYS_VCC], rt = sp[PEM_SYS_T];
    double* prow = (lk.pred && store) ? lk.pred + (size_t)d * lk.ld_pred : nullptr;
    if (jb) {
        int pk = -2;
        double lo = 0.0, hi = 0.0;
        for (int r = max(rj.x, 0); r < min(rj.x + rj.y, lk.n_rec); ++r) {
            const double4 e = r4[r];
            const int k = (int)min((unsigned)__double_as_longlong(e.w), 89u);
            if (k == pk + 1) {
                lo = hi;
                hi = jion_node(lat, jb, k + 1, lk.rank, lk.norm, lk.scale);
            } else if (k != pk) {
                lo = jion_node(lat, jb, k, lk.rank, lk.norm, lk.scale);
                hi = jion_node(lat, jb, k + 1, lk.rank, lk.norm, lk.scale);
            }
            pk = k;
            const double m = fma(e.x, hi - lo, lo);
            if (prow) prow[r] = m;
            const double z = (e.y - m) * e.z;
            ll = fma(-0.5 * z, z, ll);
        }
    }
    for (int r = max(rv.x, 0); r < min(rv.x + rv.y, lk.n_rec); ++r) {   // the cathode stage's coupling voltage
        const double4 e = r4[r];
        if (prow) prow[r] = V_cc;
        const double z = (e.y - V_cc) * e.z;
        ll = fma(-0.5 * z, z, ll);
    }
    for (int r = max(rt.x, 0); r < min(rt.x + rt.y, lk.n_rec); ++r) {   // the thruster stage's thrust T (not T_c)
        const double4 e = r4[r];
        if (prow) prow[r] = T;
        const double z = (e.y - T) * e.z;
        ll = fma(-0.5 * z, z, ll);
    }
    if (!jb && rj.y > 0) ll = __builtin_nan("");                        // j_ion records without a basis
    if (lk.a_1) {                                                       // I_d of the test double from the SURROGATE's I_B0 (mcmc.py:101)
        const double den = 1.0 - 2.0 * lk.a_1[i];
        const double i_d = I_B0 / den;
        const double z = (lk.discharge - i_d) * lk.inv_sigma;
        ll = fma(-0.5 * z, z, ll);
    }
    if (store) lk.loglik[i] = ll;
}

// out rows: sparse_chain_kernel's, then the thruster stage's latents (its outputs 2 .. n_out - 1)
template <int UW, bool UEXACT, int NOUT, bool EXACT>
__global__ __launch_bounds__(BLOCK) void fields_chain_kernel(long long n, int n_dim, int vcc_slot, int ib0_slot, ChainStage cat, ChainStage thr,
                                                             ChainStage plu, double vcc_lo, double vcc_w, double ib0_lo, double ib0_w,
                                                             const double* __restrict__ t, size_t ld, double* __restrict__ out,
                                                             size_t ld_out, int basis_words, Recon rc, Recon ru) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* basis = lds;                                    // every stage's outer bases in turn; between them: a field's latents [BLOCK][rank]
    double* coord = lds + (size_t)basis_words * BLOCK;      // [n_dim][BLOCK]: the external coordinates and the two coupling slots
    const int n_out = EXACT ? NOUT : plu.n_out;
    const int n_thr = UEXACT ? UW : thr.n_out;
    const int tid = threadIdx.x;
    const long long stride = (long long)gridDim.x * BLOCK;
    for (long long i0 = (long long)blockIdx.x * BLOCK; i0 < n; i0 += stride) {
        const long long i = i0 + tid < n ? i0 + tid : n - 1;        // a dead lane recomputes the last point and stores nothing
        for (int d = 0, r = 0; d < n_dim; ++d)
            if (d != vcc_slot && d != ib0_slot) coord[d * BLOCK + tid] = t[(size_t)(r++) * ld + i];
        double vcc[1], thrust[UW], plume[NOUT];
        stage_predict<1, true>(cat, coord, basis, tid, vcc);
        coord[vcc_slot * BLOCK + tid] = coupling_coord(vcc[0], vcc_lo, vcc_w);
        stage_predict<UW, UEXACT>(thr, coord, basis, tid, thrust);
        coord[ib0_slot * BLOCK + tid] = coupling_coord(thrust[0], ib0_lo, ib0_w);
        const double I_B0 = thrust[0], T = thrust[1];
        // the u_ion latents leave here: their rows, and the profile (every lane reaches the barriers: a dead lane has a point too)
        if (i0 + tid < n) {
#pragma unroll
            for (int o = 2; o < UW; ++o)
                if (UEXACT || o < n_thr) out[(size_t)(4 + n_out + o - 2) * ld_out + i] = thrust[o];
        }
        if (ru.field) rebuild_field<UW>(thrust, ru, lds, i0, n, tid);
        stage_predict<NOUT, EXACT>(plu, coord, basis, tid, plume);
        if (i0 + tid < n) {
            out[i] = vcc[0];
            out[ld_out + i] = I_B0;
            out[2 * ld_out + i] = T;
            out[3 * ld_out + i] = plume[0];
            out[4 * ld_out + i] = T * cos(plume[0]);
#pragma unroll
            for (int o = 1; o < NOUT; ++o)
                if (EXACT || o < n_out) out[(size_t)(4 + o) * ld_out + i] = plume[o];
        }
        if (rc.field) rebuild_field<NOUT>(plume, rc, lds, i0, n, tid);
    }
}

template <int UW, bool UEXACT, int NOUT, bool EXACT>
void launch_fields_chain(size_t n, int n_dim, int vcc_slot, int ib0_slot, const ChainStage (&s)[3], const double (&map)[4], const double* t,
                         size_t ld, double* out, size_t ld_out, int basis_words, const Recon& rc, const Recon& ru, hipStream_t st) {
    size_t blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > 256 * 8) blocks = 256 * 8;
    const size_t lds = (size_t)(basis_words + n_dim) * BLOCK * sizeof(double);
    if (lds > 64 * 1024) {
        static pem::LdsAttrOnce attr;
        (void)attr.ensure(reinterpret_cast<const void*>(fields_chain_kernel<UW, UEXACT, NOUT, EXACT>));      // a refusal shows as a launch error below
    }
    hipLaunchKernelGGL((fields_chain_kernel<UW, UEXACT, NOUT, EXACT>), dim3((unsigned)blocks), dim3(BLOCK), lds, st, (long long)n, n_dim,
                       vcc_slot, ib0_slot, s[0], s[1], s[2], map[0], map[1], map[2], map[3], t, ld, out, ld_out, basis_words, rc, ru);
}

// chain_loglik_kernel with the u_ion records served: their terms first (chain_uion_sum), then the parent's epilogue from that sum
// (chain_fields_epilogue)
template <int UW, bool UEXACT, int NOUT, bool EXACT>
__global__ __launch_bounds__(BLOCK) void fields_chain_loglik_kernel(long long n, int n_dim, int vcc_slot, int ib0_slot, ChainStage cat,
                                                                    ChainStage thr, ChainStage plu, double vcc_lo, double vcc_w, double ib0_lo,
                                                                    double ib0_w, const double* __restrict__ t, size_t ld, int basis_words,
                                                                    ChainLik lk, ChainU u) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* basis = lds;                                    // every stage's outer bases in turn; between them: this thread's latents [rank][BLOCK]
    double* coord = lds + (size_t)basis_words * BLOCK;      // [n_dim][BLOCK]
    const int n_out = EXACT ? NOUT : plu.n_out;
    const int n_thr = UEXACT ? UW : thr.n_out;
    const int tid = threadIdx.x;
    // the parent's tables, then the u_basis rows the node table names (gathered: a 200-cell basis stays out of LDS)
    const double* rec = lk.rec;
    const int32_t* span = lk.span;
    const double* jb = lk.basis;
    const double* urows = nullptr;
    if (lk.staged) {
        double* srec = coord + (size_t)n_dim * BLOCK;
        int32_t* sspan = reinterpret_cast<int32_t*>(srec + 4 * lk.n_rec);
        double* sjb = srec + 4 * lk.n_rec + 4 * lk.n_cond;
        double* srows = sjb + (lk.basis ? PEM_NANGLE * lk.rank : 0);
        for (int k = tid; k < 4 * lk.n_rec; k += BLOCK) srec[k] = lk.rec[k];
        for (int k = tid; k < 8 * lk.n_cond; k += BLOCK) sspan[k] = lk.span[k];
        if (lk.basis)
            for (int k = tid; k < PEM_NANGLE * lk.rank; k += BLOCK) sjb[k] = lk.basis[k];
        for (int k = tid; k < u.n_node * u.rank; k += BLOCK) srows[k] = uion_row(u, nullptr, (unsigned)(k / u.rank))[k % u.rank];
        __syncthreads();
        rec = srec;
        span = sspan;
        if (lk.basis) jb = sjb;
        urows = srows;
    }
    const long long stride = (long long)gridDim.x * BLOCK;
    for (long long i0 = (long long)blockIdx.x * BLOCK; i0 < n; i0 += stride) {
        const bool live = i0 + tid < n;
        const long long i = live ? i0 + tid : n - 1;        // a dead lane recomputes the last point and stores nothing
        for (int d = 0, r = 0; d < n_dim; ++d)
            if (d != vcc_slot && d != ib0_slot) coord[d * BLOCK + tid] = t[(size_t)(r++) * ld + i];
        // (each stage and both epilogues read and write this thread's own slots only: no barrier inside the loop)
        double vcc[1], thrust[UW], plume[NOUT];
        stage_predict<1, true>(cat, coord, basis, tid, vcc);
        coord[vcc_slot * BLOCK + tid] = coupling_coord(vcc[0], vcc_lo, vcc_w);
        stage_predict<UW, UEXACT>(thr, coord, basis, tid, thrust);
        coord[ib0_slot * BLOCK + tid] = coupling_coord(thrust[0], ib0_lo, ib0_w);
        const double I_B0 = thrust[0], T = thrust[1];
        // the u_ion latents leave the registers before the plume stage: their rows, then their records from the thread's basis slots
#pragma unroll
        for (int o = 2; o < UW; ++o)
            if (UEXACT || o < n_thr) {
                basis[(o - 2) * BLOCK + tid] = thrust[o];
                if (lk.out && live) lk.out[(size_t)(4 + n_out + o - 2) * lk.ld_out + i] = thrust[o];
            }
        const double ll = chain_uion_sum(lk, u, rec, span, urows, basis + tid, i, live);
        stage_predict<NOUT, EXACT>(plu, coord, basis, tid, plume);
        if (lk.out && live) {
            double* out = lk.out;
            const size_t ld_out = lk.ld_out;
            out[i] = vcc[0];
            out[ld_out + i] = I_B0;
            out[2 * ld_out + i] = T;
            out[3 * ld_out + i] = plume[0];
            out[4 * ld_out + i] = T * cos(plume[0]);
#pragma unroll
            for (int o = 1; o < NOUT; ++o)
                if (EXACT || o < n_out) out[(size_t)(4 + o) * ld_out + i] = plume[o];
        }
        if (lk.basis) {
#pragma unroll
            for (int o = 0; o < NOUT; ++o)
                if (o >= lk.lat0 && o < lk.lat0 + lk.rank) basis[(o - lk.lat0) * BLOCK + tid] = plume[o];
        }
        chain_fields_epilogue(lk, rec, span, jb, basis + tid, i, live, vcc[0], I_B0, T, ll);
    }
}

template <int UW, bool UEXACT, int NOUT, bool EXACT>
void launch_fields_chain_loglik(size_t n, int n_dim, int vcc_slot, int ib0_slot, const ChainStage (&s)[3], const double (&map)[4],
                                const double* t, size_t ld, int basis_words, size_t lds, const ChainLik& lk, const ChainU& u, hipStream_t st) {
    size_t blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > 256 * 8) blocks = 256 * 8;
    if (lds > 64 * 1024) {
        static pem::LdsAttrOnce attr;
        (void)attr.ensure(reinterpret_cast<const void*>(fields_chain_loglik_kernel<UW, UEXACT, NOUT, EXACT>));      // a refusal shows as a launch error below
    }
    hipLaunchKernelGGL((fields_chain_loglik_kernel<UW, UEXACT, NOUT, EXACT>), dim3((unsigned)blocks), dim3(BLOCK), lds, st, (long long)n, n_dim,
                       vcc_slot, ib0_slot, s[0], s[1], s[2], map[0], map[1], map[2], map[3], t, ld, basis_words, lk, u);
}

}  // namespace

namespace {

// what the two entry points that carry u_ion ask of its map (u_rank 0: none, nothing else is looked at)
int check_uion(const char* who, int u_lat0, int u_rank, int u_dof, int u_norm, double u_scale, const double* u_basis) {
    if (u_rank < 0 || u_rank > 14)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: 0 <= u_rank <= 14 (the thruster stage has 2 + u_rank <= 16 outputs)", who);
    if (u_rank == 0) return PEM_OK;
    if (u_lat0 != 2) return pem::fail(PEM_ERR_INVALID_ARG, "%s: the u_ion latents follow I_B0 and T: u_lat0 must be 2, got %d", who, u_lat0);
    if (!u_basis) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL u_basis with u_rank %d", who, u_rank);
    if (u_dof < 2) return pem::fail(PEM_ERR_INVALID_ARG, "%s: the u_ion grid needs u_dof >= 2 cells, got %d", who, u_dof);
    if (u_norm != PEM_NORM_NONE && u_norm != PEM_NORM_LOG10 && u_norm != PEM_NORM_LINEAR)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: unknown u_norm %d", who, u_norm);
    if (u_norm == PEM_NORM_LINEAR && !(std::isfinite(u_scale) && u_scale != 0.0))      // every node value is divided by it
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: the linear norm needs a finite u_scale != 0", who);
    return PEM_OK;
}

}  // namespace

// pem_surrogate_sobol.hip compiles this file's device code once more, as this file compiles pem_surrogate.hip's: the entry points
// below, and with them every kernel instantiation of this file, are left out of that unit
#ifndef PEM_SURROGATE_SOBOL_UNIT
namespace {

// Instantiations: thruster width 3 exact (the test double's profile is v_exh s(z): exactly rank 1) and 16 guarded (a plugged-in
// solver's 2 .. 14 latents); plume widths 1 exact (no j_ion), 8 and 16 guarded.  A stage's columns are summed independently of each
// other, so the width of an instantiation changes no bit of any output.
#define PEM_FIELDS_PLUME(LAUNCH, UW_, UE_) \
    (n_plume == 1 ? LAUNCH(UW_, UE_, 1, true) : (n_plume <= 8 ? LAUNCH(UW_, UE_, 8, false) : LAUNCH(UW_, UE_, 16, false)))

int predict_chain_fields(const char* who, size_t n, int n_dim, int vcc_slot, int ib0_slot, const pem_surr_stage* stages, double vcc_lo,
                         double vcc_w, double ib0_lo, double ib0_w, const double* t, size_t ld, double* out, size_t ld_out, const Recon& rc,
                         const Recon& ru, pem_stream_t stream) {
    ChainStage cs[3];
    int basis_words = 0;
    if (int rc0 = check_chain(who, n_dim, vcc_slot, ib0_slot, stages, vcc_lo, vcc_w, ib0_lo, ib0_w, cs, basis_words, 2 + ru.rank)) return rc0;
    const int n_plume = stages[2].n_out;
    if (rc.field && (rc.rank < 1 || rc.rank > 16 || rc.lat0 < 0 || rc.lat0 + rc.rank > n_plume || rc.dof < 1 || !rc.basis))
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: the reconstructed field takes 1 <= rank <= 16 latent outputs lat0 .. lat0 + rank - 1 of the plume stage", who);
    if (rc.field && rc.rank > basis_words) basis_words = rc.rank;
    if (ru.field && ru.rank > basis_words) basis_words = ru.rank;
    if ((size_t)(basis_words + n_dim) * BLOCK * sizeof(double) > 160 * 1024)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: the largest stage's outer bases and %d coordinates do not fit the LDS", who, n_dim);
    if (n == 0) return PEM_OK;
    if ((n_dim > 2 && !t) || !out) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL array", who);
    if ((n_dim > 2 && ld < n) || ld_out < n) return pem::fail(PEM_ERR_INVALID_ARG, "%s: leading dimension smaller than n", who);
    if (int rc0 = pem::check_device()) return rc0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double map[4] = {vcc_lo, vcc_w, ib0_lo, ib0_w};
#define PEM_FCHAIN(UW_, UE_, NOUT_, EXACT_) \
    launch_fields_chain<UW_, UE_, NOUT_, EXACT_>(n, n_dim, vcc_slot, ib0_slot, cs, map, t, ld, out, ld_out, basis_words, rc, ru, st)
    if (ru.rank == 1) PEM_FIELDS_PLUME(PEM_FCHAIN, 3, true);
    else PEM_FIELDS_PLUME(PEM_FCHAIN, 16, false);
#undef PEM_FCHAIN
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

int chain_fields_loglik(const char* who, size_t n, int n_dim, int vcc_slot, int ib0_slot, const pem_surr_stage* stages, double vcc_lo,
                        double vcc_w, double ib0_lo, double ib0_w, const double* t, size_t ld, int dof, double discharge_sigma, ChainLik lk,
                        ChainU u, pem_stream_t stream) {
    ChainStage cs[3];
    int basis_words = 0;
    if (int rc0 = check_chain(who, n_dim, vcc_slot, ib0_slot, stages, vcc_lo, vcc_w, ib0_lo, ib0_w, cs, basis_words, 2 + u.rank)) return rc0;
    if (u.rank > basis_words) basis_words = u.rank;                // the u_ion latents take the basis slots of their thread
    const int n_plume = stages[2].n_out;
    // (the parent's checks, pem_surrogate.hip chain_system_loglik)
    if (lk.basis) {
        if (lk.rank < 1 || lk.rank > 16 || lk.lat0 < 0 || lk.lat0 + lk.rank > n_plume)
            return pem::fail(PEM_ERR_INVALID_ARG, "%s: the j_ion map takes 1 <= rank <= 16 latent outputs lat0 .. lat0 + rank - 1 of the plume stage", who);
        if (dof != PEM_NANGLE) return pem::fail(PEM_ERR_INVALID_ARG, "%s: the j_ion records index the %d-point profile: dof must be %d, got %d", who, PEM_NANGLE, PEM_NANGLE, dof);
        if (lk.norm != PEM_NORM_NONE && lk.norm != PEM_NORM_LOG10 && lk.norm != PEM_NORM_LINEAR)
            return pem::fail(PEM_ERR_INVALID_ARG, "%s: unknown norm %d", who, lk.norm);
        if (lk.rank > basis_words) basis_words = lk.rank;
    }
    const size_t base = (size_t)(basis_words + n_dim) * BLOCK * sizeof(double);
    if (base > 160 * 1024)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: the largest stage's outer bases and %d coordinates do not fit the LDS", who, n_dim);
    if (lk.n_cond < 1 || lk.n_cond > PEM_FUSED_SYSTEM_MAX_RECORDS || lk.n_rec < 1 || lk.n_rec > PEM_FUSED_SYSTEM_MAX_RECORDS)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: 1 .. %d conditions and records (PEM_FUSED_SYSTEM_MAX_RECORDS)", who, PEM_FUSED_SYSTEM_MAX_RECORDS);
    if (lk.a_1 && !(std::isfinite(discharge_sigma) && discharge_sigma > 0.0))
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: the discharge term needs a finite discharge_sigma > 0", who);
    if (n == 0) return PEM_OK;
    if ((n_dim > 2 && !t) || !lk.rec || !lk.span || !lk.loglik) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL array", who);
    if ((n_dim > 2 && ld < n) || (lk.out && lk.ld_out < n)) return pem::fail(PEM_ERR_INVALID_ARG, "%s: leading dimension smaller than n", who);
    if (lk.pred && lk.ld_pred < (size_t)lk.n_rec) return pem::fail(PEM_ERR_INVALID_ARG, "%s: ld_pred smaller than n_rec", who);
    if (int rc0 = pem::check_device()) return rc0;
    lk.inv_sigma = lk.a_1 ? 1.0 / discharge_sigma : 0.0;
    // the parent's policy: everything beside the coordinates where that costs no resident workgroup, else everything through the cache;
    // of u_basis only the rows the node table names
    const size_t extra = (size_t)lk.n_rec * 32 + (size_t)lk.n_cond * 32 + (lk.basis ? (size_t)PEM_NANGLE * lk.rank * sizeof(double) : 0) +
                         (size_t)u.n_node * u.rank * sizeof(double);
    const size_t room = base <= 80 * 1024 ? 80 * 1024 : 160 * 1024;
    lk.staged = base + extra <= room;
    const size_t lds = base + (lk.staged ? extra : 0);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double map[4] = {vcc_lo, vcc_w, ib0_lo, ib0_w};
#define PEM_FCHAIN_LL(UW_, UE_, NOUT_, EXACT_) \
    launch_fields_chain_loglik<UW_, UE_, NOUT_, EXACT_>(n, n_dim, vcc_slot, ib0_slot, cs, map, t, ld, basis_words, lds, lk, u, st)
    if (u.rank == 1) PEM_FIELDS_PLUME(PEM_FCHAIN_LL, 3, true);
    else PEM_FIELDS_PLUME(PEM_FCHAIN_LL, 16, false);
#undef PEM_FCHAIN_LL
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

}  // namespace

extern "C" {

int pem_sparse_predict_chain_fields_f64_dev(size_t n, int n_dim, int vcc_slot, int ib0_slot, const pem_surr_stage* stages, double vcc_lo,
                                            double vcc_w, double ib0_lo, double ib0_w, const double* t, size_t ld, double* out, size_t ld_out,
                                            int lat0, int rank, int dof, int norm, double norm_scale, const double* basis, double* field,
                                            int u_lat0, int u_rank, int u_dof, int u_norm, double u_scale, const double* u_basis,
                                            double* u_field, pem_stream_t stream) {
    const char* who = "pem_sparse_predict_chain_fields";
    if (int rc0 = check_uion(who, u_lat0, u_rank, u_dof, u_norm, u_scale, u_basis)) return rc0;
    if (u_rank == 0)                                    // bit contract 1: the parent's kernels
        return pem_sparse_predict_chain_f64_dev(n, n_dim, vcc_slot, ib0_slot, stages, vcc_lo, vcc_w, ib0_lo, ib0_w, t, ld, out, ld_out, lat0,
                                                rank, dof, norm, norm_scale, basis, field, stream);
    const Recon ru{u_basis, u_field, u_dof, u_rank, u_lat0, u_norm, u_scale};
    Recon rc{};
    if (field) {
        if (norm != PEM_NORM_NONE && norm != PEM_NORM_LOG10 && norm != PEM_NORM_LINEAR)
            return pem::fail(PEM_ERR_INVALID_ARG, "%s: unknown norm %d", who, norm);
        rc = Recon{basis, field, dof, rank, lat0, norm, norm_scale};
    }
    return predict_chain_fields(who, n, n_dim, vcc_slot, ib0_slot, stages, vcc_lo, vcc_w, ib0_lo, ib0_w, t, ld, out, ld_out, rc, ru, stream);
}

int pem_chain_fields_loglik_f64_dev(size_t n, int n_dim, int vcc_slot, int ib0_slot, const pem_surr_stage* stages, double vcc_lo,
                                    double vcc_w, double ib0_lo, double ib0_w, const double* t, size_t ld, int lat0, int rank, int dof,
                                    int norm, double norm_scale, const double* basis, int n_cond, int n_rec, const double* rec,
                                    const int32_t* span, const double* a_1, double discharge_current, double discharge_sigma,
                                    double* loglik, double* out, size_t ld_out, double* pred, size_t ld_pred, int u_lat0, int u_rank,
                                    int u_dof, int u_norm, double u_scale, const double* u_basis, int n_node, const int32_t* node,
                                    const int32_t* node_host, pem_stream_t stream) {
    const char* who = "pem_chain_fields_loglik";
    if (int rc0 = check_uion(who, u_lat0, u_rank, u_dof, u_norm, u_scale, u_basis)) return rc0;
    if (n_node < 0 || n_node > 2 * PEM_FUSED_SYSTEM_MAX_RECORDS)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: 0 <= n_node <= %d (2 PEM_FUSED_SYSTEM_MAX_RECORDS)", who, 2 * PEM_FUSED_SYSTEM_MAX_RECORDS);
    if (u_rank == 0)                                    // bit contract 1: the parent's kernels (u_ion records give NaN)
        return pem_chain_system_loglik_f64_dev(n, n_dim, vcc_slot, ib0_slot, stages, vcc_lo, vcc_w, ib0_lo, ib0_w, t, ld, lat0, rank, dof, norm,
                                               norm_scale, basis, n_cond, n_rec, rec, span, a_1, discharge_current, discharge_sigma, loglik,
                                               out, ld_out, pred, ld_pred, stream);
    ChainU u{};
    if (n_node == 1) return pem::fail(PEM_ERR_INVALID_ARG, "%s: a u_ion record reads node[p] and node[p + 1]: n_node is 0 (no such records) or >= 2", who);
    if (n_node > 0 && (!node || !node_host)) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL node table (the device array and the caller's host copy of it)", who);
    for (int k = 0; k < n_node; ++k)
        if (node_host[k] < 0 || node_host[k] >= u_dof)
            return pem::fail(PEM_ERR_INVALID_ARG, "%s: node[%d] = %d is outside the u_ion grid of %d cells", who, k, (int)node_host[k], u_dof);
    u.basis = u_basis;
    u.node = node;
    u.rank = u_rank;
    u.dof = u_dof;
    u.norm = u_norm;
    u.n_node = n_node;
    u.scale = u_scale;
    ChainLik lk{};
    lk.basis = basis;
    lk.rec = rec;
    lk.span = span;
    lk.a_1 = a_1;
    lk.loglik = loglik;
    lk.out = out;
    lk.pred = pred;
    lk.ld_out = ld_out;
    lk.ld_pred = ld_pred;
    lk.lat0 = lat0;
    lk.rank = basis ? rank : 0;
    lk.norm = norm;
    lk.n_cond = n_cond;
    lk.n_rec = n_rec;
    lk.scale = norm_scale;
    lk.discharge = discharge_current;
    return chain_fields_loglik(who, n, n_dim, vcc_slot, ib0_slot, stages, vcc_lo, vcc_w, ib0_lo, ib0_w, t, ld, dof, discharge_sigma, lk, u, stream);
}

}  // extern "C"
#endif  // PEM_SURROGATE_SOBOL_UNIT
