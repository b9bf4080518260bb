/*
 * pem_hip.h -- C ABI of libpem_hip.so: the MI355X (gfx950) batched evaluator for the PEM-v0
 * cathode -> thruster -> plume sub-models of JANUS-Institute/HallThrusterPEM (hallmd 0.3.0).
 *
 * Every entry point replaces one vectorised Python model callable of the reference (paths are
 * relative to the upstream repository root).  The reference has no FFI of its own -- its models
 * are NumPy functions called as  model(inputs: dict[str, ndarray]) -> dict[str, ndarray]  by amisc
 * (scripts/pem_v0/pem_v0_SPT-100.yml:6,63,216) -- so the boundary is drawn one level below that
 * call: plain fp64 SoA buffers, one value per Monte-Carlo sample, caller-owned outputs.
 *
 *   pem_cathode_f64*    src/hallmd/models/cathode.py:16-38      cathode_coupling()
 *   pem_plume_f64*      src/hallmd/models/plume.py:21-159       current_density()
 *   pem_thruster_f64*   tests/sim_hallthruster.jl:35-48         the reference's analytic stand-in
 *                        for HallThruster.jl (a TEST DOUBLE of the thruster stage; the 1-D fluid
 *                        solver itself is a third-party Julia program and out of scope)
 *   pem_coupled_f64*    the three stages fused, wired as pem_v0_SPT-100.yml wires the components
 *                        (V_cc: cathode -> thruster; I_B0: thruster -> plume; T -> T_c)
 *
 * Conventions
 *   - All arrays are contiguous fp64 of length n (one entry per sample) unless stated.
 *   - `*_dev` functions take DEVICE pointers (HBM of the current HIP device) and enqueue on
 *     `stream` (a hipStream_t passed as void*; NULL = the default stream) without synchronising.
 *     Functions without the suffix take HOST pointers, stage through device memory and return
 *     after the results are back in the caller's buffers (calls of up to 256 KB of arrays: the
 *     kernels work on a pinned host buffer directly, without the two copies).
 *   - Nothing is retained past the call.  Inputs are never written.
 *   - j_ion is laid out [n][91][n_radii] (row-major), exactly numpy's (..., 91, R) result of
 *     plume.py:102; angle k is k degrees from the thruster centreline (plume.py:53).
 *   - Physics failures are data, not errors, as in the reference: an invalid plume sample
 *     (alpha1 <= 0 or any j_ion <= 0, plume.py:105) has its j_ion row set to 1e-20 and, if
 *     `invalid` is non-NULL, invalid[i] = 1.  NaN inputs propagate.
 *   - `torr2pa` is pem_core.constants.TORR_2_PA, which the reference imports from an
 *     un-vendored package (cathode.py:10, plume.py:12); it is a run-time argument here.
 *   - Return value: PEM_OK or a PEM_ERR_* code; pem_last_error() describes the last failure on
 *     the calling thread.  There is no CPU fallback: without a HIP device every compute entry
 *     point fails with PEM_ERR_NO_DEVICE.
 */
#ifndef PEM_HIP_H
#define PEM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PEM_NANGLE 91 /* points of the fixed 0..90 degree sweep, plume.py:53 */

#define PEM_OK 0
#define PEM_ERR_INVALID_ARG 1
#define PEM_ERR_HIP 2
#define PEM_ERR_NO_DEVICE 3

typedef void* pem_stream_t; /* hipStream_t */

/* ---- library state ------------------------------------------------------------------------- */
const char* pem_version(void);
const char* pem_last_error(void);
int pem_device_count(void);                 /* number of HIP devices, 0 if none / no driver        */
/* hipSetDevice(device) and make it the process default of the host-pointer entry points, whichever thread calls them
 * (without pem_init they run on the calling thread's current device).  The *_dev entry points follow their stream. */
int pem_init(int device);
int pem_synchronize(pem_stream_t stream);   /* hipStreamSynchronize                                */
/* Tuning knob of the plume/coupled kernels: lanes that share one sample (2, 4 or 8).
 * 0 restores the default.  Returns the value in effect. */
int pem_set_lanes_per_sample(int lanes);
/* The 91-point angle grid (host memory, valid for the life of the library): j_ion_coords.    */
const double* pem_angle_grid(void);
/* Launch geometry of the persistent coupled kernel, for callers that cut one GPU's shard into range launches (the
 * multi-GPU pipeline of SURVEY.md section 8e; the reference's only parallel call site is the executor.map of
 * scripts/gen_data.py:448-460, which has no notion of a launch).  A persistent wave walks 64-sample tiles
 * w, w + waves, ...: a range that is a whole number of `samples_per_round` leaves no wave slot idle in its last round.
 * pem_persistent_grid is pure arithmetic (no device needed): the workgroups a launch over n samples takes on a device
 * with `cus` compute units holding `wg_per_cu` workgroups each (memory_bound, the profile-writing modes: balanced rounds
 * up to three rounds of work, beyond that a one-shot grid of one tile per wave that the dispatcher deals out) and the
 * samples the workgroups resident at one time cover.  pem_coupled_occupancy reports `cus` and `wg_per_cu` of
 * pem_coupled_f64_dev (profile_mode 1), pem_coupled_mixed_dev (2) or the reduced-QoI launch (0, j_ion == NULL) on the
 * calling thread's current device.                                                                                    */
int pem_persistent_grid(size_t n, int cus, int wg_per_cu, int memory_bound, size_t* workgroups, size_t* samples_per_round);
int pem_coupled_occupancy(int profile_mode, int* cus, int* wg_per_cu);

/* ---- cathode_coupling  (cathode.py:16-38) --------------------------------------------------- */
int pem_cathode_f64_dev(size_t n, const double* P_b, const double* V_a, const double* T_e,
                        const double* V_vac, const double* Pstar, const double* P_T, double torr2pa,
                        double* V_cc, pem_stream_t stream);
int pem_cathode_f64(size_t n, const double* P_b, const double* V_a, const double* T_e,
                    const double* V_vac, const double* Pstar, const double* P_T, double torr2pa,
                    double* V_cc);

/* ---- current_density  (plume.py:21-159) ------------------------------------------------------
 * radii: HOST array of n_radii sweep radii in metres (the `sweep_radius` argument), also for the
 * _dev form (up to 256 radii travel in the kernel arguments; beyond that, and for one radius with a j_ion that is not
 * 16-byte aligned, the _dev form copies them and waits for the stream before returning).  T / T_c: optional thrust
 * in, corrected thrust out (plume.py:136-140); pass NULL for
 * both to skip.  j_ion: [n][91][n_radii]; div_angle, T_c: [n][n_radii]; invalid: [n] or NULL.   */
int pem_plume_f64_dev(size_t n, int n_radii, const double* radii, double torr2pa, const double* P_b,
                      const double* c0, const double* c1, const double* c2, const double* c3,
                      const double* c4, const double* c5, const double* sigma_cex, const double* I_B0,
                      const double* T, double* j_ion, double* div_angle, double* T_c, uint8_t* invalid,
                      pem_stream_t stream);
int pem_plume_f64(size_t n, int n_radii, const double* radii, double torr2pa, const double* P_b,
                  const double* c0, const double* c1, const double* c2, const double* c3,
                  const double* c4, const double* c5, const double* sigma_cex, const double* I_B0,
                  const double* T, double* j_ion, double* div_angle, double* T_c, uint8_t* invalid);

/* ---- analytic thruster stage  (tests/sim_hallthruster.jl:35-48; a test double) ---------------
 * Any output pointer may be NULL.                                                              */
int pem_thruster_f64_dev(size_t n, const double* V_a, const double* V_cc, const double* mdot_a,
                         const double* a_1, double* I_B0, double* I_d, double* T, double* eta_c,
                         double* eta_m, double* eta_v, double* eta_a, double* v_exh, pem_stream_t stream);
int pem_thruster_f64(size_t n, const double* V_a, const double* V_cc, const double* mdot_a,
                     const double* a_1, double* I_B0, double* I_d, double* T, double* eta_c,
                     double* eta_m, double* eta_v, double* eta_a, double* v_exh);

/* u_ion(z) = v_exh / (1 + exp(-100 (z - 0.04))) on z = range(z0, z1, length = ncells)  (sim_hallthruster.jl:46-47).
 * z: [ncells] device array or NULL; u_ion: [n][ncells].                                               */
int pem_thruster_uion_f64_dev(size_t n, const double* v_exh, double z0, double z1, int ncells, double* z,
                              double* u_ion, pem_stream_t stream);
/* The two post-run filters of hallthruster_jl (thruster.py:490-502), batched.  flags[i] bit 0: T < 0 or
 * I_B0 < 0 (the reference raises "non-physical case"); bit 1 (only if use_shock): z[argmax(u_ion[i])] <
 * shock_threshold (the reference raises "shock-like behavior").  T / I_B0 may be NULL (treated as 0).  */
int pem_thruster_filter_f64_dev(size_t n, int ncells, const double* u_ion, const double* z, double shock_threshold,
                                int use_shock, const double* T, const double* I_B0, uint8_t* flags,
                                pem_stream_t stream);

/* ---- coupled cathode -> thruster -> plume, one pass, sweep radius `radius` (R = 1) -----------
 * 15 inputs per sample; outputs V_cc, div_angle, T_c always; I_B0, T, invalid optional (NULL);
 * j_ion optional: NULL selects the reduced-QoI mode that never writes the 91-point profile (and takes the two
 * divergence integrals of plume.py:117-123 from tables of the beam width where that is exact to rounding, so its
 * div_angle / T_c agree with the profile mode's to ~1e-13 relative rather than bit for bit).                      */
int pem_coupled_f64_dev(size_t n, double torr2pa, double radius, const double* P_b, const double* V_a,
                        const double* T_e, const double* V_vac, const double* Pstar, const double* P_T,
                        const double* mdot_a, const double* a_1, const double* c0, const double* c1,
                        const double* c2, const double* c3, const double* c4, const double* c5,
                        const double* sigma_cex, double* V_cc, double* I_B0, double* T, double* j_ion,
                        double* div_angle, double* T_c, uint8_t* invalid, pem_stream_t stream);
int pem_coupled_f64(size_t n, double torr2pa, double radius, const double* P_b, const double* V_a,
                    const double* T_e, const double* V_vac, const double* Pstar, const double* P_T,
                    const double* mdot_a, const double* a_1, const double* c0, const double* c1,
                    const double* c2, const double* c3, const double* c4, const double* c5,
                    const double* sigma_cex, double* V_cc, double* I_B0, double* T, double* j_ion,
                    double* div_angle, double* T_c, uint8_t* invalid);

/* ---- how the host-pointer entry points move their data ---------------------------------------------------------------
 * pem_cathode_f64, pem_thruster_f64, pem_plume_f64 and pem_coupled_f64 cut a call into chunks of `chunk` samples and carve
 * one chunk's arrays, each padded to 256 bytes, from a workspace: the inputs first (they end at byte `in_end`), the outputs
 * after them (they end at `footprint`).
 *   chunk      cathode, thruster: min(n, 2^24).  plume: max(1024, 2^28 / (91 n_radii 8)), at most n, rounded up to 64.
 *              coupled: 2^28 / (91 * 8), at most n, rounded up to 64.
 *   reserve    bytes of workspace the call asks for: the footprint, except that the thruster stage always asks for room for
 *              all eight outputs while its footprint counts only the n_optional outputs that are not NULL.  n_optional is read
 *              for PEM_HOST_THRUSTER only (0 .. 8); the optional arrays of the plume and of the coupled model keep their place.
 *   regime     0  reserve <= 256 KiB and the environment does not say PEM_ZERO_COPY=0 (read once per process): the kernels
 *                 work on a pinned host buffer, nothing is copied by the device
 *              1  footprint <= 2 MiB: one copy in and one copy out through a pinned mirror of the layout
 *              2  in_end <= 2 MiB < footprint: one copy in for the inputs, the outputs array by array
 *              3  one copy per array
 * pem_host_plan is pure arithmetic (no device needed) and is the code the four entry points take their chunk, layout and
 * regime from.  Refused (PEM_ERR_INVALID_ARG): an unknown entry, n == 0, n_radii < 1 (pass 1 where there are no radii),
 * n_optional outside 0 .. 8 for the thruster stage, a NULL result pointer.
 * pem_host_last_regime(): the regime the last chunk of the calling thread's last host-pointer call really used, -1 before
 * the first; a refused call leaves it alone.  It differs from the plan only when the pinned buffer could not be allocated
 * (then 3).                                                                                                              */
#define PEM_HOST_CATHODE 0
#define PEM_HOST_THRUSTER 1
#define PEM_HOST_PLUME 2
#define PEM_HOST_COUPLED 3
int pem_host_plan(int entry, size_t n, int n_radii, int n_optional, size_t* chunk, size_t* n_chunks, size_t* in_end,
                  size_t* footprint, size_t* reserve, int* regime);
int pem_host_last_regime(void);

/* The same evaluation with the 15 inputs TILE-INTERLEAVED: x_tiled is [ceil(n / 64)][15][64] doubles -- for every 64-sample
 * tile of the kernel the 15 rows (order of pem_coupled_f64_dev's arguments: P_b V_a T_e V_vac Pstar P_T mdot_a a_1 c0..c5
 * sigma_cex) sit in one contiguous 7680-byte block, so a wave reads ONE block per tile instead of 512 bytes from each of 15
 * arrays.  A second layout of the same `dict of arrays` the reference's callables take (cathode.py:26-31, plume.py:40-49);
 * pem_sample_tiled_f64_dev writes it directly.  Results are bit-identical to pem_coupled_f64_dev.  Device pointers only. */
int pem_coupled_tiled_f64_dev(size_t n, double torr2pa, double radius, const double* x_tiled, double* V_cc, double* I_B0,
                              double* T, double* j_ion, double* div_angle, double* T_c, uint8_t* invalid,
                              pem_stream_t stream);

/* Mixed precision (BASELINE.json configs[4], "fp64 -> fp32 mixed with tolerance check"): identical fp64
 * arithmetic; only the 91-point profile is rounded once to fp32 when it is stored (j_ion_f32: [n][91]
 * floats, 16-byte aligned).  508 instead of 872 algorithmic bytes per evaluation.  Device pointers only.  */
int pem_coupled_mixed_dev(size_t n, double torr2pa, double radius, const double* P_b, const double* V_a,
                          const double* T_e, const double* V_vac, const double* Pstar, const double* P_T,
                          const double* mdot_a, const double* a_1, const double* c0, const double* c1,
                          const double* c2, const double* c3, const double* c4, const double* c5,
                          const double* sigma_cex, double* V_cc, double* I_B0, double* T, float* j_ion_f32,
                          double* div_angle, double* T_c, uint8_t* invalid, pem_stream_t stream);

/* ---- input samplers ------------------------------------------------------------------------------
 * Stand in for `system.sample_inputs(N, ...)` (scripts/gen_data.py:238; scripts/pem_v0/sobol.py:46-66,
 * monte_carlo.py:63-300).  amisc/uqtils are third-party and absent from the reference tree: parity is
 * UNPINNED, the formulas are this library's own (see csrc/pem_sampler.hip).
 * Counter-based (Philox4x32-10): out[d][i] depends only on (seed, stream_id, first_index + i, d), so
 * any sharding / batching of a design yields the same design.  out is SoA: row d at out + d*ld, ld >= n.
 * kind/a/b are HOST arrays of length ndim (<= PEM_SAMPLE_MAX_DIM):
 *   PEM_DIST_UNIFORM     a + (b-a) u            PEM_DIST_LOGUNIFORM  10^(a + (b-a) u)  (a, b = log10 bounds)
 *   PEM_DIST_NORMAL      a + b Phi^-1(u)  (mean a, standard deviation b)
 * swap_dim builds Saltelli blocks: -1 plain (matrix A), -2 every dimension from stream_id+1 (matrix B),
 * d >= 0 matrix A with column d taken from B.
 * pem_sample_lhs_f64_dev: Latin hypercube over n_total strata per dimension (keyed Feistel permutation
 * of the stratum index + jitter); samples first_index .. first_index+n-1 of that design.             */
#define PEM_SAMPLE_MAX_DIM 32
#define PEM_DIST_UNIFORM 0
#define PEM_DIST_LOGUNIFORM 1
#define PEM_DIST_NORMAL 2
int pem_sample_f64_dev(size_t n, uint64_t first_index, uint64_t seed, uint32_t stream_id, int ndim,
                       const int32_t* kind, const double* a, const double* b, int swap_dim, double* out,
                       size_t ld, pem_stream_t stream);
int pem_sample_lhs_f64_dev(size_t n, uint64_t first_index, uint64_t n_total, uint64_t seed, uint32_t stream_id,
                           int ndim, const int32_t* kind, const double* a, const double* b, double* out,
                           size_t ld, pem_stream_t stream);
/* pem_sample_f64_dev's numbers in the tile-interleaved layout of pem_coupled_tiled_f64_dev: out is
 * [ceil(n / 64)][ndim][64] (sample i of the call at out[(i / 64) * ndim * 64 + d * 64 + i % 64]).             */
int pem_sample_tiled_f64_dev(size_t n, uint64_t first_index, uint64_t seed, uint32_t stream_id, int ndim,
                             const int32_t* kind, const double* a, const double* b, int swap_dim, double* out,
                             pem_stream_t stream);

/* The low-discrepancy design (csrc/pem_qmc.hip): a Sobol' sequence with a random digital shift, for the same kind/a/b table.
 *   x(i, d) = XOR over the set bits j of gray(i) = i ^ (i >> 1) of v[d][j]      (30-bit Joe-Kuo direction numbers, the ones
 *             torch.quasirandom.SobolEngine and scipy.stats.qmc.Sobol(bits=30) use; left-aligned to bit 29)
 *   u(i, d) = ((x ^ s_d) + 0.5) 2^-30     the midpoint of the point's cell: exact in fp64, never 0 or 1 (Phi^-1 stays finite);
 *             for a U(0, 1) prior and scramble == 0 it is SobolEngine's draw + 2^-31, bit for bit
 *   s_d     = 0 if scramble == 0, else the top 30 bits of the first word of Philox4x32-10 with counter (d, 0, 0x534F424C,
 *             stream_id) and key seed: one shift per sequence dimension, never a block of a Monte-Carlo or Latin-hypercube stream
 * out[d][i] = transform_d(u(first_index + i, d)): a pure function of (seed, stream_id, index, dimension), no running state, so any
 * sharding of a design is the same design.  swap_dim as for pem_sample_f64_dev, with matrix B = sequence dimensions
 * ndim .. 2 ndim - 1 of the same points (the usual quasi-Monte-Carlo Saltelli construction).
 * Refused (PEM_ERR_INVALID_ARG) before any device call: ndim outside [1, PEM_SAMPLE_MAX_DIM]; swap_dim != -1 with
 * 2 ndim > PEM_SAMPLE_MAX_DIM; first_index + n > 2^30 (the sequence has 2^30 points); a NULL array; an unknown kind; ld < n.
 * pem_sobol_directions copies the 30 direction numbers of dimension dim (0 .. 31) to out30: host only, touches no device.   */
int pem_sobol_directions(int dim, uint32_t* out30);
int pem_sample_sobol_f64_dev(size_t n, uint64_t first_index, uint64_t seed, uint32_t stream_id, int scramble, int ndim,
                             const int32_t* kind, const double* a, const double* b, int swap_dim, double* out,
                             size_t ld, pem_stream_t stream);

/* Predictive checks (scripts/pem_v0/monte_carlo.py:42-60,63-300; hallthrusterpem_amd/predictive.py).
 * pem_predictive_inputs_f64_dev fills the [15][ld] SoA inputs (COUPLED_INPUTS order) of n samples, sample i belonging to
 * condition c = i mod n_cond: every input starts as draw first_index + i of the design (pem_sample_f64_dev's numbers for
 * seed, stream_id, kind/a/b: HOST arrays of 15), then rows P_b, V_a, mdot_a become operating[c][0..2] (DEVICE [n_cond][3]) and,
 * when samples (DEVICE [n_samples][n_theta]) is not NULL, row theta_rows[j] (HOST [n_theta]) becomes samples[idx_i][j] with
 *   idx_i = (x * n_samples) >> 32,   x = word 0 of Philox4x32-10(counter = (g_lo, g_hi, 0, theta_stream), key = seed), g = first_index + i
 * (PEM_PREDICTIVE_THETA_INDEX; 1 <= n_samples < 2^32): theta drawn with replacement, independently for every sample.  With
 * samples NULL the theta rows keep the prior draw (the prior predictive).
 * pem_predictive_noise_f64_dev: out[s][j] = pred[s][j] + sigma[j] Phi^-1(u53(w0, w1)), (w0, w1) words 0, 1 of
 * Philox4x32-10(counter = (g_lo, g_hi, j, stream_id), key = seed), g = first_row + s; pred, out [n_rows][ld], sigma DEVICE [m]. */
int pem_predictive_inputs_f64_dev(size_t n, int n_cond, uint64_t first_index, uint64_t seed, uint32_t stream_id,
                                  const int32_t* kind, const double* a, const double* b, const double* operating,
                                  const double* samples, size_t n_samples, int n_theta, const int32_t* theta_rows,
                                  uint32_t theta_stream, double* out, size_t ld, pem_stream_t stream);
int pem_predictive_noise_f64_dev(size_t n_rows, int m, const double* pred, size_t ld_pred, const double* sigma,
                                 uint64_t first_row, uint64_t seed, uint32_t stream_id, double* out, size_t ld_out,
                                 pem_stream_t stream);

/* Saltelli accumulation for the Sobol' estimators (uq.sobol_sa at scripts/pem_v0/sobol.py:113 -- uqtils, third-party,
 * parity UNPINNED; estimators stated in hallthrusterpem_amd/drivers.py).  fA / fB / fAB: [nq][ld] QoI rows of the
 * A, B and AB_d blocks (fAB NULL for the mean/variance sums).  partial: [n_blocks][nq][2], one deterministic partial
 * sum per workgroup: {sum fA+fB, sum fA^2+fB^2} or {sum fB (fAB-fA), sum (fA-fAB)^2}.  nq <= 8.                    */
int pem_sobol_partial_f64_dev(size_t m, int nq, size_t ld, const double* fA, const double* fB, const double* fAB,
                              double* partial, int n_blocks, pem_stream_t stream);

/* ---- likelihood of measured ion current density (scripts/pem_v0/mcmc.py:57-106, `jion` branch; the mirrored
 * linear interpolation of monte_carlo.py:265-270 / plume.py:142-149).  The scripts are stale and untested in the
 * reference: parity UNPINNED; formula in csrc/pem_likelihood.hip.  Sample i belongs to condition i mod n_cond.
 * kidx/weight/y/inv_std: [n_cond][n_ang] device arrays (k in [0, 89], weight in [0, 1]), at most
 * PEM_LOGLIK_MAX_MEASUREMENTS entries; loglik: [n].                                                          */
#define PEM_LOGLIK_MAX_MEASUREMENTS 4096
int pem_jion_loglik_f64_dev(size_t n, int n_cond, int n_ang, const int32_t* kidx, const double* weight,
                            const double* y, const double* inv_std, const double* j_ion, double* loglik,
                            pem_stream_t stream);

/* pem_coupled_f64_dev + pem_jion_loglik_f64_dev in one launch: the 91-point profile is staged in LDS, reduced against
 * the measurements there and never written (152 bytes per evaluation).  Same per-sample results as the two-launch
 * pipeline up to the summation order of the partial sums.  n_cond * (n_ang | 1) <= PEM_FUSED_LOGLIK_MAX_MEASUREMENTS
 * (LDS table).                                                                                                       */
#define PEM_FUSED_LOGLIK_MAX_MEASUREMENTS 1024
int pem_coupled_loglik_f64_dev(size_t n, double torr2pa, double radius, const double* P_b, const double* V_a,
                               const double* T_e, const double* V_vac, const double* Pstar, const double* P_T,
                               const double* mdot_a, const double* a_1, const double* c0, const double* c1,
                               const double* c2, const double* c3, const double* c4, const double* c5,
                               const double* sigma_cex, int n_cond, int n_ang, const int32_t* kidx,
                               const double* weight, const double* y, const double* inv_std, double* V_cc,
                               double* div_angle, double* T_c, double* loglik, uint8_t* invalid, pem_stream_t stream);

/* pem_coupled_f64_dev + the Gaussian log-likelihood of several measured quantities in one launch -- the `System` calibration of
 * the reference (scripts/pem_v0/mcmc.py:28-45,57-104, QOIS = V_cc, T, uion, jion; its driver layer is stale and third-party:
 * parity UNPINNED, held to the oracle + numpy).  Sample i belongs to condition i mod n_cond; loglik[i] is the sum over that
 * condition's records of -0.5 z^2, z = (y - model) / std:
 *   PEM_SYS_JION  {w, y, 1/std, k}  model = fma(w, j[k+1] - j[k], j[k]) on the 91-point profile (k an int64 bit pattern < 90):
 *                                   pem_coupled_loglik_f64_dev's term, on the profile staged in LDS
 *   PEM_SYS_VCC   {0, y, 1/std, 0}  model = the clipped cathode coupling voltage V_cc
 *   PEM_SYS_T     {0, y, 1/std, 0}  model = the thruster test double's thrust T (not the plume's T_c)
 *   PEM_SYS_UION  {w, y, 1/std, p}  model = fma(w, u(z_b) - u(z_a), u(z_a)), a = node[p], b = node[p+1] (p an int64 bit pattern),
 *                                   u(z) = v_exh / (1 + exp(-100 (z - 0.04))) on z_c = z0 + (z1 - z0) (c / (ncells - 1)): the node
 *                                   values of pem_thruster_uion_f64_dev, bit for bit
 * rec: [n_rec][4] doubles; span: [n_cond][4 kinds][2] int32 {first record, count} (kinds in the order above); node: [n_node]
 * int32 grid indices.  A condition without records of a kind adds exactly 0 for it, whatever that part of the model is.
 * The j_ion records of a sample are summed by 4 lanes against the staged profile, the others by one lane in the epilogue;
 * with j_ion records only, loglik equals pem_coupled_loglik_f64_dev's bit for bit.  The whole table is staged in LDS:
 * n_cond, n_rec <= PEM_FUSED_SYSTEM_MAX_RECORDS, n_node <= 2 PEM_FUSED_SYSTEM_MAX_RECORDS.  V_cc, div_angle, T_c, invalid
 * (optional) as pem_coupled_loglik_f64_dev.  Marginalise with pem_loglik_marginal_f64_dev ([n_chains][n_draws][n_cond]).   */
#define PEM_FUSED_SYSTEM_MAX_RECORDS 1024
#define PEM_SYS_JION 0
#define PEM_SYS_VCC 1
#define PEM_SYS_T 2
#define PEM_SYS_UION 3
int pem_coupled_system_loglik_f64_dev(size_t n, double torr2pa, double radius, const double* P_b, const double* V_a,
                                      const double* T_e, const double* V_vac, const double* Pstar, const double* P_T,
                                      const double* mdot_a, const double* a_1, const double* c0, const double* c1,
                                      const double* c2, const double* c3, const double* c4, const double* c5,
                                      const double* sigma_cex, int n_cond, int n_rec, const double* rec, const int32_t* span,
                                      int n_node, const int32_t* node, double z0, double z1, int ncells, double* V_cc,
                                      double* div_angle, double* T_c, double* loglik, uint8_t* invalid, pem_stream_t stream);

/* pem_coupled_system_loglik_f64_dev's launch with the model value of every record written out instead of compared -- the
 * predictions of the reference's validation step (scripts/pem_v0/monte_carlo.py:63-300, evaluated at each dataset's operating
 * conditions and measurement locations).  Arguments as pem_coupled_system_loglik_f64_dev, `loglik` replaced by `pred`,
 * `ld_pred` (>= n_rec).  Sample i = d * n_cond + c (condition c = i mod n_cond) writes the model value of each record r of
 * condition c to pred[d * ld_pred + r]: exactly the values the likelihood compares -- j_ion fma(w, j[k+1] - j[k], j[k]) on the
 * staged profile (which never reaches HBM), the clipped V_cc, the thrust T (not T_c), u_ion fma(w, u(z_b) - u(z_a), u(z_a)).
 * pred holds ceil(n / n_cond) rows; padding records and records of absent samples are never written.  Non-physical samples
 * give what the model gives (NaN included): nothing is filtered.  V_cc, div_angle, T_c, invalid: optional per-sample outputs.  */
int pem_coupled_system_predict_f64_dev(size_t n, double torr2pa, double radius, const double* P_b, const double* V_a,
                                       const double* T_e, const double* V_vac, const double* Pstar, const double* P_T,
                                       const double* mdot_a, const double* a_1, const double* c0, const double* c1,
                                       const double* c2, const double* c3, const double* c4, const double* c5,
                                       const double* sigma_cex, int n_cond, int n_rec, const double* rec, const int32_t* span,
                                       int n_node, const int32_t* node, double z0, double z1, int ncells, double* V_cc,
                                       double* div_angle, double* T_c, double* pred, size_t ld_pred, uint8_t* invalid,
                                       pem_stream_t stream);

/* The two launches above against ion current density measured at SEVERAL sweep radii (the reference's data schema gives it the
 * coordinates (r, theta): hallmd/data.py), still one model evaluation per sample.  plume.py:95-102 for one sample is
 *   j_ion(r, alpha_k) = base(r) g(alpha_k) + j_cex(r),   g = A1 exp(-(alpha/alpha1)^2) + A2 exp(-(alpha/alpha2)^2),
 *   decay(r) = exp(-r n sigma), base(r) = I_B0 decay(r) / r^2, j_cex(r) = I_B0 (1 - decay(r)) / (2 pi r^2):
 * the 91-point shape g does not depend on r, so it is staged once and a sample keeps n_radii pairs {base, j_cex}.
 * radii: HOST array of n_radii sweep radii [m], 2 <= n_radii <= PEM_FUSED_SYSTEM_MAX_RADII, finite, > 0, strictly ascending;
 * copied into the kernel arguments by the call.  Table, span and node as above, except that a PEM_SYS_JION record's fourth word is
 * k | (ridx << 8) (int64 bit pattern; k < 90, ridx an index into radii, clamped into it by the kernel):
 *   model = fma(base(r_ridx), fma(w, g[k+1] - g[k], g[k]), j_cex(r_ridx)).
 * A sample is non-physical (plume.py:104-107 over all radii) when alpha1 <= 0 or any j_ion(r, alpha_k) <= 0 at ANY of the radii;
 * every j_ion record of such a sample, at every radius, sees 1e-20, and `invalid` is that all-radii flag.  div_angle and T_c are
 * those of the last (largest) radius.  Everything else -- the other kinds, optional outputs, limits -- as the one-radius launches.
 * A malformed call returns PEM_ERR_INVALID_ARG before any device call.                                                          */
#define PEM_FUSED_SYSTEM_MAX_RADII 8
int pem_coupled_system_loglik_radii_f64_dev(size_t n, double torr2pa, int n_radii, const double* radii, const double* P_b,
                                            const double* V_a, const double* T_e, const double* V_vac, const double* Pstar,
                                            const double* P_T, const double* mdot_a, const double* a_1, const double* c0,
                                            const double* c1, const double* c2, const double* c3, const double* c4,
                                            const double* c5, const double* sigma_cex, int n_cond, int n_rec, const double* rec,
                                            const int32_t* span, int n_node, const int32_t* node, double z0, double z1,
                                            int ncells, double* V_cc, double* div_angle, double* T_c, double* loglik,
                                            uint8_t* invalid, pem_stream_t stream);
int pem_coupled_system_predict_radii_f64_dev(size_t n, double torr2pa, int n_radii, const double* radii, const double* P_b,
                                             const double* V_a, const double* T_e, const double* V_vac, const double* Pstar,
                                             const double* P_T, const double* mdot_a, const double* a_1, const double* c0,
                                             const double* c1, const double* c2, const double* c3, const double* c4,
                                             const double* c5, const double* sigma_cex, int n_cond, int n_rec, const double* rec,
                                             const int32_t* span, int n_node, const int32_t* node, double z0, double z1,
                                             int ncells, double* V_cc, double* div_angle, double* T_c, double* pred,
                                             size_t ld_pred, uint8_t* invalid, pem_stream_t stream);

/* pem_coupled_f64_dev + pem_svd_compress_f64_dev in one launch: latent[i][r] = sum_k norm(j_ion[i][k]) basis[k][r]
 * accumulated in the registers of the angle loop, one lane per sample (csrc/pem_latent.hip) -- the profile is neither
 * stored nor staged (120 + 24 + 8 rank bytes per evaluation).  norm: PEM_NORM_NONE or PEM_NORM_LOG10; basis: [91][rank] device array, rank <=
 * PEM_FUSED_LATENT_MAX_RANK; latent: [n][rank].  An invalid sample gets the latents of its 1e-20 profile
 * (plume.py:106), as the two-launch pipeline gives.                                                               */
#define PEM_FUSED_LATENT_MAX_RANK 8
int pem_coupled_latent_f64_dev(size_t n, double torr2pa, double radius, const double* P_b, const double* V_a,
                               const double* T_e, const double* V_vac, const double* Pstar, const double* P_T,
                               const double* mdot_a, const double* a_1, const double* c0, const double* c1,
                               const double* c2, const double* c3, const double* c4, const double* c5,
                               const double* sigma_cex, int rank, int norm, const double* basis, double* latent,
                               double* V_cc, double* div_angle, double* T_c, uint8_t* invalid, pem_stream_t stream);

/* Marginal likelihood over nuisance draws and the prior of the calibration parameters (mcmc.py:100-121; unpinned).
 * loglik: [n_chains][n_draws][n_cond] per-sample sums (pem_jion_loglik / pem_coupled_loglik output).
 * out[k] = logsumexp_m( sum_e loglik[k][m][e] + sum_e -0.5 ((discharge_current - I_d[k][m][e]) / discharge_sigma)^2 ),
 * I_d = (q/m_i) mdot_a / (1 - 2 a_1) of the analytic thruster test double; mdot_a NULL drops the discharge term.
 * log_prior (NULL or [n_chains]): out becomes the log posterior, -inf where the prior is or the likelihood is NaN. */
int pem_loglik_marginal_f64_dev(size_t n_chains, int n_draws, int n_cond, const double* loglik, const double* mdot_a,
                                const double* a_1, double discharge_current, double discharge_sigma,
                                const double* log_prior, double* out, pem_stream_t stream);
/* The same marginal with one multiplicative noise scale per group of conditions, read from the calibration table itself
 * (DESIGN.md "Noise scales").  Group g is conditions group_end[g-1] .. group_end[g] - 1 and holds group_count[g] measured records;
 * its scale on chain k is s_g = theta[k * ld_theta + scale_col[g]], or 1 exactly where scale_col[g] is -1; discharge_col is the
 * same for the discharge term (-1: discharge_sigma as given).  With w = (1 / s)^2:
 *     S[k][m] = sum_e loglik[k][m][e] * w_g(e) + w_d * sum_e -0.5 ((discharge_current - I_d[k][m][e]) / discharge_sigma)^2
 *     out[k]  = logsumexp_m S[k][m] - sum_g group_count[g] log s_g - n_cond log s_d          (+ log_prior as above)
 * A scale that is not finite and > 0 makes the likelihood NaN (-inf with log_prior).  With every scale 1 (or every column -1) out
 * is pem_loglik_marginal_f64_dev's bit for bit.  ess (NULL or [n_chains]): (sum_m p_m)^2 / sum_m p_m^2, p_m = exp(S_m - max), the
 * effective number of nuisance draws behind out.  chi (NULL or [n_chains][ld_chi], ld_chi >= n_groups + 1): sum_m p_m C_mg / sum_m
 * p_m, C_mg the UNSCALED sum of group g's conditions, in the last column that of the discharge term (0 without one): d out / d w_g
 * at fixed normaliser.  Both are NaN where the likelihood is not finite.  One workgroup per chain, no atomics: the same bits on
 * every run.  group_end, group_count, scale_col: HOST arrays [n_groups], read before return.  theta: DEVICE [n_chains][ld_theta]
 * with d columns, or NULL when every column is -1.
 * Refused with PEM_ERR_INVALID_ARG before any device call: n_groups outside [1, PEM_NOISE_MAX_GROUPS]; group_end not strictly
 * ascending within (0, n_cond] or not ending at n_cond; a negative or non-finite count; a column outside [-1, d); d < 1 or
 * ld_theta < d; discharge_col >= 0 with mdot_a NULL; ld_chi < n_groups + 1; a NULL group table; what pem_loglik_marginal_f64_dev
 * refuses.                                                                                                            */
#define PEM_NOISE_MAX_GROUPS 8
int pem_loglik_marginal_scaled_f64_dev(size_t n_chains, int n_draws, int n_cond, const double* loglik, const double* mdot_a,
                                       const double* a_1, double discharge_current, double discharge_sigma,
                                       const double* log_prior, int n_groups, const int* group_end, const double* group_count,
                                       const double* theta, int d, size_t ld_theta, const int* scale_col, int discharge_col,
                                       double* ess, double* chi, size_t ld_chi, double* out, pem_stream_t stream);
/* out[i] = sum_d log pdf_d(theta[i][d]) for the PEM_DIST_* table (kind, a, b: host arrays, ndim <= 32); -inf outside
 * the support of a uniform / log-uniform variable.  lo, hi (host arrays or NULL): the support [lo, hi] of each log-uniform
 * entry, ignored for the other kinds.  A caller that also decides the support itself passes the 10^a, 10^b it compares
 * against (calibration.BatchedPosterior passes log_prior's 10.0 ** a), so that both decisions are the same bit for bit;
 * NULL takes the host C library's pow(10, a), pow(10, b), which need not round as the caller's own code does.      */
int pem_log_prior_f64_dev(size_t n, int ndim, const int32_t* kind, const double* a, const double* b, const double* lo,
                          const double* hi, const double* theta, double* out, pem_stream_t stream);

/* ---- SVD compression / reconstruction of field QoIs (fp64 MFMA) --------------------------------
 * Stand in for amisc `Compression(method='svd')` on `j_ion` (norm log10) and `u_ion` (norm linear(1e-3)):
 * scripts/pem_v0/pem_v0_SPT-100.yml:207-214,273-280, scripts/gen_data.py:261-294.  Third-party in the
 * reference: parity UNPINNED; formulas (csrc/pem_svd.hip):
 *     latent[n][rank] = norm(field[n][dof]) @ basis[dof][rank]        (compress)
 *     field[n][dof]   = denorm(latent[n][rank] @ basis[dof][rank]^T)  (reconstruct)
 * norm: PEM_NORM_NONE x; PEM_NORM_LOG10 log10(x) / 10^y; PEM_NORM_LINEAR x*norm_scale / y/norm_scale.
 * All arrays row-major in device memory; dof <= PEM_SVD_MAX_DOF, rank <= 16.                          */
#define PEM_SVD_MAX_DOF 208
#define PEM_NORM_NONE 0
#define PEM_NORM_LOG10 1
#define PEM_NORM_LINEAR 2
int pem_svd_compress_f64_dev(size_t n, int dof, int rank, int norm, double norm_scale, const double* field,
                             const double* basis, double* latent, pem_stream_t stream);
int pem_svd_reconstruct_f64_dev(size_t n, int dof, int rank, int norm, double norm_scale, const double* latent,
                                const double* basis, double* field, pem_stream_t stream);

/* ---- sparse-grid Lagrange surrogate: batched predict ----------------------------------------------------
 * Stand in for the surrogate evaluations of amisc `System.fit(num_refine=...)` / `System.predict`
 * (scripts/fit_surr.py:101-116; BASELINE.json configs[3]).  Third-party in the reference: parity UNPINNED;
 * formula in csrc/pem_surrogate.hip, tables built by hallthrusterpem_amd/surrogate.py.
 *   out[o][i] = sum_b coef[b] * sum_nodes values[offset_b + node][o] * prod_a basis(level_a, t[dim_a][i])
 * index: [n_beta][2 + 2*PEM_SURR_MAX_ACTIVE] int32 = {n_active, value offset (rows), dims[], levels[]};
 * values: [rows][n_out]; t: [n_dim][ld] normalised coordinates in [-1, 1], n_dim <= PEM_SURR_MAX_DIM;
 * out: [n_out][ld_out]; n_out <= 16.                                                                        */
#define PEM_SURR_MAX_ACTIVE 5
#define PEM_SURR_MAX_LEVEL 4
#define PEM_SURR_MAX_DIM 32
/* max_active / max_level: the largest number of active dimensions / the highest level any multi-index of `index` has (the caller
 * built the table): they size the LDS the kernel keeps the outer dimensions' bases in -- (max_active - 1) (2^max_level + 1) + n_dim
 * doubles per thread of 256 must fit 160 KB.                                                                                          */
int pem_sparse_predict_f64_dev(size_t n, int n_dim, int n_beta, const int32_t* index, const double* coef,
                               const double* values, int n_out, const double* t, size_t ld, double* out,
                               size_t ld_out, int max_active, int max_level, pem_stream_t stream);
/* The same tables, every grid on its own: out[b][o][i] = coef[b] * (the interpolant of grid b at point i), out: [n_beta][n_out]
 * [ld_out].  The adaptive refinement scores all its candidate index sets from ONE such launch -- a prediction is linear in the
 * combination coefficients, so each trial is a [n_beta] x [n_beta][n_out n] product of these values (surrogate.py refine). */
int pem_sparse_grid_values_f64_dev(size_t n, int n_dim, int n_beta, const int32_t* index, const double* coef,
                                   const double* values, int n_out, const double* t, size_t ld, double* out,
                                   size_t ld_out, int max_active, int max_level, pem_stream_t stream);
/* Prediction + reconstruction of a compressed field QoI in one launch (round 4): outputs lat0 .. lat0 + rank - 1 of the surrogate
 * are the SVD latent coefficients the reference trains on (scripts/pem_v0/pem_v0_SPT-100.yml:273-280 `j_ion`: svd, log10 norm,
 * reconstruction_tol 0.01; scripts/fit_surr.py:101-133), and field[i][k] = denorm(sum_q latent_q(i) basis[k][q]), k < dof, leaves
 * with them -- what amisc's System.predict returns for such a variable, without pem_svd_reconstruct_f64_dev's second pass.
 * norm / norm_scale / basis as pem_svd_reconstruct_f64_dev; field: [n][dof] row-major.                                            */
int pem_sparse_predict_field_f64_dev(size_t n, int n_dim, int n_beta, const int32_t* index, const double* coef, const double* values,
                                     int n_out, const double* t, size_t ld, double* out, size_t ld_out, int max_active, int max_level,
                                     int lat0, int rank, int dof, int norm, double norm_scale, const double* basis, double* field,
                                     pem_stream_t stream);
/* The component chain in one launch (round 5): one surrogate per component, chained through the coupling variables as the reference
 * trains them (scripts/pem_v0/pem_v0_SPT-100.yml:4-6,62-63,215-219: Cathode V_cc -> Thruster; Thruster I_B0 -> Plume).  stages: HOST
 * array of three tables in the format above (device arrays), cathode, thruster, plume; their dims[] are slots of ONE coordinate table of
 * n_dim slots.  t: [n_dim - 2][ld], the external coordinates of every slot but vcc_slot and ib0_slot, in slot order.  Per point:
 *   V_cc       = cathode(t)                          (n_out == 1)
 *   slot vcc   = 2.0 * (V_cc - vcc_lo) / vcc_w - 1.0  (left to right, no contraction: system.py's input map)
 *   I_B0, T    = thruster(t)                         (n_out == 2)
 *   slot ib0   = 2.0 * (I_B0 - ib0_lo) / ib0_w - 1.0
 *   div_angle, p_1 .. p_{n_out-1} = plume(t)         (1 <= n_out <= 16)
 *   T_c        = T * cos(div_angle)                  (plume.py:136-140)
 * out: [4 + n_out(plume)][ld_out] rows V_cc, I_B0, T, div_angle, T_c, p_1, ...  field: NULL, or as pem_sparse_predict_field_f64_dev over
 * the plume stage's outputs lat0 .. lat0 + rank - 1.  LDS: the largest stage's bases plus n_dim coordinates, the 160 KB rule above.
 * Every argument is checked before the device is, so a malformed call fails with PEM_ERR_INVALID_ARG without a GPU too. */
typedef struct pem_surr_stage {
    const int32_t* index;
    const double* coef;
    const double* values;
    int n_beta, n_out, max_active, max_level;
} pem_surr_stage;
int pem_sparse_predict_chain_f64_dev(size_t n, int n_dim, int vcc_slot, int ib0_slot, const pem_surr_stage* stages, double vcc_lo,
                                     double vcc_w, double ib0_lo, double ib0_w, const double* t, size_t ld, double* out, size_t ld_out,
                                     int lat0, int rank, int dof, int norm, double norm_scale, const double* basis, double* field,
                                     pem_stream_t stream);
/* The component chain and the Gaussian log-likelihood of several measured quantities in one launch: the surrogate in the place of the
 * model inside the likelihood, as the reference calibrates (scripts/pem_v0/mcmc.py:57-106: `SURR.predict`, `jion_reconstruct`, the
 * discharge current from the surrogate's own output; its surrogate is third-party: parity UNPINNED, held to the composition of
 * pem_sparse_predict_chain_f64_dev and a long-double sum).  The chain arguments (n .. ld) as pem_sparse_predict_chain_f64_dev, and the
 * chain's values equal that launch's bit for bit.  Sample i belongs to condition c = i mod n_cond; rec / span are
 * pem_coupled_system_loglik_f64_dev's table (likelihood.SystemLikelihood), unchanged.  Per sample
 *   j[k]          = denorm(v), v = 0; v = fma(p_{lat0+q}, basis[k][q], v), q = 0 .. rank - 1 (pem_sparse_predict_field_f64_dev's
 *                   expression, dof == 91), at the nodes k, k + 1 of the condition's j_ion records only: no profile reaches HBM
 *   PEM_SYS_JION    m = fma(w, j[k+1] - j[k], j[k])
 *   PEM_SYS_VCC     m = V_cc
 *   PEM_SYS_T       m = T, the thruster stage's second output (not T_c)
 *   PEM_SYS_UION    the chain carries no u_ion latents: a condition with such records gets NaN, as does one with j_ion records when
 *                   basis is NULL
 *   loglik[i]     = sum -0.5 z^2, z = (y - m) * inv_std, one lane per sample, in the order j_ion, V_cc, T (each kind in record
 *                   order), every term added by one fma(-0.5 z, z, sum)
 *   a_1 (NULL or [n]): loglik[i] = fma(-0.5 z, z, loglik[i]) once more, z = (discharge_current - I_d) * (1 / discharge_sigma),
 *                   I_d = I_B0 / (1 - 2 a_1[i]) with the SURROGATE's I_B0 (mcmc.py:101 takes I_D from the surrogate's output);
 *                   marginalise with pem_loglik_marginal_f64_dev WITHOUT its own discharge term
 * out (NULL or [4 + n_out(plume)][ld_out]): the rows of pem_sparse_predict_chain_f64_dev.  pred (NULL or [ceil(n / n_cond)][ld_pred],
 * ld_pred >= n_rec): as pem_coupled_system_predict_f64_dev, sample i = d n_cond + c writes m of record r of condition c to
 * pred[d * ld_pred + r]; padding records are neither summed nor written.  A sample's loglik and pred bits depend on its coordinates,
 * its condition and the tables only -- not on n, its position, the grid or which optional outputs are asked for.
 * n_cond, n_rec in 1 .. PEM_FUSED_SYSTEM_MAX_RECORDS; rank <= 16.  LDS: the chain's (a latent slot per thread included), and the
 * record table, the spans and the basis beside it where they fit the 160 KB, else they are read through the cache (same bits).
 * Every argument is checked before the device is. */
int pem_chain_system_loglik_f64_dev(size_t n, int n_dim, int vcc_slot, int ib0_slot, const pem_surr_stage* stages, double vcc_lo,
                                    double vcc_w, double ib0_lo, double ib0_w, const double* t, size_t ld, int lat0, int rank, int dof,
                                    int norm, double norm_scale, const double* basis, int n_cond, int n_rec, const double* rec,
                                    const int32_t* span, const double* a_1, double discharge_current, double discharge_sigma,
                                    double* loglik, double* out, size_t ld_out, double* pred, size_t ld_pred, pem_stream_t stream);

/* The two chained launches with the ion velocity carried through the thruster stage (scripts/pem_v0/pem_v0_SPT-100.yml:207-214: `u_ion`
 * is compressed as `j_ion` is -- svd, reconstruction_tol 0.01 -- under norm linear(1.0e-3); train-shim.sh:9-11 trains it with the thruster
 * component; mcmc.py:88-89 reconstructs it inside the likelihood).  Arguments as the parents', then the thruster stage's field:
 *   u_lat0 (== 2), u_rank (0 .. 14): the thruster table has n_out == 2 + u_rank outputs I_B0, T, l_0 .. l_{u_rank-1}
 *   u_dof (>= 2): the cells of the u_ion grid; u_norm / u_scale / u_basis[u_dof][u_rank]: as pem_svd_reconstruct_f64_dev
 *   u[c] = denorm(v), v = 0; v = fma(l_q, u_basis[c][q], v), q = 0 .. u_rank - 1 (pem_sparse_predict_field_f64_dev's expression;
 *          PEM_NORM_LINEAR: v / u_scale)
 * pem_sparse_predict_chain_fields_f64_dev: out has u_rank more rows, [4 + n_out(plume) + u_rank][ld_out]: the parent's, then l_0 ...;
 *   u_field (NULL or [n][u_dof]): u[c] of every cell.
 * pem_chain_fields_loglik_f64_dev: out (optional) as above.  node ([n_node] int32 DEVICE array) and node_host (the caller's HOST copy
 *   of it, the one that is checked: every entry in [0, u_dof); the kernel clamps the device entries into the grid, so a copy that
 *   differs reads no memory outside u_basis): likelihood.SystemLikelihood's table of pem_coupled_system_loglik_f64_dev.  n_node is 0
 *   (no u_ion records) or 2 .. 2 PEM_FUSED_SYSTEM_MAX_RECORDS; the spans live in device memory, so u_ion records that meet n_node == 0
 *   cannot be refused: their condition gets NaN.
 *   PEM_SYS_UION  {w, y, 1/std, p}  m = fma(w, u[b] - u[a], u[a]), a = node[p], b = node[p + 1], p clamped to n_node - 2 as
 *                                   pem_coupled_system_loglik_f64_dev clamps it
 *   loglik[i]: the terms in the order u_ion, j_ion, V_cc, T (each kind in record order), then the discharge term, every one added by
 *   one fma(-0.5 z, z, sum) from 0.  The u_ion terms and u_field are evaluated between the thruster and the plume stage.
 * Bit contracts (tests/test_chain_uion.py):
 *   1. u_rank == 0: the parents' kernels run; every output equals the parent entry point's bit for bit, u_ion records give NaN and
 *      the other u_* / node arguments are not looked at (n_node's range aside).
 *   2. u_rank > 0: V_cc, I_B0, T, div_angle, T_c, the plume's outputs, the j_ion field and the loglik / pred of every condition
 *      without u_ion records equal, bit for bit, what the parent returns for the same chain with the thruster table cut to its first
 *      two value columns (a column of a stage is summed independently of the others).
 *   3. A sample's loglik, pred and u_field bits depend on its coordinates, its condition and the tables only -- not on n, its
 *      position, the grid, whether the tables were staged in LDS or which optional outputs are asked for.
 * LDS: the parent's policy; the u_ion latents take basis slots of their thread (counted), and of u_basis only the n_node rows the node
 * table names are gathered, once per workgroup, beside the record table where that is staged.  Every argument is checked before the
 * device is: NULL u_basis with u_rank > 0, u_lat0 != 2, u_dof < 2, an unknown u_norm, a zero or non-finite u_scale under
 * PEM_NORM_LINEAR, stages[1].n_out != 2 + u_rank, n_node outside
 * its range or == 1, a NULL node / node_host with n_node > 0, a node_host entry outside [0, u_dof). */
int pem_sparse_predict_chain_fields_f64_dev(size_t n, int n_dim, int vcc_slot, int ib0_slot, const pem_surr_stage* stages, double vcc_lo,
                                            double vcc_w, double ib0_lo, double ib0_w, const double* t, size_t ld, double* out, size_t ld_out,
                                            int lat0, int rank, int dof, int norm, double norm_scale, const double* basis, double* field,
                                            int u_lat0, int u_rank, int u_dof, int u_norm, double u_scale, const double* u_basis,
                                            double* u_field, pem_stream_t stream);
int pem_chain_fields_loglik_f64_dev(size_t n, int n_dim, int vcc_slot, int ib0_slot, const pem_surr_stage* stages, double vcc_lo,
                                    double vcc_w, double ib0_lo, double ib0_w, const double* t, size_t ld, int lat0, int rank, int dof,
                                    int norm, double norm_scale, const double* basis, int n_cond, int n_rec, const double* rec,
                                    const int32_t* span, const double* a_1, double discharge_current, double discharge_sigma,
                                    double* loglik, double* out, size_t ld_out, double* pred, size_t ld_pred, int u_lat0, int u_rank,
                                    int u_dof, int u_norm, double u_scale, const double* u_basis, int n_node, const int32_t* node,
                                    const int32_t* node_host, pem_stream_t stream);

/* ---- per-column order statistics over the sample axis -------------------------------------------------------------
 * The percentiles of scripts/gen_data.py:125-174 (`np.percentile(arr, 25 | 75, axis=0)`, NaN / interquartile-range masks) and
 * of scripts/pem_v0/monte_carlo.py:363-658 (5 / 50 / 95 % bands) at forward-UQ sizes, by exact radix selection instead of a
 * sort (csrc/pem_quantile.hip).  data: [n][ld] row-major device array of which columns 0..m-1 are used, m <= 256 (ld = m:
 * fully coalesced); for quantile i the caller gives the two ranks
 * numpy's method 'linear' reads (rank_prev[i] <= rank_next[i] < n) and its weight gamma[i] (HOST arrays);
 * out[i][c] = _lerp(x_(rank_prev[i]), x_(rank_next[i]), gamma[i]) of column c, NaN if the column holds a NaN -- equal to
 * np.percentile bit for bit.  nq <= PEM_QUANTILE_MAX_Q per call (PEM_QUANTILE_MAX_Q_WIDE for m > 128).  Allocates its workspace and synchronises the stream.
 * From n * m = 2^25 values on, every 32nd row is examined first and brackets the wanted ranks, which leaves two passes over the
 * data instead of four; a call whose data defeat the brackets (the counts say so) repeats with the four passes -- the result is
 * the same either way.  Environment: PEM_QUANTILE_PILOT = that stride (0: never), PEM_QUANTILE_PILOT_MIN = the smallest n * m it
 * is used for.  pem_quantiles_last_path(): how the last call went (0 four passes, 1 brackets held, 2 brackets failed, four passes).   */
#define PEM_QUANTILE_MAX_Q 6
#define PEM_QUANTILE_MAX_Q_WIDE 3      /* per call for 128 < m <= 256 columns */
int pem_quantiles_f64_dev(size_t n, int m, const double* data, size_t ld, int nq, const uint64_t* rank_prev, const uint64_t* rank_next,
                          const double* gamma, double* out, pem_stream_t stream);
/* The same over a strided view: value (row, c) at data[row * ld + c * cs] -- (ld >= m, cs = 1) is the form above; (ld = 1, cs >= n)
 * takes the m columns from m contiguous arrays of n values cs apart, e.g. the [3][n] reduced-QoI tensor of a batch
 * (V_cc, div_angle, T_c in ONE call instead of three).                                                                            */
int pem_quantiles_strided_f64_dev(size_t n, int m, const double* data, size_t ld, size_t cs, int nq, const uint64_t* rank_prev,
                                  const uint64_t* rank_next, const double* gamma, double* out, pem_stream_t stream);
int pem_quantiles_last_path(void);

/* Fused Monte-Carlo evaluation + percentiles of the profile, counted where the profile is produced (round 4; csrc/pem_qfused.h):
 * `sample_inputs` + `predict` of scripts/gen_data.py:238-239 followed by the `np.percentile(j_ion, ..., axis=0)` of
 * gen_data.py:163-168 and scripts/pem_v0/monte_carlo.py:363-658, without reading the profile back.  The arguments of
 * pem_coupled_mc_f64_dev (plain Monte-Carlo block: swap_dim -1) and of pem_quantiles_f64_dev (HOST arrays rank_prev / rank_next /
 * gamma of nq <= PEM_QUANTILE_MAX_Q quantiles of the n samples; q_out [nq][91] on the device).  Samples 0 .. ceil(n / 32) - 1 are
 * evaluated first and bracket the wanted ranks; ONE launch then evaluates all n samples, counts every profile value against the
 * brackets in LDS and writes the values inside them (4 %) out as records, from which the order statistics are selected.
 * j_ion NULL: the profile is never stored (pilot_rows: room for ceil(n / 32) x 91 doubles then holds the pilot's rows; ignored
 * when j_ion is given).  *fused_ok = 1: q_out equals np.percentile of the profile bit for bit.  *fused_ok = 0: the selection
 * declined -- brackets of one key or overlapping (heavy ties), a rank outside its bracket, a non-finite profile value, record
 * overflow -- q_out is not written; all other outputs are complete either way, and the caller takes pem_quantiles_f64_dev over
 * the stored profile.  n >= PEM_MC_STATS_MIN_N.  Synchronises the stream.
 * The premask (row_certain / row_uncertain [n] bytes on the device and premask_ok non-NULL, nq <= 5): quantiles q25 and q75 of the
 * call are the quartiles of gen_data.py:163-164; the outlier bounds p25 - f iqr, p75 + f iqr are then known to lie in intervals
 * (the quartiles lie in their brackets), and the counting launch also writes, per sample, how many of its 91 values lie outside
 * the bounds FOR CERTAIN and how many are UNCERTAIN (inside one of the two intervals).  certain > int(0.75 * 91) is an outlier,
 * certain + uncertain <= that is not, and the caller settles the rest from the exact bounds: gen_data.py:166-168 without a pass
 * over the profile.  *premask_ok = 0: not produced (bounds zero or not finite, f < 0, nq > 5, or the selection declined).
 * q_scalars (optional; [nq][3] on the device): the same nq percentiles of V_cc, div_angle and T_c -- which must then be rows 0, 1, 2
 * of one array (the [3][n] reduced-QoI tensor of a batch) -- as pem_quantiles_strided_f64_dev gives them, selected on a second
 * thread and a stream of the library's own while the calling thread takes the profile's records through their passes; written
 * whether or not the profile's selection declined.                                                                                */
#define PEM_MC_STATS_MIN_N 4096
int pem_coupled_mc_stats_f64_dev(size_t n, uint64_t first_index, uint64_t seed, uint32_t stream_id, const int32_t* kind, const double* a,
                                 const double* b, double torr2pa, double radius, double* x_out, size_t ld, double* V_cc, double* I_B0,
                                 double* T, double* j_ion, double* pilot_rows, double* div_angle, double* T_c, uint8_t* invalid, int nq,
                                 const uint64_t* rank_prev, const uint64_t* rank_next, const double* gamma, double* q_out, double* q_scalars,
                                 int* fused_ok, int q25, int q75, double iqr_factor, uint8_t* row_certain, uint8_t* row_uncertain,
                                 int* premask_ok, pem_stream_t stream);

/* The per-sample masks of `_filter_outputs` (scripts/gen_data.py:150-168) for one output variable in one pass over it
 * (csrc/pem_masks.hip): data [n][ld] row-major, entries 0..m-1 of a sample; lo / hi: m per-entry bounds each (DEVICE arrays:
 * p25 - f iqr and p75 + f iqr, computed by the caller from pem_quantiles_f64_dev's result as the reference does);
 * nan_out[i] = 1 if sample i holds a NaN (`np.any(np.isnan(arr), axis=rest)`), outside_out[i] = the number of its entries with
 * x < lo or x > hi (`np.sum((arr < lo) | (arr > hi), axis=rest)`; a comparison with a NaN is false, as in numpy) -- the caller
 * compares it with int(0.75 * m).  1 <= m <= PEM_ROW_MASKS_MAX_M.  Asynchronous on `stream`.                                  */
#define PEM_ROW_MASKS_MAX_M 512
int pem_row_masks_f64_dev(size_t n, int m, const double* data, size_t ld, const double* lo, const double* hi, uint8_t* nan_out,
                          int32_t* outside_out, pem_stream_t stream);

/* The masks of a campaign's SCALAR outputs and the verdict of the profile's premask counts in one pass, one thread per sample
 * (drivers.forward_uq_statistics; gen_data.py:150-168 for variables of one entry per sample): vars: HOST array of nvar <= 8 device
 * pointers to n values each; q: the variables' percentiles on the device, rows of nvar values q_ld apart (pem_coupled_mc_stats_f64_dev's
 * q_scalars), of which rows row25 / row75 are the quartiles: the bounds are p25 - f iqr and p75 + f iqr, rounded as numpy rounds them;
 * nan_out / outl_out [nvar][mask_ld] bytes, mask_ld >= n (a multiple of 4 lets the pass write words) (0 / 1: np.isnan(x); (x < lo) | (x > hi)).  With row_certain / row_uncertain (the per-sample counts
 * of pem_coupled_mc_stats_f64_dev's premask; both or neither) the arrays have one row more, the profile's: nan_out[nvar][i] = 0,
 * outl_out[nvar][i] = certain > thresh, and the samples with certain <= thresh < certain + uncertain -- whose verdict the exact bounds
 * must settle -- are appended to open_rows (int64, room for `cap`; unordered) and counted in *open_count (device int32, zeroed by the
 * caller; more than cap: the list is incomplete).  Asynchronous on `stream`.                                                       */
int pem_campaign_masks_f64_dev(size_t n, int nvar, const double* const* vars, const double* q, int q_ld, int row25, int row75,
                               double iqr_factor, uint8_t* nan_out,
                               uint8_t* outl_out, size_t mask_ld, const uint8_t* row_certain, const uint8_t* row_uncertain, int thresh,
                               int64_t* open_rows, int32_t* open_count, int cap, pem_stream_t stream);

/* The multi-rank building blocks of the same selection (samples sharded over GPUs; hallthrusterpem_amd/percentiles.py drives the
 * levels and all-reduces between them): the histogram of the keys -- the order-preserving 64-bit image of the values (sign bit
 * flipped, negative values inverted; per-column min / max and a NaN flag: pem_qsel_minmax_f64_dev below) -- inside caller-given
 * ranges, nr = 1, 2, 4 or 6 ranges per column, hist[c][r][bin] (zeroed here), m * nr * bins <= 36864.
 * Bin of key k in [klo, khi]: d = (k - klo) >> shift, shift the smallest with (khi - klo) >> shift < 2^31; bin = d if
 * ((khi - klo) >> shift) < bins, else floor(d * mult / 2^32), mult = min(2^32 - 1, floor(2^32 * bins / (((khi - klo) >> shift) + 1))).
 * All arrays on the device.  pem_range_hist does not synchronise the stream.                                                    */
int pem_range_hist_f64_dev(size_t n, int m, const double* data, size_t ld, int nr, const uint64_t* klo, const uint64_t* khi,
                           int bins, uint32_t* hist, pem_stream_t stream);
/* One level's decision, on the device: for each of n_ranges ranges the bin of hist[range][bins] (the all-reduced counts) that
 * holds resid[range], then klo / khi <- the keys of that bin and resid <- the rank inside it; ranges with klo >= khi are left. */
int pem_range_narrow_dev(int n_ranges, int bins, const uint32_t* hist, uint64_t* klo, uint64_t* khi, int64_t* resid,
                         pem_stream_t stream);

/* The sharded selection on the single-GPU selection's passes (round 3; the percentiles of scripts/gen_data.py:163-168 and
 * scripts/pem_v0/monte_carlo.py:363-658 over samples that live on several GPUs).  Every rank runs the same stages over its own
 * rows; hallthrusterpem_amd/percentiles.py all-reduces kmin / kmax / has_nan (MIN / MAX), hist1 and hist2 (SUM) between them and
 * all-gathers the padded candidate lists, so that every rank takes the same decisions: four streaming passes instead of the
 * eleven levels of pem_range_hist.  All arrays on the device, caller-owned; nt = 2 nq targets per column (the two order
 * statistics of each of nq <= PEM_QUANTILE_MAX_Q quantiles); nothing here synchronises the stream.
 *   pem_qsel_bins      bins1 / bins2 the histograms use for m columns and nt targets (pure arithmetic: LDS-bound powers of two)
 *   pem_qsel_minmax    kmin / kmax [m]: smallest / largest key of each column (kmin > kmax: no value), has_nan [m]
 *   pem_qsel_hist1     hist1[m][bins1] over [kmin, kmax] (the all-reduced ones): bin = floor(d mult / 2^32), d = (k - kmin) >> shift,
 *                      shift the smallest with (kmax - kmin) >> shift < 2^31, mult = min(2^32 - 1, floor(2^32 bins1 / (((kmax - kmin) >> shift) + 1)))
 *   pem_qsel_decide1   per (column, target): bin1 = the bin of the summed hist1 that holds resid (in: the wanted 0-based rank),
 *                      resid <- rank inside that bin; a column with kmin >= kmax is done at once (answer = kmin)
 *   pem_qsel_hist2     hist2[m][nt][bins2]: sub-bins (floor(frac bins2 / 2^32), frac = low word of d mult) of every target's bin1;
 *                      a bin shared by several targets of a column is counted under the first of them
 *   pem_qsel_decide2   bin2 from the summed hist2, resid <- rank inside it, count = values of all ranks in it, count_local = this
 *                      rank's (read from hist2_local, the rank's own counts)
 *   pem_qsel_compact   this rank's keys of every (bin1, bin2) into cand[m nt][list_len], padded with ~0; cursor[m nt] = values
 *                      offered (> list_len: the list overflowed); shared pairs are collected once, under the first target
 *   pem_qsel_select    answer[m nt] = the key of rank resid in the union of the `world` gathered lists (gathered[world][m nt][list_len]) */
int pem_qsel_bins(int m, int nt, int* bins1, int* bins2);
int pem_qsel_minmax_f64_dev(size_t n, int m, const double* data, size_t ld, uint64_t* kmin, uint64_t* kmax, int32_t* has_nan,
                            pem_stream_t stream);
int pem_qsel_hist1_f64_dev(size_t n, int m, const double* data, size_t ld, const uint64_t* kmin, const uint64_t* kmax, int bins1,
                           uint32_t* hist1, pem_stream_t stream);
int pem_qsel_decide1_dev(int m, int nt, const uint64_t* kmin, const uint64_t* kmax, const uint32_t* hist1, int bins1, uint64_t* resid,
                         int32_t* bin1, int32_t* done, uint64_t* answer, pem_stream_t stream);
int pem_qsel_hist2_f64_dev(size_t n, int m, const double* data, size_t ld, const uint64_t* kmin, const uint64_t* kmax, int nt,
                           const int32_t* bin1, int bins1, int bins2, uint32_t* hist2, pem_stream_t stream);
int pem_qsel_decide2_dev(int m, int nt, const uint32_t* hist2, const uint32_t* hist2_local, int bins2, const int32_t* bin1,
                         const int32_t* done, uint64_t* resid, int32_t* bin2, uint64_t* count, uint32_t* count_local, pem_stream_t stream);
int pem_qsel_compact_f64_dev(size_t n, int m, const double* data, size_t ld, const uint64_t* kmin, const uint64_t* kmax, int nt,
                             const int32_t* bin1, const int32_t* bin2, const int32_t* done, int bins1, int bins2, uint32_t list_len,
                             uint64_t* cand, uint32_t* cursor, pem_stream_t stream);
int pem_qsel_select_dev(int m, int nt, int world, uint32_t list_len, const uint64_t* gathered, const int32_t* bin1, const int32_t* bin2,
                        const int32_t* done, const uint64_t* resid, uint64_t* answer, pem_stream_t stream);

/* ---- fused Monte-Carlo evaluation -----------------------------------------------------------------
 * sample_inputs + predict of scripts/gen_data.py:238-239 in ONE launch: the 15 coupled inputs of global samples
 * first_index .. first_index+n-1 are generated in registers from the counter-based design (kind/a/b as for
 * pem_sample_f64_dev, input order P_b V_a T_e V_vac Pstar P_T mdot_a a_1 c0..c5 sigma_cex) and never touch HBM
 * unless x_out ([15][ld], ld >= n) is given.  Results are bit-identical to pem_sample_f64_dev followed by
 * pem_coupled_f64_dev (swap_dim selects the Saltelli block as there).  752 instead of 872 bytes per evaluation. */
int pem_coupled_mc_f64_dev(size_t n, uint64_t first_index, uint64_t seed, uint32_t stream_id, int swap_dim,
                           const int32_t* kind, const double* a, const double* b, double torr2pa, double radius,
                           double* x_out, size_t ld,
                           double* V_cc, double* I_B0, double* T, double* j_ion, double* div_angle, double* T_c,
                           uint8_t* invalid, pem_stream_t stream);

/* ---- single-precision arithmetic: reduced QoIs and the fused Saltelli design (csrc/pem_fp32.hip) ----------------------
 * SURVEY.md section 8b "fp32/mixed entry points optional with a tolerance report", section 8d config 5 (BASELINE
 * configs[4]: Sobol' sensitivity, "fp64 -> fp32 mixed with tolerance check").  The same formulas as pem_coupled_f64_dev
 * (cathode.py:24-38, tests/sim_hallthruster.jl:35-48, plume.py:39-140) evaluated in fp32 from fp32 tables; only the
 * scalar QoIs are produced.  The tolerance report (fp32 against fp64 on identical inputs, per QoI) is
 * hallthrusterpem_amd.fp32.compare_with_fp64 / bench.py --fp32 / tests/test_fp32.py.
 *   x:   [15][ld] floats, rows in the order P_b V_a T_e V_vac Pstar P_T mdot_a a_1 c0..c5 sigma_cex
 *   qoi: [3][ldq] floats: V_cc, div_angle, T_c;  invalid (optional): plume.py:105's flag per sample.                       */
int pem_coupled_f32_dev(size_t n, float torr2pa, float radius, const float* x, size_t ld, float* qoi, size_t ldq,
                        uint8_t* invalid, pem_stream_t stream);
/* The Saltelli design of scripts/pem_v0/sobol.py:46-118 (uqtils sobol_sa, third-party: parity UNPINNED) as ONE launch:
 * for base samples first_index .. first_index+n_base-1 the rows A (stream_id) and B (stream_id + 1) of the counter-based
 * design -- the same numbers as pem_sample_f64_dev, rounded to float -- are generated in registers, the fp32 model is
 * evaluated on A, B and on A with column varied[j] from B for j < n_varied, and the estimator sums are accumulated in
 * fp64: partial[n_blocks][2 + 2 n_varied][3] (rows: sum fA+fB, sum fA^2+fB^2, then per varied input sum fB (fAB-fA) and
 * sum (fA-fAB)^2; columns V_cc, div_angle, T_c), one deterministic partial per workgroup.  flags[n_blocks][2]: counts of
 * non-physical thruster results (thruster.py:490-493: T < 0 or I_B0 < 0) and of invalid plume samples over all
 * n_base (n_varied + 2) evaluations.  Nothing but the partial sums touches HBM.                                         */
int pem_saltelli_f32_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, const int32_t* kind,
                         const double* a, const double* b, int n_varied, const int32_t* varied, float torr2pa,
                         float radius, double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream);
/* The same launch around the fp64 model (lane per sample; the scalar stages and tables of the coupled kernel, bit-identical
 * to pem_coupled_f64_dev's reduced-QoI results for samples inside the table range), on the design itself, not rounded.  */
int pem_saltelli_f64_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, const int32_t* kind,
                         const double* a, const double* b, int n_varied, const int32_t* varied, double torr2pa,
                         double radius, double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream);
/* The same two launches on the shifted Sobol' design: rows A and B of base sample first_index + i are sequence dimensions
 * 0..14 and 15..29 of point first_index + i -- the numbers of pem_sample_sobol_f64_dev(ndim = 15, swap_dim = -1 / -2) with the
 * same seed, stream_id and scramble.  first_index + n_base > 2^30 is refused.  Everything else as above.                  */
int pem_saltelli_qmc_f32_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, int scramble,
                             const int32_t* kind, const double* a, const double* b, int n_varied, const int32_t* varied,
                             float torr2pa, float radius, double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream);
int pem_saltelli_qmc_f64_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, int scramble,
                             const int32_t* kind, const double* a, const double* b, int n_varied, const int32_t* varied,
                             double torr2pa, double radius, double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream);
/* The Saltelli (2002) extension to second-order indices, one launch (csrc/pem_saltelli2.hip): the arguments of the four launches
 * above plus `centre`, 3 host doubles c (V_cc, div_angle, T_c; copied into the launch).  Per base sample the model also runs on
 * B with column varied[j] from A (BA_j): n_base (2 n_varied + 2) evaluations, which `flags` counts over.
 * partial[n_blocks][rows][3], rows = 3 + 4 nv + nv (nv - 1) / 2 with nv = n_varied:
 *   0, 1: sum fA+fB, sum fA^2+fB^2;  2+2j, 3+2j: sum fB (fAB_j-fA), sum (fA-fAB_j)^2 (the rows of the launches above);
 *   2+2nv+2j, 3+2nv+2j: the mirrored sums, sum fA (fBA_j-fB), sum (fB-fBA_j)^2;  2+4nv: D = sum (fA-c)(fB-c);
 *   3+4nv+p: C_ij = sum (fBA_i-c)(fAB_j-c) for the pairs i < j < nv of `varied` in lexicographic order.                      */
int pem_saltelli2_f32_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, const int32_t* kind,
                          const double* a, const double* b, int n_varied, const int32_t* varied, const double* centre,
                          float torr2pa, float radius, double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream);
int pem_saltelli2_f64_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, const int32_t* kind,
                          const double* a, const double* b, int n_varied, const int32_t* varied, const double* centre,
                          double torr2pa, double radius, double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream);
int pem_saltelli2_qmc_f32_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, int scramble,
                              const int32_t* kind, const double* a, const double* b, int n_varied, const int32_t* varied,
                              const double* centre, float torr2pa, float radius, double* partial, uint64_t* flags, int n_blocks,
                              pem_stream_t stream);
int pem_saltelli2_qmc_f64_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, int scramble,
                              const int32_t* kind, const double* a, const double* b, int n_varied, const int32_t* varied,
                              const double* centre, double torr2pa, double radius, double* partial, uint64_t* flags, int n_blocks,
                              pem_stream_t stream);
/* First-order and total sums of the whole 91-angle j_ion profile, one launch (csrc/pem_saltelli_profile.hip): the design, rows and
 * arguments of pem_saltelli_f64_dev / pem_saltelli_qmc_f64_dev, evaluated on A, B and AB_j -- n_base (n_varied + 2) evaluations,
 * which `flags` counts over.  One evaluation at angle k is the reference's expression (plume.py:99-102), alpha_90 = pi/2 exactly:
 *   t = alpha_k / a;  j_k = X1a exp(-(t1 t1)) + X2a exp(-(t2 t2)) + j_cex;  a1 <= 0 or any j_k <= 0: the whole row is 1e-20
 * f_k = j_k (norm = 0) or log10 j_k (norm = 1).  `centre`: 91 DEVICE doubles c_k, or NULL for zeros.  n_varied may be 0 (then
 * `varied` may be NULL).  partial[n_blocks][2 + 4 n_varied][91], one deterministic partial per workgroup:
 *   row 0        sum (fA - c) + (fB - c)
 *   row 1        sum (fA - c)^2 + (fB - c)^2
 *   row 2 + 4 j  sum t1,    t1 = (fB - c) (fAB_j - fA)
 *   row 3 + 4 j  sum t1^2
 *   row 4 + 4 j  sum t2,    t2 = (fA - fAB_j)^2
 *   row 5 + 4 j  sum t2^2
 * flags[n_blocks][2]: non-physical thruster results, invalid plume rows.  n_base = 0 writes zeros.  PEM_ERR_INVALID_ARG, nothing
 * launched: n_varied outside 0..15, norm outside {0, 1}, n_blocks < 1, radius <= 0, a NULL output, and for the Sobol' design
 * first_index + n_base > 2^30.                                                                                            */
int pem_saltelli_profile_f64_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, const int32_t* kind,
                                 const double* a, const double* b, int n_varied, const int32_t* varied, int norm,
                                 const double* centre, double torr2pa, double radius, double* partial, uint64_t* flags, int n_blocks,
                                 pem_stream_t stream);
int pem_saltelli_profile_qmc_f64_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, int scramble,
                                     const int32_t* kind, const double* a, const double* b, int n_varied, const int32_t* varied,
                                     int norm, const double* centre, double torr2pa, double radius, double* partial, uint64_t* flags,
                                     int n_blocks, pem_stream_t stream);

/* ---- the model's Jacobian and the sums of a derivative-based sensitivity study (csrc/pem_jacobian.hip) --------------------
 * The three reduced QoIs f = (V_cc, div_angle, T_c) of the coupled fp64 model and d f_q / d x_i in physical units, exact and on the
 * branch the evaluation takes (csrc/pem_jacobian.h states the chain): V_cc clamped to 0 has a zero row and T sees no cathode input;
 * V_cc clamped to V_a has dV_cc/dV_a = 1; a1 clipped at pi/2 has no derivative with respect to P_b, c2, c3.
 * x: [15][n] DEVICE doubles, rows as pem_coupled_f64_dev's inputs.  varied: n_varied HOST indices 0..14 in any order (n_varied may be
 * 0, then `varied` and `jac` may be NULL).  qoi[3][n], jac[3][n_varied][n], flags[n]: bit 0 a non-physical thruster result (T < 0 or
 * I_B0 < 0), bit 1 an invalid plume row.  PEM_ERR_INVALID_ARG, nothing launched: n_varied outside 0..15, an index outside 0..14,
 * radius <= 0, a NULL array with n > 0.                                                                                       */
int pem_coupled_jacobian_f64_dev(size_t n, const double* x, int n_varied, const int32_t* varied, double torr2pa, double radius,
                                 double* qoi, double* jac, uint8_t* flags, pem_stream_t stream);
/* One launch: row A of the design of pem_saltelli_f64_dev / pem_saltelli_qmc_f64_dev (samples first_index .. first_index + n - 1,
 * bit-identical to pem_sample_f64_dev / pem_sample_sobol_f64_dev), the function above on it, the gradient in the prior's own
 * coordinate -- g_i = df/dx_i, or (x_i ln 10) df/dx_i for a PEM_DIST_LOGUNIFORM input -- and per QoI q, about the centre c_q
 * (`centre`: 3 DEVICE doubles, or NULL for zeros), with d = n_varied, partial[n_blocks][2 + 2 d + d (d + 1) / 2][3]:
 *   row 0                 sum (f - c)
 *   row 1                 sum (f - c)^2
 *   rows 2 .. 1 + d       sum g_i
 *   rows 2 + d .. 1 + 2d  sum g_i^4
 *   rows 2 + 2d ..        sum g_i g_j for i <= j, the upper triangle row by row
 * flags[n_blocks][3]: non-physical thruster results, invalid plume rows, skipped samples -- a sample with an f or a g that is not
 * finite adds nothing to any sum.  One deterministic partial per workgroup (no floating-point atomics); n = 0 writes zeros.
 * PEM_ERR_INVALID_ARG, nothing launched: n_varied outside 0..15, an index outside 0..14, n_blocks < 1, radius <= 0, a NULL output,
 * an unknown distribution kind, and for the Sobol' design first_index + n > 2^30.                                           */
int pem_gradient_sums_f64_dev(size_t n, uint64_t first_index, uint64_t seed, uint32_t stream_id, const int32_t* kind, const double* a,
                              const double* b, int n_varied, const int32_t* varied, const double* centre, double torr2pa,
                              double radius, double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream);
int pem_gradient_sums_qmc_f64_dev(size_t n, uint64_t first_index, uint64_t seed, uint32_t stream_id, int scramble,
                                  const int32_t* kind, const double* a, const double* b, int n_varied, const int32_t* varied,
                                  const double* centre, double torr2pa, double radius, double* partial, uint64_t* flags,
                                  int n_blocks, pem_stream_t stream);

/* ---- the Sobol' study over a pressure sweep (csrc/pem_sobol_sweep.hip) --------------------------------------------------
 * scripts/pem_v0/sobol.py:46-118 (compute_indices; uqtils sobol_sa, third-party: parity UNPINNED): per QoI group only the
 * exogenous inputs of the component that produces it are varied, every other input sits at a pin, at each of n_p background
 * pressures.  ONE launch covers one group at every pressure (blockIdx.y = pressure):
 *   group PEM_SWEEP_CATHODE   QoI V_cc                     varied P_b T_e V_vac Pstar P_T       (input rows 0 2 3 4 5)
 *         PEM_SWEEP_THRUSTER  QoIs T, u_ion(uion_z)        varied P_b mdot_a T_e a_1            (input rows 0 6 2 7)
 *         PEM_SWEEP_PLUME     QoI j_ion(gamma = 0)         varied P_b c0..c5 sigma_cex          (input rows 0 8..14)
 *   The Thruster group runs cathode -> thruster test double (u_ion = v_exh / (1 + exp(-100 (uion_z - 0.04))),
 *   sim_hallthruster.jl:46-47); the Plume group runs the plume alone at I_B0 = i_b0 and r = radius.
 * kind, a, b: DEVICE arrays [n_p][15] (rows as pem_coupled_f64_dev's inputs), the PEM_DIST_* prior of every input at each
 *   pressure; for an input outside the group's varied set only a[p][d] is read: the value it is pinned at.
 * Streams: attempt k of row r (0: A, 1: B) of group g at pressure p is stream 2 * 3 * n_p * k + 2 (g n_p + p) + r of the
 *   counter-based design (seed; base samples first_index ..): the numbers of pem_sample_f64_dev for that stream and table.
 *   Only the Plume group makes attempts k > 0: a row whose j_ion profile reaches spike_threshold anywhere on the 91-angle
 *   grid is redrawn, at most max_attempts times (sobol.py:50-66).  The accepted set does not depend on the launch shape.
 * clip (Plume only, DEVICE [n_p] or NULL): every j_ion(0) of pressure p -- A, B and AB -- is min(j, clip[p]) (sobol.py:82-89).
 * j0_out (Plume only, DEVICE [n_p][2 n_base] or NULL): the PRE-PASS; j_ion(0) of the accepted rows A (at [p][i]) and B
 *   (at [p][n_base + i]), unclipped, is written and no estimator sums are formed (partial may be NULL).
 * partial: DEVICE [n_p][n_blocks][2 + 4 nv][nq] fp64, one deterministic partial per workgroup.  Rows: sum fA + fB,
 *   sum fA^2 + fB^2, then per varied input j: sum t1, sum t1^2, sum t2, sum t2^2 with t1 = fB (fAB_j - fA),
 *   t2 = (fA - fAB_j)^2.  nq = 2 (T, u_ion) for the Thruster group, 1 otherwise.
 * flags: DEVICE [n_p][n_blocks][4] counts: non-physical thruster results (thruster.py:490-493, T < 0 or I_B0 < 0) and invalid
 *   plume samples (plume.py:105) among the evaluations, rejected draws, rows never accepted within max_attempts.           */
#define PEM_SWEEP_CATHODE 0
#define PEM_SWEEP_THRUSTER 1
#define PEM_SWEEP_PLUME 2
#define PEM_SWEEP_MAX_PRESSURES 65535
int pem_sobol_sweep_f64_dev(int group, size_t n_base, uint64_t first_index, uint64_t seed, int n_p, const int32_t* kind,
                            const double* a, const double* b, double torr2pa, double radius, double i_b0, double uion_z,
                            double spike_threshold, int max_attempts, const double* clip, double* j0_out, double* partial,
                            uint64_t* flags, int n_blocks, pem_stream_t stream);

/* ---- the same study through the chained surrogate (csrc/pem_surrogate_sobol.hip) ----------------------------------------------
 * scripts/pem_v0/sobol.py:70-98: model() takes V_cc, T and u_ion(z = L_ch) from `SURR.predict` of the component chain; only j_ion
 * goes to the true plume model.  ONE launch covers the Cathode or the Thruster group at every pressure, with the chain's cathode
 * table (and, for the Thruster group, the coupling map and the thruster table) in the analytic stages' place; the plume table is
 * checked and never read.  PEM_SWEEP_PLUME is refused: that group stays on pem_sobol_sweep_f64_dev.
 * group, n_base, first_index, seed, n_p, kind, a, b: as pem_sobol_sweep_f64_dev.
 * Streams: row r (0: A, 1: B) of group g at pressure p is stream 2 (g n_p + p) + r, base samples first_index ..: exactly
 *   pem_sobol_sweep_f64_dev's rows (attempt 0) for the same seed and tables, so a model sweep and a surrogate sweep see one design.
 * n_dim, vcc_slot, ib0_slot, stages, vcc_lo, vcc_w: the chain, as pem_sparse_predict_chain_fields_f64_dev takes it (the thruster
 *   table has 2 + u_rank outputs).  The I_B0 slot is never written.
 * slot_row, slot_log, slot_a, slot_w: HOST arrays [n_dim - 2]; entry k describes the k-th external coordinate (row k of the
 *   parents' t: the slots other than vcc_slot and ib0_slot, in order) and reads input row slot_row[k] (0 .. 14, distinct).
 *   Coordinates:  u = slot_log[k] ? log10(x) : x;  t = 2.0 * (u - slot_a[k]) / slot_w[k] - 1.0, left to right, no contraction,
 *   slot_w = b - a formed in fp64 by the caller (calibration.SurrogatePosterior.assemble_inputs' expression).  A varied input takes
 *   x from the design row, any other input its pin a[p][row].  Every input the group varies must have a slot.
 * u_rank (0 .. 14), u_dof, u_norm, u_scale, u_basis: the thruster stage's field as pem_sparse_predict_chain_fields_f64_dev takes
 *   it (u_lat0 == 2); u_cell (0 .. u_dof - 1): the one cell of the profile the study reads.
 * QoIs: Cathode V_cc; Thruster T (the thruster table's output 1) and u = denorm(v), v = 0; v = fma(l_q, u_basis[u_cell][q], v).
 *   With u_rank == 0 the u column of every output is NaN.
 * f_out (DEVICE [n_p][nv + 2][nq][n_base] or NULL): every f; evaluation 0 is row A, 1 row B, 2 + j row A with varied input j
 *   from B.  For tests: production passes NULL.
 * partial: DEVICE [n_p][n_blocks][2 + 4 nv][nq], rows and nq as pem_sobol_sweep_f64_dev's, one deterministic partial per workgroup.
 * flags: DEVICE [n_p][n_blocks][2] counts over the evaluations: non-physical thruster values (T < 0 or I_B0 < 0), and V_cc
 *   coupling coordinates outside [-1, 1] (the thruster table is extrapolated there; counted for the Cathode group too).
 * Bit contracts (tests/test_chain_sobol.py):
 *   1. Every f equals, bit for bit, the V_cc / T row and column u_cell of u_field that
 *      pem_sparse_predict_chain_fields_f64_dev gives at the same coordinates (u_rank == 0: pem_sparse_predict_chain_f64_dev's rows).
 *      An AB evaluation whose swapped input the cathode table does not read reuses row A's V_cc coordinate: the same bits.
 *   2. An f depends on seed, the sample's index first_index + i, the tables and the chain only -- not on n_base, n_blocks or
 *      whether f_out is asked for.
 * LDS: the larger of the cathode's and (Thruster group) the thruster's outer bases, n_dim coordinates per thread and about 2 KB
 * of accumulators and tables, at most 160 KB; above 64 KB it is requested as the chained launches request it.  Every argument is
 * checked before the device is.                                                                                              */
int pem_chain_sobol_sweep_f64_dev(int group, size_t n_base, uint64_t first_index, uint64_t seed, int n_p, const int32_t* kind,
                                  const double* a, const double* b, int n_dim, int vcc_slot, int ib0_slot,
                                  const pem_surr_stage* stages, double vcc_lo, double vcc_w, const int32_t* slot_row,
                                  const int32_t* slot_log, const double* slot_a, const double* slot_w, int u_rank, int u_dof,
                                  int u_norm, double u_scale, const double* u_basis, int u_cell, double* f_out, double* partial,
                                  uint64_t* flags, int n_blocks, pem_stream_t stream);

/* ---- differential evolution over the prior's quantile cube (csrc/pem_de.hip, hallthrusterpem_amd/optimize.py) ---------------
 * Stands in for run_mle(optimizer='evolution') (scripts/pem_v0/mcmc.py:170-231): scipy's differential_evolution semantics
 * (best1bin or rand1bin, F ~ U(mut_lo, mut_hi) once per generation, binomial crossover with probability cr and one forced
 * dimension, deferred updating, components leaving (0, 1) redrawn uniformly), MAXIMISING f over u in (0, 1)^ndim; theta =
 * the prior transform of u (kind/a/b: HOST arrays of ndim, as pem_sample_f64_dev).  One workgroup, one thread per member.
 * DEVICE arrays: pop_u, trial_u, theta [pop][ndim]; pop_f, trial_f [pop]; state [1]; record [3]; history [history_len] or NULL.
 * state = g counts the launches so far (the caller zeroes it; a captured graph advances it on every replay):
 *   g == 0  trial_u holds the initial design: it is clamped into [2^-53, 1 - 2^-53] and theta = its transform.
 *   g >= 1  1. the trials (u in trial_u, values in trial_f) replace the members they beat (all of them when g == 1);
 *           NaN and -inf never beat anything.  2. record = {best value, best index, converged}: the largest value (NaN / -inf
 *           rank as -inf; ties to the lowest index) and std(f) <= atol + tol |mean(f)| (sums in a fixed order; a non-finite
 *           member is never converged); history[g - 1] = best value when g - 1 < history_len.  3. unless finalize, the next
 *           trials from Philox4x32-10(counter = (member, g, purpose, pair), key = seed) into trial_u and their transform
 *           into theta, and state = g + 1.  With finalize, theta = the transform of the population and state is kept.
 * 4 <= pop <= PEM_DE_MAX_POP, 1 <= ndim <= PEM_DE_MAX_DIM.                                                                 */
#define PEM_DE_MAX_POP 1024
#define PEM_DE_MAX_DIM 16
#define PEM_DE_BEST1BIN 0
#define PEM_DE_RAND1BIN 1
int pem_de_step_f64_dev(int pop, int ndim, int strategy, int finalize, uint64_t seed, double mut_lo, double mut_hi, double cr,
                        double tol, double atol, const int32_t* kind, const double* a, const double* b, double* pop_u,
                        double* pop_f, double* trial_u, const double* trial_f, double* theta, uint64_t* state, double* record,
                        double* history, size_t history_len, pem_stream_t stream);

/* ---- bounded Nelder-Mead, many simplices, one launch per iteration (csrc/pem_nm.hip, optimize.NelderMead) -------------------
 * Stands in for minimize(obj_fun, x0, method='Nelder-Mead', bounds=bds, tol=1e-4, options={'adaptive': True}) of run_mle
 * (scripts/pem_v0/mcmc.py:170-231, the default optimizer): scipy's _minimize_neldermead for n_simplex independent simplices of
 * dimension ndim, one wave64 workgroup each, MAXIMISING f over x in [lb, ub]^ndim (g = -f is minimised; a NaN f is g = +inf).
 * Every point an iteration can ask for is emitted before it starts; the caller evaluates f on all of them between launches.
 * kind/a/b (the prior table, theta = the prior transform of x, as pem_de_step_f64_dev) and lb/ub are HOST arrays of ndim.
 * rho, chi, psi, sigma are scipy's coefficients (1, 2, 0.5, 0.5, or adaptive 1, 1 + 2/d, 0.75 - 1/(2d), 1 - 1/d).
 * DEVICE arrays, S = n_simplex, d = ndim:
 *   sim [S][d+1][d], fsim [S][d+1]   the simplex, best vertex first, and f there (a NaN f is stored as -inf)
 *   cand_x [S][d+4][d]               the pending points; theta [S*(d+4)][d] their transform, the rows f is called on
 *   cand_f [S][d+4]                  f of those rows, written by the caller between launches
 *   state [S][PEM_NM_STATE_WORDS]    0 launches, 1 nit, 2 nfev, 3 status (0 running, 1 converged), 4-8 the counts of
 *                                    reflections, expansions, outside contractions, inside contractions and shrinks, 9 the code
 *                                    of the last operation (1 ... 5 in that order, 0 none).  The caller zeroes word 0.
 *   history [history_len][S] or NULL   the best f after launch l >= 1 goes to row l - 1 when l - 1 < history_len
 * By the launch counter l = state word 0 of a simplex:
 *   l == 0  the caller's simplex (already inside the bounds) is emitted: rows 0 ... d are its vertices, rows d+1 ... d+3 repeat
 *           vertex 0.  Words 1-9 are zeroed, l = 1.  With finalize nothing happens.
 *   l == 1  rows 0 ... d of cand_f are the vertices' values: nit = 1, nfev = d + 1; sort, test, emit.
 *   l >= 2  resolve: with gr, ge, gc, gcc the values of rows 0-3 and g the sorted simplex values,
 *             gr < g[0]: the expansion (row 1) if ge < gr, else the reflection (row 0); nfev += 2
 *             else gr < g[d-1]: the reflection; nfev += 1
 *             else gr < g[d]: the outside contraction (row 2) if gc <= gr, else shrink; nfev += 2
 *             else: the inside contraction (row 3) if gcc < g[d], else shrink; nfev += 2
 *           the taken row replaces the worst vertex; a shrink replaces vertices 1 ... d by rows 4 ... d+3, nfev += d.  nit += 1.
 *   sort    stable: the rank of vertex i is #{j : g_j < g_i or (g_j == g_i and j < i)}.
 *   test    converged when max|sim[1:] - sim[0]| <= xatol and max|g[0] - g[1:]| <= fatol (a NaN or infinite difference is not).
 *           A converged simplex is frozen: only its launch counter and its history column move from then on.
 *   emit    (not converged, not finalize) with xbar = (((sim[0] + sim[1]) + ...) + sim[d-1]) / d and w = sim[d], each clipped as
 *           min(max(., lb), ub), products and sums rounded separately:
 *             row 0  (1 + rho) xbar - rho w           row 2  (1 + psi rho) xbar - psi rho w
 *             row 1  (1 + rho chi) xbar - rho chi w   row 3  (1 - psi) xbar + psi w
 *             rows 4 ... d+3  sim[0] + sigma (sim[j] - sim[0]), j = 1 ... d
 *           and l += 1.
 *   finalize  resolve, sort and test as above without emitting; all d + 4 rows of the simplex's block of theta become the
 *           transform of its best vertex; l is kept.  The search cannot be continued after it.
 * No atomics, no communication between workgroups: the same bits on every run.
 * Refused with PEM_ERR_INVALID_ARG before the device is looked at: n_simplex 0, ndim outside [1, PEM_NM_MAX_DIM], a NULL array
 * other than history, lb > ub, a negative or NaN tolerance, a history with history_len 0.                                  */
#define PEM_NM_MAX_DIM 32
#define PEM_NM_STATE_WORDS 10
int pem_nm_step_f64_dev(size_t n_simplex, int ndim, int finalize, double rho, double chi, double psi, double sigma, double xatol,
                        double fatol, const int32_t* kind, const double* a, const double* b, const double* lb, const double* ub,
                        double* sim, double* fsim, double* cand_x, const double* cand_f, double* theta, uint64_t* state,
                        double* history, size_t history_len, pem_stream_t stream);

/* ---- bounded Powell, many searches, one launch per function value (csrc/pem_powell.hip, optimize.Powell) --------------------
 * Stands in for minimize(obj_fun, x0, method='Powell', bounds=bds, options={'maxiter': maxfev, 'ftol': tol}) of run_mle
 * (scripts/pem_v0/mcmc.py:170-231, optimizer='powell'): scipy 1.15's _minimize_powell with its bounded line search
 * (_linesearch_powell, _line_for_search, _minimize_scalar_bounded) for n_search independent searches of dimension ndim, one
 * wave64 workgroup each, MAXIMISING f over x in [lb, ub]^ndim (g = -f is minimised; a NaN f is g = +inf).  A launch takes the
 * value of the point it emitted last, advances the algorithm until the next value is needed, and emits that point.
 * kind/a/b (the prior table, theta = the prior transform of x, as pem_de_step_f64_dev) and lb/ub are HOST arrays of ndim.
 * sqrt_eps = sqrt(2.2e-16) and golden_mean = 0.5 (3 - sqrt(5)) as the host rounds them; max_iter 0 is no limit.
 * DEVICE arrays, S = n_search, d = ndim:
 *   vec [S][PEM_POWELL_VEC_ROWS][d]  rows 0 x (the point after the last completed line search), 1 x1 (x when the iteration
 *                                    before ended), 2 p and 3 xi (base and direction of the line search in progress; xi also
 *                                    keeps the displacement while the extrapolated point is out), 4 best_x, 5 the emitted point
 *   direc [S][d][d]                  the direction set, one direction per row
 *   scal [S][PEM_POWELL_SCALARS]     0-14 of _minimize_scalar_bounded: a, b, fulc, nfc, xf, rat, e, fx, ffulc, fnfc, fu, xm, tol1,
 *                                    tol2, and the alpha emitted last; 15-18 of the outer loop: fx, fval, fx2, delta; 19 best_f,
 *                                    the largest f consumed (at best_x).  All but best_f are values of g = -f.
 *   cand_f [S]                       f of the emitted rows, written by the caller between launches;  theta [S][d] those rows
 *   state [S][PEM_POWELL_STATE_WORDS]  0 launches, 1 nit, 2 nfev, 3 status (0 running, 1 the ftol test met, 2 max_iter reached),
 *                                    4 phase (0 the value of x0 pending, 1 line search i, 2 the value of the extrapolated point
 *                                    pending, 3 the extra line search), 5 i, 6 bigind, 7 num (values the line search has had),
 *                                    8 line searches started, then the counts of 9 golden steps, 10 parabolic steps taken,
 *                                    11 parabolas rejected, 12 parabolic steps moved off an interval end, 13 steps lengthened to
 *                                    tol1, 14 extrapolations clipped by a bound (lmax < 1), 15 extra line searches, 16 direction
 *                                    replacements, 17 line searches that returned a worse value than they started from, 18 zero
 *                                    directions skipped, 19 all-zero displacements, 20 line bounds with lmax <= lmin, 21 line
 *                                    searches of one value, 22 line searches ended by the 500-value cap, 23 spare.
 *                                    The caller zeroes word 0.
 *   history [history_len][S] or NULL   best_f after launch l >= 1 goes to row l - 1 when l - 1 < history_len
 * By the launch counter l = state word 0 of a search:
 *   l == 0  the caller has put x0 (already inside the bounds) into row 0 of vec and the directions into direc.  x0 is copied to
 *           the other rows of vec and emitted; scal is zeroed (best_f = -inf), words 1-23 are zeroed, l = 1.
 *   l >= 1, status 0  g = -cand_f (+inf for a NaN); nfev += 1; best_f / best_x take it when l == 1 or g < -best_f.  Then by phase
 *             0: fval = g; an iteration begins (fx = fval, bigind = 0, delta = 0, i = 0) with line search 0.
 *             1, 3: the value enters _minimize_scalar_bounded where it waited.  While |xf - xm| > tol2 - (b - a) / 2 and num <
 *                500 the next alpha is scipy's (parabolic when |e| > tol1 and the parabola is acceptable AND p, q and p / q are
 *                finite, else golden; moved off an end; lengthened to tol1) and p + alpha xi is emitted.  Otherwise the line
 *                search is done: x = p + xf xi, fval = its fx; phase 1: delta / bigind, i += 1 and line search i, or the end
 *                of the iteration; phase 3: when xf xi is not all zero direc[bigind] = direc[d-1], direc[d-1] = xf xi; the next
 *                iteration begins.
 *             2: fx2 = g; when fx > fx2 and t < 0 (scipy's t) the extra line search from x along the displacement starts,
 *                otherwise the next iteration begins.
 *           A line search starts with p = x and (a, b) = _line_for_search(p, xi) over the non-zero components of xi, (0, 0)
 *           when b < a or either is not finite, tolerance xatol = (xtol * 100) / 100, and emits p + fulc xi, fulc = a +
 *           golden_mean (b - a); a zero direction is skipped.  The end of an iteration: nit += 1; status 1 when 2 (fx - fval) <=
 *           ftol (|fx| + |fval|) + 1e-20, else status 2 when nit >= max_iter, else xi = x - x1, x1 = x and x + min(lmax, 1) xi
 *           is emitted, lmax of _line_for_search(x, xi), 1 for an all-zero xi (scipy raises there).  Every emitted point, and x,
 *           is min(max(., lb), ub): rounding can carry p + alpha xi one ulp past a bound.  Products and sums are rounded
 *           separately.  l += 1.
 *   l >= 1, status != 0  frozen: the emitted point is x and stays; only l and the history column move.
 *   finalize 1  consumes nothing: the search's row of theta becomes the transform of x, whose value is fval (exactly what scipy
 *           returns when maxfev interrupts a line search); l is kept.  finalize 2: the same with best_x, whose value is best_f.
 *           Nothing happens to a search with l == 0.
 * No atomics, no communication between workgroups: the same bits on every run.
 * Refused with PEM_ERR_INVALID_ARG before the device is looked at: n_search 0, ndim outside [1, PEM_POWELL_MAX_DIM], finalize
 * outside 0 ... 2, a NULL array other than history, lb > ub, a negative or NaN tolerance, sqrt_eps or golden_mean outside (0, 1), an unknown prior
 * kind, a history with history_len 0.                                                                                      */
#define PEM_POWELL_MAX_DIM 32
#define PEM_POWELL_STATE_WORDS 24
#define PEM_POWELL_SCALARS 20
#define PEM_POWELL_VEC_ROWS 6
int pem_powell_step_f64_dev(size_t n_search, int ndim, int finalize, double xtol, double ftol, uint64_t max_iter, double sqrt_eps,
                            double golden_mean, const int32_t* kind, const double* a, const double* b, const double* lb,
                            const double* ub, double* vec, double* direc, double* scal, const double* cand_f, double* theta,
                            uint64_t* state, double* history, size_t history_len, pem_stream_t stream);

/* ---- DIRECT, one search with its rectangles on the device, many values per launch (csrc/pem_direct.hip, optimize.Direct) ----
 * Stands in for direct(obj_fun, bds, eps=1, maxiter=maxfev, locally_biased=False) of run_mle (scripts/pem_v0/mcmc.py:170-231,
 * optimizer='direct'): scipy 1.15's DIRECT without local bias, one workgroup, MAXIMISING f over x in [lb, ub]^ndim (g = -f + 0 is
 * minimised).  A launch takes the values of the rows it emitted last, completes the divisions they belong to, selects when the
 * round's queue is empty, and emits the points of as many queued rectangles as fit into `rows`; the consumed rows, in order,
 * are scipy's evaluation sequence.  kind/a/b (the prior table, theta = the prior transform of x) and lb/ub are HOST arrays of ndim.
 * DEVICE arrays, d = ndim, D = n_depth:
 *   thirds [D + 1]      thirds[0] = 1, thirds[i] = 1 / h, h = 3 multiplied by 3 after each entry, as the host rounds them
 *   levels [D d]        levels[i d + j] = w[j] / h, w[j] = sqrt(d - j + j / 9.) * 0.5, h = 1 multiplied by 3 after each i
 *   centres [cap][d]    the centre c of every rectangle in the unit cube; the point evaluated for it is (c + xs2) xs1 with
 *                       xs1 = ub - lb, xs2 = lb / xs1, the sum and the product rounded separately
 *   values [cap]        g at the centre;  expo [cap][d] int32: side i is 3^-expo[i];  level [cap] int32: k d + (d - p) with
 *                       k = min_i expo[i], p = the sides with expo[i] == k; the rectangle's size measure is levels[level]
 *   queue [PEM_DIRECT_MAX_LEVELS] int32   the rectangles the current round divides, in ascending level
 *   rowinfo [rows][2] int32   of the rows emitted last: the rectangle divided (-1 a left-over row, -2 the start's centre) and
 *                       2 side + (1 for c - delta, 0 for c + delta)
 *   cand_f [rows]       f of the emitted rows, written by the caller between launches;  theta [rows][d] those rows
 *   state [PEM_DIRECT_STATE_WORDS]  0 launches, 1 nit, 2 nfev (= the rectangles stored), 3 status, 4 queue head, 5 queue length,
 *                       6 the lowest index of the lowest g, 7 rows emitted last, 8 ties met (below), 9 the launch counter after the
 *                       launch that ended the search.  The caller zeroes word 0.
 *   history [history_len][PEM_DIRECT_HISTORY_COLS] or NULL   after launch l >= 1, row l - 1: the best f, nfev, nit
 * By the launch counter l = state word 0:
 *   l == 0  words 1-9 are zeroed; centre 0 = 0.5 in every coordinate is emitted as row 0 (the other rows carry it too); l = 1.
 *   l >= 1, status 0
 *     1. consume: g = -cand_f + 0 of the rows emitted last.  One that is not finite: status 7, nothing is stored.  Otherwise
 *        row r becomes rectangle nfev + r.  A divided rectangle's 2 |I| rows are always in one launch: with k = min expo,
 *        I = its sides with expo == k ascending and w_i = min(g+, g-), the sides are taken in ascending w (stably); each
 *        raises expo[i] by one and its two children copy expo as it then is.  The best index moves to the lowest new index of
 *        the lowest new g when that is strictly below the best g.
 *     2. when the queue is empty the round has ended.  After the start's value: the queue is rectangle 0.  Otherwise nit += 1
 *        and, in this order: status 1 when nfev > max_fun; 4 when the product of thirds[expo[i]] of the best rectangle, taken
 *        in ascending i, is < vol_tol; 5 when its levels[level] < len_tol; 2 when nit + 1 >= max_iter (nit = max(max_iter, 2),
 *        as scipy reports it: max_iter allows max_iter - 2 selections).  Else the selection: per level the lowest g and the
 *        lowest index that has it (the anchor); walking the levels upwards an anchor is kept iff its g is strictly below every
 *        anchor's before it; while more than one is kept, the last kept j is dropped when g_j - lo levels[level_j] > gmin - eps
 *        |gmin|, lo = the minimum over the kept i before j of (g_i - g_j) / (levels[level_i] - levels[level_j]) -- difference,
 *        quotient and product rounded separately --, and the pruning ends at the first j that stays.  Status 6 when the kept
 *        anchors' points do not fit into cap or one of them has k + 2 > n_depth; else they are the queue.
 *     3. emit: rectangles are popped from the queue while their 2 |I| points fit into the rows left: for i in I ascending
 *        c + thirds[k + 1] e_i, then c - thirds[k + 1] e_i.  Left-over rows carry the best point; their values are ignored.
 *   l >= 1, status != 0  frozen: every row is the best point and stays; only l and the history move.
 *   finalize 1  consumes nothing: row 0 of theta becomes the best centre's point; l is kept.  Nothing happens when l == 0.
 * Statuses 1, 2, 4 and 5 are scipy's (its f_min stop, 3, is not offered).  Two are not: 6, the store or the level table
 * cannot hold the next round (scipy allocates what maxfun needs and stops with an error); 7, a value was NaN or infinite
 * (scipy replaces such points by a rule that is not restated).  Ties -- equal g inside a level, equal w across sides -- are
 * outside the contract (scipy divides every tied rectangle; here the lowest index wins) and are counted in word 8.
 * Integer minima in LDS on an order-preserving key of g, no floating-point atomics: the same bits on every run.
 * Refused with PEM_ERR_INVALID_ARG before the device is looked at: ndim outside [1, PEM_DIRECT_MAX_DIM], rows outside
 * [2 ndim, PEM_DIRECT_MAX_ROWS], cap outside [2 ndim + 1, PEM_DIRECT_MAX_STORE], n_depth outside [2, PEM_DIRECT_MAX_DEPTH] or
 * n_depth ndim > PEM_DIRECT_MAX_LEVELS, finalize outside 0 ... 1, eps negative, NaN or infinite, vol_tol or len_tol outside
 * [0, 1], max_iter 0, a NULL array other than history, lb >= ub or a bound that is not finite, an unknown prior kind, a history
 * with history_len 0.                                                                                                      */
#define PEM_DIRECT_MAX_DIM 32
#define PEM_DIRECT_MAX_LEVELS 1024
#define PEM_DIRECT_MAX_DEPTH 64
#define PEM_DIRECT_MAX_ROWS 1024
#define PEM_DIRECT_MAX_STORE 16777216
#define PEM_DIRECT_STATE_WORDS 10
#define PEM_DIRECT_HISTORY_COLS 3
int pem_direct_step_f64_dev(int ndim, int rows, size_t cap, int n_depth, int finalize, double eps, double vol_tol, double len_tol,
                            uint64_t max_iter, uint64_t max_fun, const int32_t* kind, const double* a, const double* b,
                            const double* lb, const double* ub, const double* thirds, const double* levels, double* centres,
                            double* values, int32_t* expo, int32_t* level, int32_t* queue, int32_t* rowinfo, const double* cand_f,
                            double* theta, uint64_t* state, double* history, size_t history_len, pem_stream_t stream);

/* ---- delayed-rejection adaptive Metropolis, one launch per step (csrc/pem_dram.hip, calibration.DeviceDRAM) -----------------
 * Stands in for uq.dram(fun, p0, niter, adapt_after, adapt_interval, eps, gamma) of run_mcmc (scripts/pem_v0/mcmc.py:275-300;
 * uqtils is third-party and absent: parity UNPINNED, the algorithm is calibration.DRAM's) for n_chains chains of dimension
 * ndim, one wave64 workgroup per chain.  All state is in DEVICE arrays of the caller:
 *   theta [K][d], logp [K]        the current point and its log posterior
 *   L [K][d][d]                   lower Cholesky factor of the proposal covariance, row-major
 *   mean [K][d], scatter [K][d][d]  running moments of the chain (Welford); the start point is observation 1
 *   prop [2][K][d]                the pending proposals y1 (block 0) and y2 (block 1): the caller evaluates the log posterior on
 *   prop_logp [2][K]              prop seen as (2K, d) and writes the 2K values here between two launches
 *   state [K]                     launches seen by the chain (the caller zeroes it; a captured graph advances it on every replay)
 *   accepted [2][K]               acceptances per stage;   flags [K]: bit 0 = an adaptation was skipped (see 3.)
 *   trace [trace_len][K][d], logp_trace [trace_len][K]   either may be NULL
 *   draws NULL or [K][2d + 2]     z1[d], z2[d], u1, u2 as the launch used them for the step it resolved
 * Launch s = state[k].  s == 0: nothing is pending.  s >= 1 resolves step s:
 *   a1 = exp(min(lp1 - lp0, 0)) (a NaN difference stays NaN and is rejected), accepted when u1 < a1; otherwise y2 is accepted
 *   when log(u2) < (lp2 - lp0) + log_q + log1p(-a1_rev) - log1p(-a1), a1_rev = exp(min(lp1 - lp2, 0)),
 *   log_q = -(|w|^2 - |z1|^2) / 2, w = z1 - sqrt(gamma) z2 (= L^-1 (y1 - y2)); z1, z2 are recomputed from their counters.  Then
 *   1. theta, logp and accepted are updated; with r = s - 1 - trace_first the point goes to row r / thin of the traces when
 *      r >= 0, r mod thin == 0 and r / thin < trace_len;
 *   2. count = s + 1, delta = theta - mean, mean += delta / count, scatter_ij += delta_i (theta_j - mean_j);
 *   3. when s >= adapt_after and (s - adapt_after) mod adapt_interval == 0: L = the Cholesky factor (row by row, lower triangle
 *      of the argument) of (2.4^2 / d) (scatter / (count - 1) + eps I), built in LDS and committed only if every pivot is > 0;
 *      otherwise L is kept whole and bit 0 of flags[k] is set.
 * Every launch then draws the proposals of step s + 1, y1_j = x_j + sum_{i<=j} L_ji z1_i and y2_j = x_j + sqrt(gamma) sum_{i<=j}
 * L_ji z2_i (i ascending, products and sums rounded separately), and sets state[k] = s + 1.  The draws of step s are
 * Philox4x32-10(counter = (chain, s mod 2^32, purpose, pair), key = seed): purposes 0x44520000 (z1), 0x44520001 (z2) -- pair p
 * gives dimensions 2p and 2p + 1, each normcdfinv((2k + 1) 2^-53) of a 52-bit k -- and 0x44520002, whose pair 0 gives
 * u1 = u53(x, y) and u2 = u53(z, w).  No atomics, no communication between workgroups: the same bits on every run.
 * Refused with PEM_ERR_INVALID_ARG before the device is looked at: n_chains 0, ndim outside [1, PEM_DRAM_MAX_DIM], gamma not > 0,
 * eps < 0, adapt_interval 0, thin 0, a NULL required array, a trace with trace_len 0.                                        */
#define PEM_DRAM_MAX_DIM 32
int pem_dram_step_f64_dev(size_t n_chains, int ndim, uint64_t seed, double gamma, double eps, uint64_t adapt_after,
                          uint64_t adapt_interval, uint64_t trace_first, size_t trace_len, uint64_t thin, double* theta,
                          double* logp, double* L, double* mean, double* scatter, double* prop, const double* prop_logp,
                          uint64_t* state, uint64_t* accepted, uint32_t* flags, double* trace, double* logp_trace, double* draws,
                          pem_stream_t stream);

/* ---- affine-invariant ensemble sampler, one launch per half-step (csrc/pem_ensemble.hip, calibration.DeviceEnsemble) --------
 * Goodman & Weare's stretch move and ter Braak's DE move as emcee runs them (third-party and absent: parity UNPINNED; the
 * launch is restated in tests/ensemble_np.py) for n_ensembles independent ensembles of n_walkers = K walkers (K even, H = K / 2)
 * of dimension ndim = d, one workgroup per ensemble.  The halves are fixed: half 0 is walkers [0, H), half 1 walkers [H, K).
 * Half-step s = 1, 2, ... moves half (s - 1) mod 2 against the other, the complement; two half-steps are a step.  All state is
 * in DEVICE arrays of the caller:
 *   theta [E][K][d], logp [E][K]  the walkers and their log posteriors
 *   prop [E][H][d]                the pending proposals of the half that moves: the caller evaluates the log posterior on prop
 *   prop_logp [E][H]              seen as (E H, d) and writes the E H values here between two launches
 *   log_q [E][H]                  log of the proposal weight of each pending proposal (written by the launch that proposed)
 *   state [E]                     launches seen by the ensemble (the caller zeroes it; a captured graph advances it)
 *   accepted [E][K]               acceptances per walker
 *   trace [trace_len][E][K][d], logp_trace [trace_len][E][K]   either may be NULL
 *   draws NULL or [E][H][6]       per moving walker: move (0 stretch, 1 DE), z or g, j1, j2 (-1: none) and, in column 5, u_move
 *                                 of the half-step PROPOSED by the launch; in column 4 u_acc of the half-step it RESOLVED
 * Launch s = state[e].  s == 0: nothing is pending.  s >= 1 resolves half-step s: walker m of the moving half takes its proposal
 * and prop_logp iff log(u_acc) < log_q + (prop_logp - logp) (a NaN on either side compares false; -inf is never accepted; a
 * walker at -inf takes any finite value).  When s is even, step t = s / 2 has ended: with r = t - 1 - trace_first the ensemble
 * goes to row r / thin of the traces when r >= 0, r mod thin == 0 and r / thin < trace_len.  Every launch then proposes
 * half-step s + 1 from the complement as it now stands, and sets state[e] = s + 1.  One u_move per (ensemble, half-step) picks
 * the move of the whole half, DE when u_move < de_fraction:
 *   stretch  z = ((a - 1) u + 1)^2 / a,  y = x_j1 + z (x_w - x_j1),      log_q = (d - 1) log z
 *   DE       g = g0 (1 + sigma n),        y = x_w + g (x_j1 - x_j2),      log_q = 0
 * products and sums rounded separately.  Draws: Philox4x32-10(counter = (ensemble, half-step mod 2^32, purpose, m), key = seed),
 * m the walker's index in its half: purpose 0x454E0000 (m = 0) u_move = u53(x, y); 0x454E0001 j1 = (x H) >> 32, j2 =
 * (y (H - 1)) >> 32 plus 1 if >= j1, u = u53(z, w) or n = normcdfinv((2k + 1) 2^-53) of the 52-bit k from (z, w); 0x454E0002
 * u_acc = u53(x, y).  No atomics, no communication between workgroups: the same bits on every run.
 * Refused with PEM_ERR_INVALID_ARG before the device is looked at: n_ensembles 0, n_walkers odd or outside
 * [2, PEM_ENSEMBLE_MAX_WALKERS], de_fraction > 0 with n_walkers < 4, ndim outside [1, PEM_ENSEMBLE_MAX_DIM], a not finite or
 * not > 1, de_fraction outside [0, 1], g0 not > 0, sigma < 0, either not finite, thin 0, a NULL required array, a trace with
 * trace_len 0.                                                                                                                 */
#define PEM_ENSEMBLE_MAX_DIM 32
#define PEM_ENSEMBLE_MAX_WALKERS 1024
int pem_ensemble_step_f64_dev(size_t n_ensembles, int n_walkers, int ndim, uint64_t seed, double a, double de_fraction, double g0,
                              double sigma, uint64_t trace_first, size_t trace_len, uint64_t thin, double* theta, double* logp,
                              double* prop, const double* prop_logp, double* log_q, uint64_t* state, uint64_t* accepted,
                              double* trace, double* logp_trace, double* draws, pem_stream_t stream);

/* ---- replica exchange over the ensemble sampler, one launch per half-step (csrc/pem_tempering.hip,
 * calibration.DeviceTemperedEnsemble) -- parallel tempering as ptemcee runs it over emcee (third-party and absent: parity UNPINNED;
 * the rules are the ones below, restated in tests/tempering_np.py).  n_replicas = R independent replicas of a ladder of
 * n_temperatures = T inverse temperatures 1 = beta[0] > beta[1] > ... > beta[T-1] >= 0; ensemble e = r T + t samples
 * prior(x) likelihood(x)^beta[t] with K walkers in the two fixed halves of pem_ensemble_step_f64_dev, E = R T ensembles in all,
 * one workgroup per REPLICA.  All state is in DEVICE arrays of the caller, beta included:
 *   beta [T]                      the ladder; the caller guarantees finite, strictly decreasing values in [0, 1]
 *   theta [E][K][d]               the walkers;  loglik [E][K], logprior [E][K]: their log likelihoods and log priors, all finite
 *   prop [E][H][d]                the pending proposals: the caller evaluates both functions on prop seen as (E H, d) and writes
 *   prop_loglik, prop_logprior [E][H]   the values here between two launches
 *   log_q [E][H]                  log of the proposal weight of each pending proposal
 *   state [R]                     launches seen by the replica (the caller zeroes it; a captured graph advances it)
 *   accepted [E][K]               accepted moves per walker
 *   swap_attempts, swap_accepted [R][T-1]   walker pairs offered a swap / swapped, per (replica, lower temperature t of the pair
 *                                 (t, t + 1)); may be NULL when T == 1
 *   trace [trace_len][E][K][d], loglik_trace, logprior_trace [trace_len][E][K]   each may be NULL
 *   draws NULL or [E][H][6]       as pem_ensemble_step_f64_dev reports them
 * Launch s = state[r].  s == 0: nothing is pending.  s >= 1 resolves half-step s with pem_ensemble_step_f64_dev's draws (the
 * ensemble word of the counter is e): walker m of the moving half takes its proposal, prop_loglik and prop_logprior iff both
 * values are finite and
 *   log(u_acc) < (log_q + (prop_logprior - logprior)) + beta[t] (prop_loglik - loglik)
 * at every temperature, beta = 0 included, so that beta loglik is never 0 inf.  When s is even, step n = s / 2 has ended and the
 * SWAPS of step n follow: in every replica the pairs (t, t + 1) with t = n mod 2, n mod 2 + 2, ... and t + 1 < T (every ensemble
 * is in at most one pair; the top of the ladder idles when its pair is not due); walker k of t and walker k of t + 1 exchange
 * theta, loglik and logprior iff
 *   log(u_swap) < (beta[t] - beta[t+1]) (loglik[t+1][k] - loglik[t][k])
 * with u_swap = u53(x, y) of Philox4x32-10(counter = (r T + t, n mod 2^32, 0x454E0003, k), key = seed) -- the purpose word keeps
 * it apart from the move draws 0x454E0000 ... 0x454E0002 -- and the pair's counters advance by K and by the number swapped.  Then,
 * with q = n - 1 - trace_first, the ladder as the swaps left it goes to row q / thin of the traces when q >= 0, q mod thin == 0
 * and q / thin < trace_len.  Every launch then proposes half-step s + 1 as pem_ensemble_step_f64_dev does and sets
 * state[r] = s + 1.  Products and sums are rounded separately, and log_q = (d - 1) log z of the stretch takes its log through
 * IEEE operations alone (csrc/pem_ensemble_moves.h, log_restatable: fdlibm's e_log.c, below 1 ulp), so that the restatement holds
 * EVERY state word bit for bit; pem_ensemble_step_f64_dev asks the library, whose last bit is its own.  With T == 1 and
 * logprior == 0 the launch therefore visits pem_ensemble_step_f64_dev's points on finite values -- the same draws, proposals and
 * decisions, log_q within an ulp.  No atomics, no communication between workgroups, no cooperative launch: the same bits on
 * every run.
 * Refused with PEM_ERR_INVALID_ARG before the device is looked at: n_replicas 0, n_temperatures < 1, n_replicas n_temperatures
 * or n_temperatures n_walkers ndim above INT_MAX, everything pem_ensemble_step_f64_dev refuses about n_walkers, ndim, a,
 * de_fraction, g0, sigma and thin, a NULL required array, NULL swap counters with T > 1, a trace with trace_len 0.           */
int pem_tempered_ensemble_step_f64_dev(size_t n_replicas, int n_temperatures, int n_walkers, int ndim, uint64_t seed, double a,
                                       double de_fraction, double g0, double sigma, const double* beta, uint64_t trace_first,
                                       size_t trace_len, uint64_t thin, double* theta, double* loglik, double* logprior,
                                       double* prop, const double* prop_loglik, const double* prop_logprior, double* log_q,
                                       uint64_t* state, uint64_t* accepted, uint64_t* swap_attempts, uint64_t* swap_accepted,
                                       double* trace, double* loglik_trace, double* logprior_trace, double* draws,
                                       pem_stream_t stream);

/* ---- tempered sequential Monte Carlo, two launches (csrc/pem_smc.hip, calibration.DeviceSMC) -------------------------------
 * TMCMC (Ching & Chen 2007) / the SMC sampler of Del Moral et al. 2006 as PyMC's sample_smc runs it (third-party and absent:
 * parity UNPINNED; the rules are the ones below, restated in tests/smc_np.py).  n_populations = R independent populations of
 * n_particles = N particles of dimension ndim = d move from the law the caller drew them from (beta = 0) to prior x likelihood
 * (beta = 1) along prior x likelihood^beta.  All state is in DEVICE arrays of the caller:
 *   theta [R][N][d], loglik [R][N], logprior [R][N]   the particles and their values; logprior finite, loglik may be anything
 *   beta [R], log_evidence [R]    the inverse temperature reached and the log evidence accumulated (the caller zeroes both)
 *   stage [R]                     stages completed (the caller zeroes it)
 *   L [R][d][d]                   lower Cholesky factor of the proposal covariance, row-major
 *   prop [R][N][d]                the pending proposals: the caller evaluates both functions on prop seen as (R N, d) and writes
 *   prop_loglik, prop_logprior [R][N]   the values here between two launches
 *   accept_count [R][N]           uint32: moves of the current stage each particle accepted (what keeps the move launch free of
 *                                 atomics; the stage launch sums and zeroes it)
 *   accepted [R]                  accepted moves of the last stage whose moves have ended: set by the stage launch that follows
 *                                 them and kept until the next stage's moves have ended (the caller zeroes it)
 *   flags [R]                     bit 0: a Cholesky factor was refused; bit 1: no particle had a finite log likelihood
 *   moves_active [R]              uint32: set by the stage launch, read by the move launch
 *   scratch [R][N][d + 2]         the resampling gather's staging area
 *   hist_beta, hist_ess, hist_accept, hist_dlogz [R][history_len]   per stage s = 0, 1, ... (stages past history_len are not
 *                                 recorded): beta', ESS(beta'), accepted / (N n_mcmc), the evidence increment
 *   record (stage launch)  NULL or [R][3N + Nd + 1 + d + d d]: w [N] un-normalised, W [N] normalised, ancestors [N] (as doubles),
 *                                 the normals of the proposals [N][d], u of the resampler, mean [d], cov [d][d] (before scale, eps)
 *   record (move launch)   NULL or [R][N][d + 2]: the normals of the proposals it drew [d], then u and the decision (0 / 1) of the
 *                                 proposal it resolved
 *
 * pem_smc_stage_f64_dev: one workgroup of 1024 per population, thread t holding particles t P ... t P + P - 1, P = ceil(N / 1024).
 *   0. If moves_active: accepted = sum of accept_count, and with s = stage >= 1, hist_accept[s - 1] = accepted / (N n_mcmc).
 *      If beta is not < 1 the population is finished: moves_active = 0 and nothing else changes, so a replay after that changes
 *      no word at all.
 *   1. l_max = the largest finite loglik; a loglik that is not finite has weight 0 at every temperature.  No finite value: bit 1
 *      of flags is set, moves_active = 0, nothing else changes.  Otherwise w_i(b) = exp((b - beta) (l_i - l_max)) and
 *      ESS(b) = (sum w)^2 / sum w^2.  beta' = 1 if ESS(1) >= tau N; otherwise PEM_SMC_BISECTIONS halvings of [lo, hi] = [beta, 1],
 *      mid = 0.5 (lo + hi), lo = mid if ESS(mid) >= tau N else hi = mid, and beta' = lo if lo > beta else hi: every stage advances.
 *   2. log_evidence += log(sum w(beta') / N) + (beta' - beta) l_max; N counts the particles of weight 0 as well.
 *   3. mean_j = (sum_i w_i x_ij) / sum w, cov_jk = (sum_i (w_i (x_ij - mean_j)) (x_ik - mean_k)) / sum w, and L = the Cholesky factor
 *      (column by column, from the lower triangle) of scale^2 cov + eps I, committed only if every pivot is > 0; otherwise L is kept
 *      whole and bit 0 of flags is set (pem_dram_step_f64_dev's rule).
 *   4. Systematic resampling: u = u53(x, y) of Philox4x32-10(counter = (population, new stage number mod 2^32, 0x534D0000, 0),
 *      key = seed); ancestor a_j = the smallest i with C_i > (((j + u) / N) C_{N-1}), clamped to the last particle of positive
 *      weight.  C is the inclusive cumulative sum of w in this FIXED ORDER: C_i = W_v + (O_t + c_i), where c_i is the running
 *      sum of thread t's own P weights in particle order, O_t the running sum, from 0, of the totals (last c) of the threads
 *      before t in its wave of 64 threads, W_v the running sum, from 0, of the totals (O + total of the wave's last thread) of the
 *      waves before wave v; particles past N count as weight 0.  Every level starts where the one below ends, so C never
 *      decreases.  theta, loglik and logprior are gathered through scratch; accept_count is zeroed.
 *   5. The history row s = stage; beta = beta', stage += 1, moves_active = 1.
 *   6. The proposals of move 1 of the new stage (below).
 * pem_smc_move_f64_dev: workgroups of 256 over 64 particles each; for the populations with moves_active it resolves proposal
 * `move` (1 ... n_mcmc) of the stage: a particle takes prop, prop_loglik and prop_logprior iff both values are finite and
 *   log(u) < (prop_logprior - logprior) + beta (prop_loglik - loglik)
 * (symmetric proposal; a NaN on either side compares false; refused at beta = 0 as well, so beta loglik is never 0 inf), u =
 * u53(x, y) of counter (population N + particle, (stage n_mcmc + move) mod 2^32, 0x534D0002, 0), and accept_count += 1.  Unless
 * propose == 0 it then draws proposal move + 1, y_j = x_j + sum_{i<=j} L_ji z_i (i ascending, products and sums rounded
 * separately), z_2p and z_2p+1 from counter (population N + particle, (stage n_mcmc + move + 1) mod 2^32, 0x534D0001, p), each
 * normcdfinv((2k + 1) 2^-53) of a 52-bit k as pem_dram_step_f64_dev draws them.  `stage` is the number of the stage the move
 * belongs to (1 for the first).  The last move of a stage, move == n_mcmc, must come with propose == 0: its proposals would be
 * drawn under the word (stage + 1) n_mcmc + 1 of the next stage launch's own.  tau, scale and eps are checked and not used.
 * No atomics, no communication between workgroups, no cooperative launch: the same bits on every run.
 * PEM_SMC_MAX_PARTICLES is 16384: what limits it is the one LDS array of N doubles (128 KiB of a CU's 160) in which the stage
 * workgroup holds l - l_max, then the weights, then their cumulative sums, then the ancestors.
 * Both refuse with PEM_ERR_INVALID_ARG before the device is looked at: n_populations 0, n_particles outside
 * [2, PEM_SMC_MAX_PARTICLES], ndim outside [1, PEM_SMC_MAX_DIM], n_populations n_particles above 2^32 - 1, tau not in (0, 1), scale
 * not finite or not > 0, eps < 0, n_mcmc 0, a NULL required array (everything but record), history_len 0 (stage), move outside
 * [1, n_mcmc], move == n_mcmc with propose != 0, or n_populations ceil(n_particles / 64) above INT_MAX (move).                                                      */
#define PEM_SMC_MAX_DIM 32
#define PEM_SMC_MAX_PARTICLES 16384
#define PEM_SMC_BISECTIONS 52
int pem_smc_stage_f64_dev(size_t n_populations, int n_particles, int ndim, uint64_t seed, double tau, double scale, double eps,
                          uint32_t n_mcmc, double* theta, double* loglik, double* logprior, double* beta, double* log_evidence,
                          uint64_t* stage, double* L, double* prop, uint32_t* accept_count, uint64_t* accepted, uint32_t* flags,
                          uint32_t* moves_active, double* scratch, double* hist_beta, double* hist_ess, double* hist_accept,
                          double* hist_dlogz, size_t history_len, double* record, pem_stream_t stream);
int pem_smc_move_f64_dev(size_t n_populations, int n_particles, int ndim, uint64_t seed, double tau, double scale, double eps,
                         uint32_t n_mcmc, uint32_t move, int propose, double* theta, double* loglik, double* logprior,
                         const double* beta, const uint64_t* stage, const double* L, double* prop, const double* prop_loglik,
                         const double* prop_logprior, uint32_t* accept_count, const uint32_t* moves_active, double* record,
                         pem_stream_t stream);

/* ---- MCMC chain diagnostics (hallthrusterpem_amd/diagnostics.py; the lag sums of uq.autocorrelation at
 * scripts/pem_v0/mcmc.py:310 -- uqtils, third-party, parity UNPINNED).  x: fp64 [n_rows][ld], unit column stride (a
 * (n, K, d) trace seen as n rows of K*d series; the pointer needs only 8-byte alignment).  Segment s is rows
 * s*seg_stride ... s*seg_stride + seg_len - 1 (whole chains: n_seg 1; split halves: n_seg 2, seg_len floor(n/2),
 * seg_stride ceil(n/2)).  With N = seg_len and y_t = x_t - mean, for i < n_lags, l = lag0 + i*lag_step:
 *   mean[s][c]    = (1/N) sum_{t<N} x_t
 *   acov[s][i][c] = (1/N) sum_{t<N-l} y_t y_{t+l}        (values centred as they are staged, before the products)
 * A non-finite value makes that series' mean and every acov NaN in that segment; other series are untouched.  The sums
 * run in an order that depends on N and the series only: the same bits on every run and whichever other lags the call
 * asks for.  work: DEVICE scratch of work_len >= n_seg * ceil(seg_len / PEM_CHAIN_TIME_BLOCK) * n_lags * n_series
 * doubles (one partial per time block).  Refused with PEM_ERR_INVALID_ARG: a zero size, ld < n_series, seg_len < 2, a
 * segment past n_rows, a lag >= seg_len, lag_step 0, a null pointer, a short workspace.  lag_step > 1 costs what the
 * lags lag0 ... lag0 + (n_lags - 1) lag_step cost, less the 128-lag blocks that hold no requested lag.              */
#define PEM_CHAIN_TIME_BLOCK 4096
int pem_chain_autocov_f64_dev(size_t n_rows, size_t n_series, size_t ld, const double* x, size_t n_seg, size_t seg_len,
                              size_t seg_stride, size_t lag0, size_t lag_step, size_t n_lags, double* mean, double* acov,
                              double* work, size_t work_len, pem_stream_t stream);

/* ---- marginals of a pooled MCMC trace (csrc/pem_marginals.hip, hallthrusterpem_amd/marginals.py; the arrays behind
 * uq.ndscatter at scripts/pem_v0/mcmc.py:339-385 -- uqtils, third-party, parity UNPINNED; the definitions are numpy's
 * np.histogram / np.histogram2d with range= given and scipy.stats.gaussian_kde's formula).  x: fp64 [n_rows][ld], unit
 * column stride, n_par <= ld columns used, read in place (8-byte alignment suffices).  Every array is a DEVICE array.
 *
 * pem_chain_hist_f64_dev: edges [n_par][bins + 1], non-decreasing per parameter (the caller's np.linspace).  A value v of
 * parameter i is in bin k iff edges[i][k] <= v < edges[i][k+1], the last bin also taking v == edges[i][bins]; anything else
 * (outside, NaN, +-inf) is in no bin.  The decision is a comparison against the table.
 *   hist1d[i][k]          draws with parameter i in bin k
 *   hist2d[p][ki][kj]     pair p = (i, j), i < j, in the order (0,1), (0,2) ... (n_par-2, n_par-1): draws with parameter i in
 *                         bin ki AND parameter j in bin kj; NULL: 1-D only
 *   dropped[i]            draws of parameter i in no bin;  nonfinite[i]: how many of those were NaN or +-inf
 * Exact 64-bit counts (integer adds: the same for every run).  The outputs are zeroed by the call.
 *
 * pem_chain_kde_f64_dev: grid [n_par][n_grid], inv_h [n_par] (1 / bandwidth), scale [n_par] (inv_h / (n_rows sqrt(2 pi))):
 *   kde[i][q] = scale[i] * sum_t exp(-((grid[i][q] - x[t][i]) * inv_h[i])^2 / 2)
 * a direct, untruncated sum; the difference grid - x is formed first.  Each wave sums its rows of a PEM_KDE_ROW_BLOCK-row
 * block in increasing t, the 4 wave sums are added in order, one partial per row block goes to work (work_len >=
 * ceil(n_rows / PEM_KDE_ROW_BLOCK) * n_par * n_grid doubles) and the partials are added in block order: the same bits on
 * every run, and a grid point's value does not depend on the other grid points.  A NaN inv_h gives NaN for that parameter.
 *
 * Refused with PEM_ERR_INVALID_ARG: a zero size, n_par outside 1 ... PEM_MARGINALS_MAX_PAR, bins outside 1 ...
 * PEM_MARGINALS_MAX_BINS, n_grid > PEM_KDE_MAX_GRID, ld < n_par, a null pointer (hist2d excepted), a short workspace,
 * n_rows beyond one launch.  For the counts: a workgroup's 32-bit tables must see fewer than 2^32 rows, and the launch
 * has floor(1024 / task blocks) row blocks (at most; task blocks = ceil(tables / min(256, floor(9216 / bins^2))), tables = n_par or
 * n_par (n_par + 1) / 2), so n_rows >= 2^32 * floor(1024 / task blocks) is refused: 2^42 with one task block, 2^40 at
 * n_par = 17, bins = 15.  For the density: more than 65535 row blocks, n_rows > 65535 * PEM_KDE_ROW_BLOCK.              */
#define PEM_MARGINALS_MAX_PAR 32
#define PEM_MARGINALS_MAX_BINS 64
#define PEM_HIST_ROW_TILE 128
#define PEM_KDE_MAX_GRID 4096
#define PEM_KDE_ROW_BLOCK 4096
int pem_chain_hist_f64_dev(size_t n_rows, int n_par, size_t ld, const double* x, int bins, const double* edges,
                           uint64_t* hist1d, uint64_t* hist2d, uint64_t* dropped, uint64_t* nonfinite, pem_stream_t stream);
int pem_chain_kde_f64_dev(size_t n_rows, int n_par, size_t ld, const double* x, size_t n_grid, const double* grid,
                          const double* inv_h, const double* scale, double* kde, double* work, size_t work_len,
                          pem_stream_t stream);

/* ---- hexagonal pair bins of a pooled MCMC trace (csrc/pem_hexbin.hip, marginals.hexbins / corner(plot2d='hex'); the pair
 * panels of uq.ndscatter(..., plot2d='hex') at scripts/pem_v0/mcmc.py:344-385 -- uqtils UNPINNED; the definition is
 * matplotlib's Axes.hexbin with C=None, linear scales, gridsize=(nx, ny) and extent= given, bit for bit).  x as above: DEVICE,
 * fp64 [n_rows][ld], n_par <= ld columns used, read in place.
 *   lattice [n_par][4]     HOST array, {x0, sx, y0, sy} per parameter: with the parameter's extent (lo, hi) and
 *                          pad = 1e-9 (hi - lo), x0 = lo - pad, sx = ((hi + pad) - x0) / nx, y0 = lo, sy = (hi - lo) / ny
 *                          (matplotlib pads x only).  Read and checked before the call returns; it travels as a kernel argument.
 *   counts [P][n_cells]    DEVICE, zeroed by the call; P = n_par (n_par - 1) / 2 pairs (i, j), i < j, in the order (0,1), (0,2)
 *                          ... (n_par-2, n_par-1), parameter i the x and j the y coordinate; n_cells = (nx+1)(ny+1) + nx ny
 * A draw (x, y) of a pair, every operation rounded once and none contracted:
 *   ix = (x - x0_i) / sx_i,  iy = (y - y0_j) / sy_j;  r1 = rint(ix) (half to even), s1 = rint(iy), r2 = floor(ix), s2 = floor(iy)
 *   d1 = (ix - r1)^2 + 3.0 (iy - s1)^2,  d2 = (ix - r2 - 0.5)^2 + 3.0 (iy - s2 - 0.5)^2
 *   d1 <  d2: counted in cell r1 (ny+1) + s1                  iff 0 <= r1 <= nx and 0 <= s1 <= ny
 *   else    : counted in cell (nx+1)(ny+1) + r2 ny + s2       iff 0 <= r2 <  nx and 0 <= s2 <  ny     (ties: second lattice)
 * The range tests are made on the floating-point r, s: a draw outside the lattice, NaN or +-inf in either coordinate is
 * dropped from that pair only.  Exact 64-bit counts (integer adds: the same for every run and whichever other parameters
 * the call holds).  Cell k < (nx+1)(ny+1) has its centre at (x0 + (k / (ny+1)) sx, y0 + (k % (ny+1)) sy); cell
 * (nx+1)(ny+1) + k at (x0 + (k / ny + 0.5) sx, y0 + (k % ny + 0.5) sy): matplotlib's get_offsets() order.
 * Refused with PEM_ERR_INVALID_ARG before any device call: a zero size, n_par outside 2 ... PEM_MARGINALS_MAX_PAR, nx or ny
 * outside 1 ... PEM_HEX_MAX_GRID, ld < n_par, a null pointer, a lattice entry that is not finite, sx or sy not positive,
 * n_rows beyond one launch (a workgroup's 32-bit tables must see fewer than 2^32 rows; the launch has floor(1024 / task
 * blocks) row blocks of PEM_HEX_ROW_TILE-row tiles, task blocks = ceil(P / min(256, floor(9216 / n_cells)))).           */
#define PEM_HEX_MAX_GRID 64
#define PEM_HEX_ROW_TILE 128
int pem_chain_hex_f64_dev(size_t n_rows, int n_par, size_t ld, const double* x, int nx, int ny, const double* lattice,
                          uint64_t* counts, pem_stream_t stream);

/* ---- all-pairs Gaussian log-density with a log-sum-exp over the inner draws (csrc/pem_information.hip,
 * hallthrusterpem_amd/information.py: the nested Monte Carlo estimator of the expected information gain of groups of
 * measurements, Ryan 2003, Huan & Marzouk 2013; the reference has no such analysis, nothing to pin).
 *   z_out [n_out][ld_out]  DEVICE, the standardised observations of the outer draws, n_col <= ld_out columns used
 *   z_in  [n_in][ld_in]    DEVICE, the standardised predictions of the inner draws
 *   group_end [n_groups]   HOST: group c is the columns group_end[c-1] ... group_end[c] - 1 (group_end[-1] = 0); read and checked
 *                          before the call returns, it travels as a kernel argument.  Set n_groups is the union of all columns.
 *   lse, ess [n_out][n_groups + 1]  DEVICE
 * For every outer row i and set c, all in fp64:
 *   d2_c(i, j) = sum_{k in c} (z_out[i][k] - z_in[j][k])^2   the direct form, one fma chain in increasing k; the union's d2 is the
 *                                                            sum of the groups' d2 of the same (i, j), added in group order
 *   l = -d2 / 2,  m = max_j l,  s1 = sum_j exp(l - m),  s2 = sum_j exp(l - m)^2
 *   lse[i][c] = m + log s1 - log n_in        ess[i][c] = s1^2 / s2     (1 <= ess <= n_in: the inner draws that carry the sum)
 * The n_out x n_in matrix is never written: a workgroup owns 32 outer rows and a block of PEM_INFORMATION_INNER_BLOCK inner
 * rows, stages PEM_INFORMATION_CHUNK columns of both operands at a time, and leaves one (m, s1, s2) per (block, row, set) in
 * work; a second launch merges the blocks in block order.  No floating-point atomics.  The bits of row i depend on that row,
 * z_in and the groups only -- not on n_out, the grid or the other rows of the call.
 * The domain is finite inputs whose d2 stays finite (an infinite d2 for every j of a block gives NaN).
 * pem_pairwise_lse_work_len: the doubles of work, ceil(n_in / PEM_INFORMATION_INNER_BLOCK) n_out (n_groups + 1) 3; 0 for a
 * zero size, n_groups outside [1, PEM_INFORMATION_MAX_GROUPS] or a product past size_t.  Host only.
 * Refused with PEM_ERR_INVALID_ARG before any device call: a zero size, n_groups outside [1, PEM_INFORMATION_MAX_GROUPS], a null
 * pointer, ld_out or ld_in < n_col, group_end not strictly ascending from above 0 or not ending at n_col, work_len short,
 * more than 65535 inner blocks, n_col > INT_MAX - PEM_INFORMATION_CHUNK.                                           */
#define PEM_INFORMATION_MAX_GROUPS 32
#define PEM_INFORMATION_CHUNK 16
#define PEM_INFORMATION_INNER_BLOCK 512
int pem_pairwise_lse_f64_dev(size_t n_out, size_t n_in, int n_col, const double* z_out, size_t ld_out, const double* z_in,
                             size_t ld_in, int n_groups, const int* group_end, double* lse, double* ess, double* work,
                             size_t work_len, pem_stream_t stream);
size_t pem_pairwise_lse_work_len(size_t n_out, size_t n_in, int n_groups);

/* ---- the conditional term of the information gain about a subset of the inputs (csrc/pem_information_theta.hip,
 * hallthrusterpem_amd/information.py `about=`): every outer draw's log-mean-exp over its OWN set of predictions, straight from the
 * output of the system-predict launch.
 *   z_out [n_out][ld_out]       DEVICE, the standardised observations, n_col <= ld_out columns used
 *   pred  [n_out n_per][ld_pred] DEVICE, the raw predictions, padding records included; outer row i owns rows i n_per ... (i+1) n_per - 1
 *   col   [n_col]               DEVICE, nullable (= identity, then n_col <= ld_pred): the record index of column k.  An index outside
 *                               [0, ld_pred) is not read: the column counts as NaN
 *   scale [n_col]               DEVICE, nullable (= 1): the factor of column k
 *   group_end [n_groups]        HOST, as in pem_pairwise_lse_f64_dev; set n_groups is the union of all columns
 *   lse, ess [n_out][n_groups + 1], used [n_out]   DEVICE
 * For outer row i, its row l and set c, all in fp64:
 *   v_k  = fl64(pred[i n_per + l][col[k]] * scale[k])        the product is rounded before the subtraction
 *   d2_c = sum_{k in c} (z_out[i][k] - v_k)^2                one fma chain in increasing k; the union's d2 is the sum of the groups'
 *                                                            d2 of the same row, added in group order
 *   a row is used iff its union d2 is finite (a NaN or inf in one of its columns leaves it out of EVERY set); used[i] counts them
 *   l = -d2 / 2,  m = max l,  s1 = sum exp(l - m),  s2 = sum exp(l - m)^2   over the used rows
 *   lse[i][c] = m + log s1 - log used[i]      ess[i][c] = s1^2 / s2;   used[i] = 0 gives NaN for both
 * The gathered, scaled (n_out n_per, n_col) tensor is never written; pred is read once, a wave load covering 2 rows x
 * PEM_CONDITIONAL_CHUNK columns.  One workgroup of one wave per outer row walks its rows in tiles of 64 and merges the tiles in
 * their order: no floating-point atomics, and the bits of row i depend on that row, its n_per rows, col, scale and the groups
 * only -- not on n_out or the grid.
 * Refused with PEM_ERR_INVALID_ARG before any device call: a zero size, n_groups outside [1, PEM_INFORMATION_MAX_GROUPS], a null
 * pointer other than col and scale, ld_out < n_col, ld_pred < 1 (< n_col without col), group_end not strictly ascending from above
 * 0 or not ending at n_col, n_out n_per ld_pred or n_out ld_out doubles past size_t, n_out or n_per > INT_MAX,
 * n_col > INT_MAX - PEM_CONDITIONAL_CHUNK.                                                                          */
#define PEM_CONDITIONAL_CHUNK 32
int pem_conditional_lse_f64_dev(size_t n_out, size_t n_per, int n_col, const double* z_out, size_t ld_out, const double* pred,
                                size_t ld_pred, const int* col, const double* scale, int n_groups, const int* group_end, double* lse,
                                double* ess, int* used, pem_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PEM_HIP_H */
