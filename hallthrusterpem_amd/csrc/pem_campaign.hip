// pem_campaign.hip -- the host side of the fused campaign statistics, pem_coupled_mc_stats_f64_dev: a fused Monte-Carlo evaluation with
// the percentiles of its profile counted on the way (round 4) and the scalar QoIs' percentiles selected beside it.  It reaches the
// evaluation kernel (csrc/pem_kernels.hip) and the selection (csrc/pem_quantile.hip) through csrc/pem_qfused.h only.
#include <exception>
#include <functional>
#include <future>
#include <mutex>
#include <string>
#include <thread>

#include "pem_common.h"
#include "pem_qfused.h"

namespace {

using pem::aligned16;
using pem::check_device;
using pem::fail;

// The scalar QoIs' percentiles of a campaign, selected on a second host thread and stream while the calling thread takes the
// profile through its pilot, its counting launch and the passes over its records (csrc/pem_quantile.hip keeps a second set of
// buffers for it).  Two stages, each released on the host (a promise) and ordered on the device (an event): the scalars of the
// pilot's samples exist once the pilot evaluation is under way -- the worker brackets the wanted ranks from them while the
// counting launch runs -- and all of them once the counting launch (or, after a decline, the plain launch) is.
struct ScalarJob {
    struct Stage {
        std::promise<int> go;                  // 1: `ev` marks the launch; 0: give up (an error on the calling thread)
        std::future<int> gone;
        bool signalled = false;
        hipEvent_t ev = nullptr;
        Stage() : gone(go.get_future()) {}
        void signal(int v) {
            if (!signalled) {
                signalled = true;
                go.set_value(v);
            }
        }
        int launched(hipStream_t st) {         // after the launch has been enqueued on `st`
            if (signalled) return PEM_OK;
            HIP_TRY(hipEventRecord(ev, st));
            signal(1);
            return PEM_OK;
        }
        // the worker: block until the launch is under way, then make `side` wait for it
        int await(hipStream_t side) {
            if (gone.get() != 1) return fail(PEM_ERR_HIP, "pem_coupled_mc_stats (scalar selection): given up");
            HIP_TRY(hipStreamWaitEvent(side, ev, 0));
            return PEM_OK;
        }
    };
    Stage pilot, full;
    // The other direction: the counting launch must not START while the side selection's subsample passes are still running -- their
    // histograms take most of a CU's LDS, a workgroup of the persistent counting grid that finds no room waits for a whole pass of its
    // neighbours, and the launch takes 4 ms instead of 2.3 (seen in two calls of seven under the profiler, whose host threads are
    // slow).  The worker marks the end of those passes (`side`: released by the worker, awaited by the calling thread).
    Stage side;
    std::thread worker;
    std::function<void()> body;                // what the worker runs
    bool started = false;
    int rc = PEM_OK;
    std::string error;
    // Events and thread are made AFTER the pilot evaluation has been enqueued (McProducer::pilot): their 50-100 us of host time then
    // pass while the GPU works instead of in front of the call's first kernel.
    int start() {
        if (started) return PEM_OK;
        started = true;
        HIP_TRY(hipEventCreateWithFlags(&pilot.ev, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&full.ev, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&side.ev, hipEventDisableTiming));
        try {
            worker = std::thread(body);
        } catch (const std::exception& e) {    // (no thread to be had: nothing may leave a C entry point but its return code)
            return fail(PEM_ERR_HIP, "pem_coupled_mc_stats: could not start the scalar selection's thread: %s", e.what());
        }
        return PEM_OK;
    }
    int join() {
        pilot.signal(0);
        full.signal(0);
        if (worker.joinable()) worker.join();
        for (Stage* s : {&pilot, &full, &side}) {
            if (s->ev) (void)hipEventDestroy(s->ev);
            s->ev = nullptr;
        }
        return rc;
    }
    ~ScalarJob() { (void)join(); }
};

// a stream of the library's own per device (created once)
int side_stream(hipStream_t* out) {
    static std::mutex mu;
    static hipStream_t streams[64] = {};
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(PEM_ERR_INVALID_ARG, "device index out of range");
    std::lock_guard<std::mutex> lock(mu);
    // (a higher stream priority for the side work was measured and changes nothing: 3.85-3.92 ms per 1e7-sample campaign either way)
    if (!streams[dev]) HIP_TRY(hipStreamCreateWithFlags(&streams[dev], hipStreamNonBlocking));
    *out = streams[dev];
    return PEM_OK;
}

struct McProducer : pem::FusedProducer {
    pem::McLaunch a;
    bool store_profile;
    bool counted = false;                          // the counting launch is under way: every output but the percentiles gets written
    ScalarJob* job = nullptr;
    int pilot(size_t rows, double* dst, hipStream_t st) override {
        pem::McLaunch p = a;                       // samples 0 .. rows-1 of the same design; their profile rows go to dst
        p.n = rows;
        p.j_ion = dst;
        if (int rc = pem::launch_coupled_mc(p, st)) return rc;
        if (!job) return PEM_OK;
        if (int rc = job->start()) return rc;
        return job->pilot.launched(st);            // (their scalars too: the side selection's subsample)
    }
    int waves(int nq, unsigned* w) override { return pem::coupled_count_waves(a.n, nq, store_profile, w); }
    int count(const pem::CountIO& io, hipStream_t st) override {
        if (job && job->worker.joinable() && job->side.gone.get() == 1) HIP_TRY(hipStreamWaitEvent(st, job->side.ev, 0));   // (see ScalarJob::side)
        if (int rc = pem::launch_coupled_mc_count(a, io, store_profile, st)) return rc;
        counted = true;
        return job ? job->full.launched(st) : PEM_OK;    // (the side selection's passes over all samples may follow this launch)
    }
};
}  // namespace

extern "C" int pem_coupled_mc_stats_f64_dev(size_t n, uint64_t first_index, uint64_t seed, uint32_t stream_id, const int32_t* kind, const double* a,
                                 const double* b, double torr2pa, double radius, double* x_out, size_t ld, double* V_cc, double* I_B0,
                                 double* T, double* j_ion, double* pilot_rows, double* div_angle, double* T_c, uint8_t* invalid, int nq,
                                 const uint64_t* rank_prev, const uint64_t* rank_next, const double* gamma, double* q_out, double* q_scalars,
                                 int* fused_ok, int q25, int q75, double iqr_factor, uint8_t* row_certain, uint8_t* row_uncertain,
                                 int* premask_ok, pem_stream_t stream) {
    if (!kind || !a || !b || !V_cc || !div_angle || !T_c || !rank_prev || !rank_next || !gamma || !q_out || !fused_ok)
        return fail(PEM_ERR_INVALID_ARG, "pem_coupled_mc_stats: NULL array");
    if (!j_ion && !pilot_rows) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_mc_stats: without a profile array, room for the pilot rows is needed");
    if (j_ion && !aligned16(j_ion)) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_mc_stats: j_ion must be 16-byte aligned");
    if (pilot_rows && !aligned16(pilot_rows)) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_mc_stats: pilot_rows must be 16-byte aligned");
    if (x_out && ld < n) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_mc_stats: leading dimension smaller than n");
    if (nq < 1 || nq > PEM_QUANTILE_MAX_Q) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_mc_stats: 1 <= nq <= %d", PEM_QUANTILE_MAX_Q);
    if (n < PEM_MC_STATS_MIN_N) return fail(PEM_ERR_INVALID_ARG, "pem_coupled_mc_stats: at least %d samples", PEM_MC_STATS_MIN_N);
    // q_scalars: V_cc, div_angle, T_c must then be rows 0, 1, 2 of one [3][row stride >= n] array (the reduced-QoI tensor)
    const ptrdiff_t qstride = div_angle - V_cc;
    if (q_scalars && (qstride < (ptrdiff_t)n || T_c - div_angle != qstride))
        return fail(PEM_ERR_INVALID_ARG, "pem_coupled_mc_stats: q_scalars needs V_cc, div_angle, T_c as equally spaced rows of one array");
    if (int rc = check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ScalarJob job;
    McProducer prod;
    if (q_scalars) {
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        hipStream_t side = nullptr;
        if (int rc = side_stream(&side)) return rc;
        job.body = [&job, dev, side, n, nq, V_cc, qstride, rank_prev, rank_next, gamma, q_scalars]() {
            struct Release {                                             // (whatever happens: the calling thread is not left waiting)
                ScalarJob& j;
                ~Release() { j.side.signal(0); }
            } release{job};
            auto note = [&job](int rc) {
                job.rc = rc;
                if (rc != PEM_OK) job.error = pem_last_error();          // (the message lives in this thread's buffer)
                return rc;
            };
            if (hipSetDevice(dev) != hipSuccess) {
                (void)note(fail(PEM_ERR_HIP, "pem_coupled_mc_stats (scalar selection): hipSetDevice failed"));
                return;
            }
            if (note(job.pilot.await(side))) return;
            pem::SidePlan plan;
            plan.ctx = &job;
            plan.before_full = [](void* ctx, hipStream_t st) {
                ScalarJob* j = static_cast<ScalarJob*>(ctx);
                if (j->side.launched(st)) j->side.signal(0);             // the subsample's passes end here (on `st`, the side stream)
                return j->full.await(st);
            };
            (void)note(pem::quantiles_side(n, 3, V_cc, 1, (size_t)qstride, nq, rank_prev, rank_next, gamma, q_scalars, side, &plan));
        };
        prod.job = &job;
    }
    prod.a.n = n;
    prod.a.first_index = first_index;
    prod.a.seed = seed;
    prod.a.stream_id = stream_id;
    for (int d = 0; d < 15; ++d) {
        prod.a.kind[d] = kind[d];
        prod.a.a[d] = a[d];
        prod.a.b[d] = b[d];
    }
    prod.a.torr2pa = torr2pa;
    prod.a.radius = radius;
    prod.a.x_out = x_out;
    prod.a.ld = ld;
    prod.a.V_cc = V_cc;
    prod.a.I_B0 = I_B0;
    prod.a.T = T;
    prod.a.j_ion = j_ion;
    prod.a.div_angle = div_angle;
    prod.a.T_c = T_c;
    prod.a.invalid = invalid;
    prod.store_profile = j_ion != nullptr;
    if (row_certain && row_uncertain && premask_ok) {
        prod.pm_q25 = q25;
        prod.pm_q75 = q75;
        prod.pm_factor = iqr_factor;
        prod.pm_certain = row_certain;
        prod.pm_uncertain = row_uncertain;
    }
    if (premask_ok) *premask_ok = 0;
    *fused_ok = 0;
    // with a profile array the pilot rows are its own first rows (the counting launch writes the same values there again)
    if (int rc = pem::quantiles_fused(n, PEM_NANGLE, nq, rank_prev, rank_next, gamma, j_ion ? j_ion : pilot_rows, prod, q_out, fused_ok, st))
        return rc;                                 // (~ScalarJob tells the worker to give up and joins it)
    if (premask_ok) *premask_ok = (*fused_ok && prod.pm_done) ? 1 : 0;
    if (!*fused_ok && !prod.counted) {
        // declined before the counting launch (the fused form refused the call's shape), with nothing but the pilot's samples evaluated:
        // the plain launch makes every output complete.  (Declined AFTER it -- unfit brackets, a rank outside its bracket, record
        // overflow, a non-finite value -- the counting launch has written every output already; only the percentiles are missing.)
        if (int rc = pem::launch_coupled_mc(prod.a, st)) return rc;
        if (q_scalars) {
            if (int rc = job.start()) return rc;
            if (int rc = job.pilot.launched(st)) return rc;               // (no-ops for a stage that has been released)
            if (int rc = job.full.launched(st)) return rc;
        }
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (q_scalars) {                               // (both stages released by now on every path that comes here)
        if (int rc = job.join()) return fail(rc, "%s", job.error.c_str());
    }
    return PEM_OK;
}
