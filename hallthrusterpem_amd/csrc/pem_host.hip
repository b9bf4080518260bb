// pem_host.hip -- the host-pointer entry points of libpem_hip.so: the caller's arrays are staged through a device workspace in chunks
// and handed to the device-pointer entry points (pem_*_f64_dev, include/pem_hip.h).  With them the library's housekeeping calls:
// version, device count, pem_init (whose device these entry points run on), pem_synchronize.
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>

#include "pem_common.h"

namespace {

using pem::check_device;
using pem::fail;

constexpr int NANG = PEM_NANGLE;

std::atomic<int> g_device{-1};   // process default of the host-pointer entry points (pem_init); -1: the calling thread's

// Host-pointer entry points run on the device given to pem_init, whichever thread calls them: a new thread's current
// HIP device is 0, which is the wrong card for the worker threads of a one-process-per-GPU rank (gen_data.py:448-456
// evaluates models on Thread pools).
int use_default_device() {
    const int d = g_device.load(std::memory_order_relaxed);
    if (d >= 0) HIP_TRY(hipSetDevice(d));
    return PEM_OK;
}

// device workspace of the host-pointer entry points
struct Workspace {
    std::mutex mu;
    void* buf = nullptr;
    size_t cap = 0;
    int device = -1;
    int reserve(size_t bytes) {
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        if (buf && (cap < bytes || dev != device)) {
            (void)hipFree(buf);
            buf = nullptr;
            cap = 0;
        }
        if (!buf) {
            HIP_TRY(hipMalloc(&buf, bytes));
            cap = bytes;
            device = dev;
        }
        return PEM_OK;
    }
} g_ws;

// carve 256-byte aligned arrays out of the workspace (base == nullptr: only measure the layout, pem_host_plan)
struct Carver {
    unsigned char* base;
    size_t off = 0;
    explicit Carver(void* b) : base(static_cast<unsigned char*>(b)) {}
    template <class T>
    T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (count * sizeof(T) + 255) & ~size_t(255);
        return p;
    }
};

// Host <-> device movement of one chunk of a host-pointer entry point.  A chunk whose whole workspace footprint fits
// the pinned staging buffer is moved with ONE host-to-device and ONE device-to-host copy through a pinned mirror of the
// workspace layout (inputs are carved first, outputs after them, so each side is one contiguous range): a call with
// 15 input and 6 output arrays otherwise pays ~20 pageable-copy latencies (coupled, n = 1: 186 -> 61 us per call,
// tools/latency_probe.py).  The two sides decide separately: inputs are staged when they fit, outputs when the whole
// footprint does; what does not fit is copied array by array, where bandwidth is what matters.
constexpr size_t STAGE_BYTES = size_t(2) << 20;
struct Stage {
    unsigned char* pin = nullptr;
    bool tried = false;
    unsigned char* get() {
        if (!tried) {
            tried = true;
            void* p = nullptr;
            if (hipHostMalloc(&p, STAGE_BYTES, hipHostMallocPortable) == hipSuccess) pin = static_cast<unsigned char*>(p);
            else (void)hipGetLastError();
        }
        return pin;
    }
} g_stage;   // guarded by g_ws.mu

// Small calls skip the copies altogether: the kernels read their inputs from the pinned staging buffer and write their results
// to it over PCIe (hipHostMalloc memory is device-accessible at its host address and coherent), so a call is memcpy in, ONE launch,
// a stream synchronisation, memcpy out -- without the two copy-engine round trips: the calls amisc makes while it trains (a few to a
// few hundred samples) go from 33-35 to 27-29 us (cathode_coupling) and from 60-63 to 54-59 us (pem_v0_coupled), n = 1000: 113-148 ->
// 95-108 us (tools/latency_probe.py, interleaved; profiles/latency_r04.txt).  At 560 KB of footprint (BASELINE configs[0]: 1e4 cathode
// samples) the kernels' reads over the link cost what the copies saved: ZC_BYTES stays below that.  PEM_ZERO_COPY=0 switches it off.
constexpr size_t ZC_BYTES = size_t(256) << 10;
bool zero_copy_enabled() {
    static const bool on = !(getenv("PEM_ZERO_COPY") && atoi(getenv("PEM_ZERO_COPY")) == 0);
    return on;
}

// The workspace layout of one chunk of each host-pointer entry point: the inputs are carved first (they end at `in_end`), the
// outputs after them (they end at `end`).  With base == nullptr only the two offsets are computed: pem_host_plan measures the
// very layout the entry points carve.
struct CathodeArrays {
    double* d[7];           // six inputs, V_cc
    size_t in_end, end;
    CathodeArrays(void* base, size_t chunk) {
        Carver cv(base);
        for (int i = 0; i < 6; ++i) d[i] = cv.take<double>(chunk);
        in_end = cv.off;
        d[6] = cv.take<double>(chunk);
        end = cv.off;
    }
};
struct ThrusterArrays {
    double *in[4], *out[8];  // an output the caller does not ask for takes no room
    size_t in_end, end;
    ThrusterArrays(void* base, size_t chunk, const bool (&wanted)[8]) {
        Carver cv(base);
        for (auto& p : in) p = cv.take<double>(chunk);
        in_end = cv.off;
        for (int i = 0; i < 8; ++i) out[i] = wanted[i] ? cv.take<double>(chunk) : nullptr;
        end = cv.off;
    }
};
struct PlumeArrays {
    double *d[10], *j, *div, *tc;
    uint8_t* inv;
    size_t in_end, end;
    PlumeArrays(void* base, size_t chunk, size_t R) {
        Carver cv(base);
        for (auto& p : d) p = cv.take<double>(chunk);
        in_end = cv.off;
        j = cv.take<double>(chunk * NANG * R);
        div = cv.take<double>(chunk * R);
        tc = cv.take<double>(chunk * R);
        inv = cv.take<uint8_t>(chunk);
        end = cv.off;
    }
};
struct CoupledArrays {
    double *d[15], *vcc, *ib0, *T, *div, *tc, *j;
    uint8_t* inv;
    size_t in_end, end;
    CoupledArrays(void* base, size_t chunk) {
        Carver cv(base);
        for (auto& p : d) p = cv.take<double>(chunk);
        in_end = cv.off;
        vcc = cv.take<double>(chunk);
        ib0 = cv.take<double>(chunk);
        T = cv.take<double>(chunk);
        div = cv.take<double>(chunk);
        tc = cv.take<double>(chunk);
        inv = cv.take<uint8_t>(chunk);
        j = cv.take<double>(chunk * NANG);   // last: without a profile the staged copy-back stops before it
        end = cv.off;
    }
};

// What a host-pointer call does, decided before it touches the device (pem_host_plan reports exactly this): the samples per
// chunk, the workspace it reserves, where the carved inputs and outputs end, and how the chunk's data moves.
//   regime 0  zero-copy: the reserved bytes fit ZC_BYTES and PEM_ZERO_COPY allows it -- the arrays are carved in the pinned buffer
//   regime 1  inputs and outputs staged through the pinned mirror: the footprint fits STAGE_BYTES
//   regime 2  only the inputs staged: they end within STAGE_BYTES, the footprint does not
//   regime 3  array by array
struct HostPlan {
    size_t chunk, n_chunks, in_end, footprint, reserve;
    int regime;
};
HostPlan finish_plan(size_t n, size_t chunk, size_t in_end, size_t footprint, size_t reserve) {
    HostPlan pl{chunk, (n + chunk - 1) / chunk, in_end, footprint, reserve, 3};
    if (zero_copy_enabled() && reserve <= ZC_BYTES) pl.regime = 0;
    else if (footprint <= STAGE_BYTES) pl.regime = 1;
    else if (in_end <= STAGE_BYTES) pl.regime = 2;
    return pl;
}
HostPlan plan_cathode(size_t n) {
    const size_t chunk = n < (size_t(1) << 24) ? n : (size_t(1) << 24);
    const CathodeArrays a(nullptr, chunk);
    return finish_plan(n, chunk, a.in_end, a.end, a.end);
}
// the workspace (and with it the zero-copy decision) is sized for all eight outputs, whichever the caller asks for
HostPlan plan_thruster(size_t n, const bool (&wanted)[8]) {
    const size_t chunk = n < (size_t(1) << 24) ? n : (size_t(1) << 24);
    const bool all[8] = {true, true, true, true, true, true, true, true};
    const ThrusterArrays a(nullptr, chunk, wanted), full(nullptr, chunk, all);
    return finish_plan(n, chunk, a.in_end, a.end, full.end);
}
HostPlan plan_plume(size_t n, size_t R) {
    size_t chunk = (size_t(1) << 28) / (NANG * R * 8);   // bound the profile chunk to ~256 MiB of device memory
    if (chunk < 1024) chunk = 1024;
    if (chunk > n) chunk = n;
    chunk = (chunk + 63) & ~size_t(63);
    const PlumeArrays a(nullptr, chunk, R);
    return finish_plan(n, chunk, a.in_end, a.end, a.end);
}
HostPlan plan_coupled(size_t n) {
    size_t chunk = (size_t(1) << 28) / (NANG * 8);
    if (chunk > n) chunk = n;
    chunk = (chunk + 63) & ~size_t(63);
    const CoupledArrays a(nullptr, chunk);
    return finish_plan(n, chunk, a.in_end, a.end, a.end);
}

thread_local int t_last_regime = -1;   // pem_host_last_regime

struct Mover {
    unsigned char* ws;
    unsigned char* pin;       // staging for the inputs, or nullptr: array-by-array copies
    unsigned char* pin_out;   // staging for the outputs (needs the whole footprint to fit), or nullptr
    size_t in_lo = ~size_t(0), in_hi = 0, out_lo = ~size_t(0), out_hi = 0;
    struct Out {
        void* host;
        size_t off, bytes;
    } outs[8];
    int nout = 0;
    // where a host-pointer call carves its arrays: g_ws.mu held, g_ws reserved
    static unsigned char* base(const HostPlan& pl) {
        if (pl.regime == 0)
            if (unsigned char* p = g_stage.get()) return p;
        return static_cast<unsigned char*>(g_ws.buf);
    }
    // one chunk of the planned call; without the pinned buffer every regime falls back to array-by-array copies
    Mover(void* workspace, const HostPlan& pl)
        : ws(static_cast<unsigned char*>(workspace)),
          pin(pl.regime <= 2 ? g_stage.get() : nullptr),
          pin_out(pl.regime <= 1 ? pin : nullptr) {
        t_last_regime = pin ? pl.regime : 3;
    }
    int in(const void* host, void* dev, size_t bytes) {
        if (!pin) {
            HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, nullptr));
            return PEM_OK;
        }
        const size_t off = static_cast<unsigned char*>(dev) - ws;
        memcpy(pin + off, host, bytes);
        if (off < in_lo) in_lo = off;
        if (off + bytes > in_hi) in_hi = off + bytes;
        return PEM_OK;
    }
    int flush_in() {
        if (pin && pin != ws && in_hi > in_lo) HIP_TRY(hipMemcpyAsync(ws + in_lo, pin + in_lo, in_hi - in_lo, hipMemcpyHostToDevice, nullptr));
        return PEM_OK;
    }
    int out(void* host, const void* dev, size_t bytes) {
        if (!pin_out || nout == 8) {
            HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, nullptr));
            return PEM_OK;
        }
        const size_t off = static_cast<const unsigned char*>(dev) - ws;
        outs[nout++] = Out{host, off, bytes};
        if (off < out_lo) out_lo = off;
        if (off + bytes > out_hi) out_hi = off + bytes;
        return PEM_OK;
    }
    int finish() {
        if (pin_out && pin_out != ws && out_hi > out_lo)       // (ws == pin: the zero-copy form -- the kernels wrote there)
            HIP_TRY(hipMemcpyAsync(pin_out + out_lo, ws + out_lo, out_hi - out_lo, hipMemcpyDeviceToHost, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
        for (int i = 0; i < nout; ++i) memcpy(outs[i].host, pin_out + outs[i].off, outs[i].bytes);
        return PEM_OK;
    }
};

}  // namespace

extern "C" {

const char* pem_version(void) { return "hallthrusterpem_amd libpem_hip 0.1.0 (gfx950)"; }

int pem_device_count(void) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return cnt;
}

int pem_init(int device) {
    if (int rc = check_device()) return rc;
    HIP_TRY(hipSetDevice(device));
    g_device.store(device, std::memory_order_relaxed);
    return PEM_OK;
}

int pem_synchronize(pem_stream_t stream) {
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return PEM_OK;
}

int pem_host_plan(int entry, size_t n, int n_radii, int n_optional, size_t* chunk, size_t* n_chunks, size_t* in_end,
                  size_t* footprint, size_t* reserve, int* regime) {
    if (!chunk || !n_chunks || !in_end || !footprint || !reserve || !regime)
        return fail(PEM_ERR_INVALID_ARG, "pem_host_plan: NULL result pointer");
    if (n == 0 || n_radii < 1) return fail(PEM_ERR_INVALID_ARG, "pem_host_plan: n and n_radii must be positive");
    HostPlan pl;
    switch (entry) {
        case PEM_HOST_CATHODE: pl = plan_cathode(n); break;
        case PEM_HOST_THRUSTER: {
            if (n_optional < 0 || n_optional > 8) return fail(PEM_ERR_INVALID_ARG, "pem_host_plan: the thruster stage has 0 to 8 outputs");
            bool wanted[8];
            for (int i = 0; i < 8; ++i) wanted[i] = i < n_optional;   // the layout depends on their number only
            pl = plan_thruster(n, wanted);
            break;
        }
        case PEM_HOST_PLUME: pl = plan_plume(n, (size_t)n_radii); break;
        case PEM_HOST_COUPLED: pl = plan_coupled(n); break;
        default: return fail(PEM_ERR_INVALID_ARG, "pem_host_plan: unknown entry point %d", entry);
    }
    *chunk = pl.chunk;
    *n_chunks = pl.n_chunks;
    *in_end = pl.in_end;
    *footprint = pl.footprint;
    *reserve = pl.reserve;
    *regime = pl.regime;
    return PEM_OK;
}

int pem_host_last_regime(void) { return t_last_regime; }

// =============================================================================================
// host-pointer entry points: stage through the device workspace in chunks
// =============================================================================================
int pem_cathode_f64(size_t n, const double* P_b, const double* V_a, const double* T_e, const double* V_vac,
                    const double* Pstar, const double* P_T, double torr2pa, double* V_cc) {
    if (n == 0) return PEM_OK;
    if (!P_b || !V_a || !T_e || !V_vac || !Pstar || !P_T || !V_cc) return fail(PEM_ERR_INVALID_ARG, "pem_cathode: NULL array");
    if (int rc = check_device()) return rc;
    if (int rc = use_default_device()) return rc;
    std::lock_guard<std::mutex> lock(g_ws.mu);
    const HostPlan pl = plan_cathode(n);
    const size_t chunk = pl.chunk;
    if (int rc = g_ws.reserve(pl.reserve)) return rc;
    unsigned char* const base = Mover::base(pl);
    const double* in[6] = {P_b, V_a, T_e, V_vac, Pstar, P_T};
    const CathodeArrays a(base, chunk);
    double* const* d = a.d;
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = (n - off < chunk) ? n - off : chunk;
        Mover mv(base, pl);
        for (int i = 0; i < 6; ++i) PEM_TRY(mv.in(in[i] + off, d[i], m * 8));
        PEM_TRY(mv.flush_in());
        if (int rc = pem_cathode_f64_dev(m, d[0], d[1], d[2], d[3], d[4], d[5], torr2pa, d[6], nullptr)) return rc;
        PEM_TRY(mv.out(V_cc + off, d[6], m * 8));
        PEM_TRY(mv.finish());
    }
    return PEM_OK;
}

int pem_thruster_f64(size_t n, const double* V_a, const double* V_cc, const double* mdot_a, const double* a_1,
                     double* I_B0, double* I_d, double* T, double* eta_c, double* eta_m, double* eta_v, double* eta_a,
                     double* v_exh) {
    if (n == 0) return PEM_OK;
    if (!V_a || !V_cc || !mdot_a || !a_1) return fail(PEM_ERR_INVALID_ARG, "pem_thruster: NULL input array");
    if (int rc = check_device()) return rc;
    if (int rc = use_default_device()) return rc;
    std::lock_guard<std::mutex> lock(g_ws.mu);
    const double* in[4] = {V_a, V_cc, mdot_a, a_1};
    double* out[8] = {I_B0, I_d, T, eta_c, eta_m, eta_v, eta_a, v_exh};
    bool wanted[8];
    for (int i = 0; i < 8; ++i) wanted[i] = out[i] != nullptr;
    const HostPlan pl = plan_thruster(n, wanted);
    const size_t chunk = pl.chunk;
    if (int rc = g_ws.reserve(pl.reserve)) return rc;
    unsigned char* const base = Mover::base(pl);
    const ThrusterArrays a(base, chunk, wanted);
    double* const* di = a.in;
    double* const* dout = a.out;
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = (n - off < chunk) ? n - off : chunk;
        Mover mv(base, pl);
        for (int i = 0; i < 4; ++i) PEM_TRY(mv.in(in[i] + off, di[i], m * 8));
        PEM_TRY(mv.flush_in());
        if (int rc = pem_thruster_f64_dev(m, di[0], di[1], di[2], di[3], dout[0], dout[1], dout[2], dout[3], dout[4],
                                          dout[5], dout[6], dout[7], nullptr))
            return rc;
        for (int i = 0; i < 8; ++i)
            if (out[i]) PEM_TRY(mv.out(out[i] + off, dout[i], m * 8));
        PEM_TRY(mv.finish());
    }
    return PEM_OK;
}

int pem_plume_f64(size_t n, int n_radii, const double* radii, double torr2pa, const double* P_b, const double* c0,
                  const double* c1, const double* c2, const double* c3, const double* c4, const double* c5,
                  const double* sigma_cex, const double* I_B0, const double* T, double* j_ion, double* div_angle,
                  double* T_c, uint8_t* invalid) {
    if (n_radii < 1 || !radii) return fail(PEM_ERR_INVALID_ARG, "pem_plume: need at least one sweep radius");
    if (n == 0) return PEM_OK;
    if (!P_b || !c0 || !c1 || !c2 || !c3 || !c4 || !c5 || !sigma_cex || !I_B0 || !j_ion || !div_angle)
        return fail(PEM_ERR_INVALID_ARG, "pem_plume: NULL array");
    if ((T == nullptr) != (T_c == nullptr)) return fail(PEM_ERR_INVALID_ARG, "pem_plume: T and T_c go together");
    if (int rc = check_device()) return rc;
    if (int rc = use_default_device()) return rc;
    std::lock_guard<std::mutex> lock(g_ws.mu);
    const size_t R = (size_t)n_radii;
    const HostPlan pl = plan_plume(n, R);
    const size_t chunk = pl.chunk;
    if (int rc = g_ws.reserve(pl.reserve)) return rc;
    unsigned char* const base = Mover::base(pl);
    const double* in[10] = {P_b, c0, c1, c2, c3, c4, c5, sigma_cex, I_B0, T};
    const PlumeArrays a(base, chunk, R);
    double* const* d = a.d;
    double *const dj = a.j, *const ddiv = a.div, *const dtc = a.tc;
    uint8_t* const dinv = a.inv;
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = (n - off < chunk) ? n - off : chunk;
        Mover mv(base, pl);
        for (int i = 0; i < 10; ++i)
            if (in[i]) PEM_TRY(mv.in(in[i] + off, d[i], m * 8));
        PEM_TRY(mv.flush_in());
        if (int rc = pem_plume_f64_dev(m, n_radii, radii, torr2pa, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8],
                                       T ? d[9] : nullptr, dj, ddiv, T ? dtc : nullptr, invalid ? dinv : nullptr, nullptr))
            return rc;
        PEM_TRY(mv.out(j_ion + off * NANG * R, dj, m * NANG * R * 8));
        PEM_TRY(mv.out(div_angle + off * R, ddiv, m * R * 8));
        if (T) PEM_TRY(mv.out(T_c + off * R, dtc, m * R * 8));
        if (invalid) PEM_TRY(mv.out(invalid + off, dinv, m));
        PEM_TRY(mv.finish());
    }
    return PEM_OK;
}

int pem_coupled_f64(size_t n, double torr2pa, double radius, const double* P_b, const double* V_a, const double* T_e,
                    const double* V_vac, const double* Pstar, const double* P_T, const double* mdot_a, const double* a_1,
                    const double* c0, const double* c1, const double* c2, const double* c3, const double* c4,
                    const double* c5, const double* sigma_cex, double* V_cc, double* I_B0, double* T, double* j_ion,
                    double* div_angle, double* T_c, uint8_t* invalid) {
    if (n == 0) return PEM_OK;
    const double* in[15] = {P_b, V_a, T_e, V_vac, Pstar, P_T, mdot_a, a_1, c0, c1, c2, c3, c4, c5, sigma_cex};
    for (auto p : in)
        if (!p) return fail(PEM_ERR_INVALID_ARG, "pem_coupled: NULL input array");
    if (!V_cc || !div_angle || !T_c) return fail(PEM_ERR_INVALID_ARG, "pem_coupled: NULL output array");
    if (int rc = check_device()) return rc;
    if (int rc = use_default_device()) return rc;
    std::lock_guard<std::mutex> lock(g_ws.mu);
    const HostPlan pl = plan_coupled(n);
    const size_t chunk = pl.chunk;
    if (int rc = g_ws.reserve(pl.reserve)) return rc;
    unsigned char* const base = Mover::base(pl);
    const CoupledArrays a(base, chunk);
    double* const* d = a.d;
    double *const dvcc = a.vcc, *const dib0 = a.ib0, *const dT = a.T, *const ddiv = a.div, *const dtc = a.tc, *const dj = a.j;
    uint8_t* const dinv = a.inv;
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = (n - off < chunk) ? n - off : chunk;
        Mover mv(base, pl);
        for (int i = 0; i < 15; ++i) PEM_TRY(mv.in(in[i] + off, d[i], m * 8));
        PEM_TRY(mv.flush_in());
        if (int rc = pem_coupled_f64_dev(m, torr2pa, radius, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9],
                                         d[10], d[11], d[12], d[13], d[14], dvcc, I_B0 ? dib0 : nullptr, T ? dT : nullptr,
                                         j_ion ? dj : nullptr, ddiv, dtc, invalid ? dinv : nullptr, nullptr))
            return rc;
        PEM_TRY(mv.out(V_cc + off, dvcc, m * 8));
        if (I_B0) PEM_TRY(mv.out(I_B0 + off, dib0, m * 8));
        if (T) PEM_TRY(mv.out(T + off, dT, m * 8));
        if (j_ion) PEM_TRY(mv.out(j_ion + off * NANG, dj, m * NANG * 8));
        PEM_TRY(mv.out(div_angle + off, ddiv, m * 8));
        PEM_TRY(mv.out(T_c + off, dtc, m * 8));
        if (invalid) PEM_TRY(mv.out(invalid + off, dinv, m));
        PEM_TRY(mv.finish());
    }
    return PEM_OK;
}

}  // extern "C"
