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

// carve 256-byte aligned arrays out of the workspace
struct Carver {
    unsigned char* base;
    size_t off = 0;
    explicit Carver(void* b) : base(static_cast<unsigned char*>(b)) {}
    template <class T>
    T* take(size_t count) {
        T* p = reinterpret_cast<T*>(base + off);
        off += (count * sizeof(T) + 255) & ~size_t(255);
        return p;
    }
};
size_t padded(size_t bytes) { return (bytes + 255) & ~size_t(255); }

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
unsigned char* host_call_base(size_t footprint) {          // where a host-pointer call carves its arrays: g_ws.mu held, g_ws reserved
    static const bool on = !(getenv("PEM_ZERO_COPY") && atoi(getenv("PEM_ZERO_COPY")) == 0);
    if (on && footprint <= ZC_BYTES)
        if (unsigned char* pin = g_stage.get()) return pin;
    return static_cast<unsigned char*>(static_cast<void*>(g_ws.buf));
}

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
    // inputs are carved first: they end at `in_end`; the outputs end at `footprint`
    Mover(void* workspace, size_t in_end, size_t footprint)
        : ws(static_cast<unsigned char*>(workspace)),
          pin(in_end <= STAGE_BYTES ? g_stage.get() : nullptr),
          pin_out(footprint <= STAGE_BYTES ? pin : nullptr) {}
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
    const size_t chunk = n < (size_t(1) << 24) ? n : (size_t(1) << 24);
    if (int rc = g_ws.reserve(7 * padded(chunk * 8))) return rc;
    unsigned char* const base = host_call_base(7 * padded(chunk * 8));
    const double* in[6] = {P_b, V_a, T_e, V_vac, Pstar, P_T};
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = (n - off < chunk) ? n - off : chunk;
        Carver cv(base);
        double* d[7];
        for (int i = 0; i < 6; ++i) d[i] = cv.take<double>(chunk);
        const size_t in_end = cv.off;
        d[6] = cv.take<double>(chunk);
        Mover mv(base, in_end, cv.off);
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
    const size_t chunk = n < (size_t(1) << 24) ? n : (size_t(1) << 24);
    if (int rc = g_ws.reserve(12 * padded(chunk * 8))) return rc;
    unsigned char* const base = host_call_base(12 * padded(chunk * 8));
    const double* in[4] = {V_a, V_cc, mdot_a, a_1};
    double* out[8] = {I_B0, I_d, T, eta_c, eta_m, eta_v, eta_a, v_exh};
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = (n - off < chunk) ? n - off : chunk;
        Carver cv(base);
        double *di[4], *dout[8];
        for (auto& p : di) p = cv.take<double>(chunk);
        const size_t in_end = cv.off;
        for (int i = 0; i < 8; ++i) dout[i] = out[i] ? cv.take<double>(chunk) : nullptr;
        Mover mv(base, in_end, cv.off);
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
    // bound the profile chunk to ~256 MiB of device memory
    size_t chunk = (size_t(1) << 28) / (NANG * R * 8);
    if (chunk < 1024) chunk = 1024;
    if (chunk > n) chunk = n;
    chunk = (chunk + 63) & ~size_t(63);
    const size_t need = 10 * padded(chunk * 8) + padded(chunk * NANG * R * 8) + 2 * padded(chunk * R * 8) + padded(chunk);
    if (int rc = g_ws.reserve(need)) return rc;
    unsigned char* const base = host_call_base(need);
    const double* in[10] = {P_b, c0, c1, c2, c3, c4, c5, sigma_cex, I_B0, T};
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = (n - off < chunk) ? n - off : chunk;
        Carver cv(base);
        double* d[10];
        for (auto& p : d) p = cv.take<double>(chunk);
        const size_t in_end = cv.off;
        double* dj = cv.take<double>(chunk * NANG * R);
        double* ddiv = cv.take<double>(chunk * R);
        double* dtc = cv.take<double>(chunk * R);
        uint8_t* dinv = cv.take<uint8_t>(chunk);
        Mover mv(base, in_end, cv.off);
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
    size_t chunk = (size_t(1) << 28) / (NANG * 8);
    if (chunk > n) chunk = n;
    chunk = (chunk + 63) & ~size_t(63);
    const size_t need = 20 * padded(chunk * 8) + padded(chunk * NANG * 8) + padded(chunk);
    if (int rc = g_ws.reserve(need)) return rc;
    unsigned char* const base = host_call_base(need);
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = (n - off < chunk) ? n - off : chunk;
        Carver cv(base);
        double* d[15];
        for (auto& p : d) p = cv.take<double>(chunk);
        const size_t in_end = cv.off;
        double* dvcc = cv.take<double>(chunk);
        double* dib0 = cv.take<double>(chunk);
        double* dT = cv.take<double>(chunk);
        double* ddiv = cv.take<double>(chunk);
        double* dtc = cv.take<double>(chunk);
        uint8_t* dinv = cv.take<uint8_t>(chunk);
        double* dj = cv.take<double>(chunk * NANG);   // last: without a profile the staged copy-back stops before it
        Mover mv(base, in_end, cv.off);
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
