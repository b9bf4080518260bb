// Worst errors, in double ulps, of csrc/pem_math.h as this ROCm compiles it for gfx950 -- pem_log10_tab, pem_log10_tab_pos, the
// series pem_log10 (with its v_rcp_f64 + Newton quotient, which no host restatement can reproduce) and pem_exp10 -- and of the
// library exp10 that the fused field path (csrc/pem_surrogate.hip) calls.  The device evaluates each function on an array of
// arguments; the host compares with log10l / powl of the same argument (64-bit significand: 2^-11 of a double ulp).
//   error [ulp] = |got - ref| / 2^(ilogb(ref) - 52), scored where ref is a normal double; results in the denormal range are scored
//   in units of 2^-1074 on a line of their own.
// Arguments: the named sets of tests/hp_math.py generated here by the same rules, plus 2^24 x 6 = 1.007e8 random ones per function:
//   log10  every table-interval edge 0.5 + i / 2048, i = 0 .. 1024, with both neighbours, scaled by 2^sh for the sh of LOG_SHIFTS
//          (denormal binades, 2^-1022, around 1, 2^1023); 5e-324, DBL_MIN, DBL_MAX, every 1e<k>; 1 + k 2^-53 (1 + (k & 1023)) for
//          k = -3e6 .. 3e6 in steps of 10; the worst arguments the host runs found; random: 1/4 uniform in [0.25, 4), 1/4 random bit
//          patterns (log-uniform over all positive doubles), 1/4 in [1, 1 + 2^-10) and 1/4 in [1 - 2^-11, 1) (table entries 0 and 1023)
//   exp10  every integer in [-330, 310]; k log10(2) and both neighbours for |k| <= 1100; (j + 1/2) / log2(10) and two neighbours
//          either side for every j with the value inside the clamps (the ties of rint); -330, 310 and their neighbours, +-1e6,
//          +-1e308; random: 5/6 uniform in [-330, 310], 1/6 uniform in [-1, 1]
// and the special values, which must come out as the source's selects say.
// tests/hp_math.py holds the figures rounded up (tests/test_log_table_host.py asserts the rounding against profiles/pem_math_r01.txt,
// which is this program's output).
// Build + run:  hipcc --offload-arch=gfx950 -O3 -Ihallthrusterpem_amd/csrc tools/microbench/pem_math_ulps.hip -o pmu -lpthread && ./pmu
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "pem_math.h"

enum { F_TAB, F_TABPOS, F_SERIES, F_EXP10, F_LIBEXP10, NFUNC };
static const char* NAMES[NFUNC] = {"pem_log10_tab", "pem_log10_tab_pos", "pem_log10", "pem_exp10", "exp10"};
constexpr int THREADS = 16;
constexpr size_t CHUNK = (size_t)1 << 24;
constexpr int RANDOM_CHUNKS = 6;
static const int LOG_SHIFTS[] = {-1060, -1040, -1022, -1021, -300, -1, 0, 1, 2, 300, 1023, 1024};

#define CHECK(call)                                                                      \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess) {                                                          \
            std::printf("%s failed: %s\n", #call, hipGetErrorString(e_));                \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

template <int F>
__global__ __launch_bounds__(256) void apply(const double* __restrict__ x, double* __restrict__ out, size_t n) {
    __shared__ __attribute__((aligned(16))) double logtab[pem::LOG_TABLE_DOUBLES];
    if (F == F_TAB || F == F_TABPOS) {
        pem::load_log_table(logtab, threadIdx.x, 256);
        __syncthreads();
    }
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const double a = x[i];
        double r = 0.0;
        if (F == F_TAB) r = pem::pem_log10_tab(a, logtab);
        if (F == F_TABPOS) r = pem::pem_log10_tab_pos(a, logtab);
        if (F == F_SERIES) r = pem::pem_log10(a);
        if (F == F_EXP10) r = pem::pem_exp10(a);
        if (F == F_LIBEXP10) r = exp10(a);
        out[i] = r;
    }
}

struct Worst {
    long double worst = 0, worst_den = 0;
    double at = 0, at_den = 0;
    size_t n = 0, n_den = 0, n_bad = 0;
    void merge(const Worst& o) {
        if (o.worst > worst) worst = o.worst, at = o.at;
        if (o.worst_den > worst_den) worst_den = o.worst_den, at_den = o.at_den;
        n += o.n, n_den += o.n_den, n_bad += o.n_bad;
    }
};

static void score(Worst& w, double x, double got, long double ref) {
    const long double aref = fabsl(ref);
    ++w.n;
    if (ref != ref || aref > 1.7976931348623157e308L || ref == 0) {
        w.n_bad += !((ref != ref && got != got) || got == (double)ref);
    } else if (aref < 2.2250738585072014e-308L) {
        const long double e = ldexpl(fabsl((long double)got - ref), 1074);
        ++w.n_den;
        if (e > w.worst_den) w.worst_den = e, w.at_den = x;
    } else {
        const long double e = fabsl((long double)got - ref) * ldexpl(1.0L, 52 - ilogbl(ref));
        if (e > w.worst) w.worst = e, w.at = x;
    }
}

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t bits64() {   // xorshift64*
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return g_state * 0x2545f4914f6cdd1dull;
}
static double uniform() { return (double)(bits64() >> 11) * 0x1p-53; }

static double *d_x, *d_out;
static Worst g_worst[NFUNC];
static size_t g_tabpos_differs = 0;

template <int F>
static int device(const std::vector<double>& x, std::vector<double>& got) {
    const size_t n = x.size();
    got.resize(n);
    CHECK(hipMemcpy(d_x, x.data(), n * 8, hipMemcpyHostToDevice));
    apply<F><<<4096, 256>>>(d_x, d_out, n);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(got.data(), d_out, n * 8, hipMemcpyDeviceToHost));
    return 0;
}

// one chunk of arguments (at most CHUNK) through every function of its family; the reference once per argument
static int run_chunk(bool logs, const std::vector<double>& x) {
    static std::vector<double> got[3];
    if (logs) {
        if (device<F_TAB>(x, got[0]) || device<F_TABPOS>(x, got[1]) || device<F_SERIES>(x, got[2])) return 1;
    } else {
        if (device<F_EXP10>(x, got[0]) || device<F_LIBEXP10>(x, got[1])) return 1;
    }
    const int nf = logs ? 3 : 2, f0 = logs ? F_TAB : F_EXP10;
    Worst part[THREADS][3];
    size_t differs[THREADS] = {};
    std::vector<std::thread> pool;
    for (int t = 0; t < THREADS; ++t)
        pool.emplace_back([&, t] {
            for (size_t i = t; i < x.size(); i += THREADS) {
                const long double ref = logs ? log10l((long double)x[i]) : powl(10.0L, (long double)x[i]);
                for (int f = 0; f < nf; ++f) score(part[t][f], x[i], got[f][i], ref);
                if (logs) differs[t] += std::memcmp(&got[0][i], &got[1][i], 8) != 0;
            }
        });
    for (auto& th : pool) th.join();
    for (int t = 0; t < THREADS; ++t) {
        for (int f = 0; f < nf; ++f) g_worst[f0 + f].merge(part[t][f]);
        g_tabpos_differs += differs[t];
    }
    return 0;
}

static void with_neighbours(std::vector<double>& v, double c, int m = 1) {
    double lo = c, hi = c;
    v.push_back(c);
    for (int k = 0; k < m; ++k) {
        lo = std::nextafter(lo, -INFINITY);
        hi = std::nextafter(hi, INFINITY);
        v.push_back(lo);
        v.push_back(hi);
    }
}

static std::vector<double> log10_set() {
    std::vector<double> raw, v;
    for (int sh : LOG_SHIFTS)
        for (int i = 0; i <= PEM_LOG_N; ++i) with_neighbours(raw, std::ldexp(0.5 + 0.5 * i / PEM_LOG_N, sh));
    for (double c : {5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 0x1.fffff6d0a7df6p-1, 0x1.ffdb2d6b9fc39p-1, 0x1.5366393480faap+0})
        raw.push_back(c);
    for (int k = -323; k <= 308; ++k) {
        char buf[16];
        std::snprintf(buf, sizeof buf, "1e%d", k);
        raw.push_back(std::strtod(buf, nullptr));
    }
    for (long k = -3000000; k <= 3000000; k += 10) raw.push_back(1.0 + (double)k * 0x1p-53 * (double)(1 + (k & 1023)));
    for (double c : raw)
        if (c > 0 && std::isfinite(c)) v.push_back(c);
    return v;
}

static std::vector<double> exp10_set() {
    std::vector<double> v;
    for (int k = -330; k <= 310; ++k) v.push_back((double)k);
    for (int k = -1100; k <= 1100; ++k) with_neighbours(v, (double)k * 0.30102999566398120);
    for (int j = -1097; j <= 1030; ++j) {
        const double y = ((double)j + 0.5) / 3.32192809488736234787;
        if (y > -330.0 && y < 310.0) with_neighbours(v, y, 2);
    }
    with_neighbours(v, -330.0);
    with_neighbours(v, 310.0);
    for (double c : {1e6, -1e6, 1e308, -1e308}) v.push_back(c);
    return v;
}

static void report(int f) {
    const Worst& w = g_worst[f];
    std::printf("%-18s %10zu arguments: normal results worst %.4Lf ulp at x = %a (%.17g)\n", NAMES[f], w.n, w.worst, w.at, w.at);
    if (w.n_den) std::printf("%-18s %10zu results below 2^-1022: worst %.4Lf units of 2^-1074 at x = %a (%.17g)\n", "", w.n_den, w.worst_den, w.at_den, w.at_den);
    std::printf("%-18s results 0, past DBL_MAX: %s\n", "", w.n_bad ? "MISMATCH" : "all as the long double function rounds");
}

static bool same(double a, double b) { return (a != a && b != b) || std::memcmp(&a, &b, 8) == 0; }

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    std::printf("pem_math_ulps: %s (%s), against log10l / powl on the host\n", prop.name, prop.gcnArchName);
    CHECK(hipMalloc(&d_x, CHUNK * 8));
    CHECK(hipMalloc(&d_out, CHUNK * 8));
    std::vector<double> x = log10_set();
    std::printf("log10 set: %zu arguments; then %d x %zu random ones\n", x.size(), RANDOM_CHUNKS, CHUNK);
    if (run_chunk(true, x)) return 1;
    for (int c = 0; c < RANDOM_CHUNKS; ++c) {
        x.clear();
        while (x.size() < CHUNK) {
            const uint64_t b = bits64() & 0x7fefffffffffffffull;
            double r;
            std::memcpy(&r, &b, 8);
            if (r > 0) x.push_back(r);
            x.push_back(0.25 + 3.75 * uniform());
            x.push_back(1.0 + 0x1p-10 * uniform());
            x.push_back(1.0 - 0x1p-11 * (1.0 - uniform()));
        }
        x.resize(CHUNK);
        if (run_chunk(true, x)) return 1;
    }
    for (int f : {F_TAB, F_TABPOS, F_SERIES}) report(f);
    std::printf("pem_log10_tab_pos against pem_log10_tab: %zu results differ in their bits\n", g_tabpos_differs);
    x = exp10_set();
    std::printf("exp10 set: %zu arguments; then %d x %zu random ones\n", x.size(), RANDOM_CHUNKS, CHUNK);
    if (run_chunk(false, x)) return 1;
    for (int c = 0; c < RANDOM_CHUNKS; ++c) {
        x.clear();
        for (size_t i = 0; i < CHUNK; ++i) x.push_back(i % 6 == 5 ? 2.0 * uniform() - 1.0 : -330.0 + 640.0 * uniform());
        if (run_chunk(false, x)) return 1;
    }
    for (int f : {F_EXP10, F_LIBEXP10}) report(f);
    // the special values: +-0 -> -inf, negative -> NaN, +inf -> +inf, NaN -> NaN; 10^NaN = NaN, 10^inf = inf, 10^-inf = 0, beyond the clamps 0 / inf
    const double inf = INFINITY, nan = NAN;
    const std::vector<double> ls = {0.0, -0.0, -5e-324, -1.0, -inf, inf, nan}, lw = {-inf, -inf, nan, nan, nan, inf, nan};
    const std::vector<double> es = {nan, inf, -inf, -330.0, -331.0, -1e308, 309.0, 310.0, 1e308}, ew = {nan, inf, 0.0, 0.0, 0.0, 0.0, inf, inf, inf};
    std::vector<double> got;
    size_t bad = 0;
    if (device<F_TAB>(ls, got)) return 1;
    for (size_t i = 0; i < ls.size(); ++i) bad += !same(got[i], lw[i]);
    if (device<F_SERIES>(ls, got)) return 1;
    for (size_t i = 0; i < ls.size(); ++i) bad += !same(got[i], lw[i]);
    if (device<F_EXP10>(es, got)) return 1;
    for (size_t i = 0; i < es.size(); ++i) bad += !same(got[i], ew[i]);
    std::printf("special values (+-0, negative, +-inf, NaN, beyond the clamps): %s\n", bad ? "MISMATCH" : "all as the source says");
    CHECK(hipFree(d_x));
    CHECK(hipFree(d_out));
    return bad || g_tabpos_differs ? 1 : 0;
}
