// Worst errors, in double ulps, of the fp64 functions the model kernels (csrc/pem_model.h, pem_kernels.hip, pem_radii.hip,
// pem_latent.hip, pem_stages.hip) are built from, as this ROCm compiles them for gfx950: exp, log, sqrt, the division, acos, log10 and
// the project's own exp_nonpos.  The device evaluates each function on an array of arguments; the host compares with the long
// double function of the same argument (64-bit significand: 2^-11 of a double ulp).  Arguments: random ones over the ranges the
// model uses (below) plus every binade edge of the range with its two neighbours.
//   error [ulp] = |got - ref| / 2^(ilogb(ref) - 52), scored where ref is a normal double; results in the denormal range are scored
//   in units of 2^-1074 on a line of their own.
//   exp        x in [-745.2, 88] uniform, +-10^[-12, 0] log-uniform, +-2^e           (decay = exp(-r n sigma), the literal Gaussians)
//   exp_nonpos x in [-708, 0] the same way                                           (the recurrences' seeds)
//   log        x = 1 + 10^[-16, 9] log-uniform, 2^e                                   (log(1 + PB / PT))
//   sqrt       x = 10^[-300, 300]                                                     (v_exh)
//   div        a / b, both 10^[-150, 150] with random significands
//   acos       x in [-1, 1] uniform, +-(1 - 2^-e), +-2^-e                             (div_angle)
//   log10      x = 10^[-300, 300]                                                     (norm log10 of the compression map)
// tests/hp_model.py holds the figures, rounded up to the next half ulp; profiles/f64_intrinsics_r01.txt is this program's output.
// Build + run:  hipcc --offload-arch=gfx950 -O3 -Iinclude -Ihallthrusterpem_amd/csrc tools/microbench/f64_intrinsics.hip -o f64i && ./f64i
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pem_model.h"

enum { F_EXP, F_EXPNP, F_LOG, F_SQRT, F_DIV, F_ACOS, F_LOG10, NFUNC };

#define CHECK(call)                                                                      \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess) {                                                          \
            std::printf("%s failed: %s\n", #call, hipGetErrorString(e_));                \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

template <int F>
__global__ __launch_bounds__(256) void apply(const double* __restrict__ x, const double* __restrict__ y, double* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double a = x[i];
    double r = 0.0;
    if (F == F_EXP) r = exp(a);
    if (F == F_EXPNP) r = pem_model::exp_nonpos(a);
    if (F == F_LOG) r = log(a);
    if (F == F_SQRT) r = sqrt(a);
    if (F == F_DIV) r = a / y[i];
    if (F == F_ACOS) r = acos(a);
    if (F == F_LOG10) r = log10(a);
    out[i] = r;
}

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static double uniform() {   // xorshift64*, 53 bits
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return (double)((g_state * 0x2545f4914f6cdd1dull) >> 11) * 0x1p-53;
}
static double log_uniform(double lo_exp10, double hi_exp10) { return std::pow(10.0, lo_exp10 + (hi_exp10 - lo_exp10) * uniform()) * (1.0 + uniform()) / 1.5; }
static void edges(std::vector<double>& v, int e0, int e1, double sign, double lo, double hi) {
    for (int e = e0; e <= e1; ++e) {
        const double b = sign * std::ldexp(1.0, e);
        for (double c : {std::nextafter(b, -INFINITY), b, std::nextafter(b, INFINITY)})
            if (c >= lo && c <= hi) v.push_back(c);
    }
}

static long double reference(int f, double a, double b) {
    switch (f) {
        case F_EXP: case F_EXPNP: return expl((long double)a);
        case F_LOG: return logl((long double)a);
        case F_SQRT: return sqrtl((long double)a);
        case F_DIV: return (long double)a / (long double)b;
        case F_ACOS: return acosl((long double)a);
        default: return log10l((long double)a);
    }
}

template <int F>
int run(const char* name, const std::vector<double>& x, const std::vector<double>& y) {
    const size_t n = x.size();
    double *dx, *dy, *dout;
    CHECK(hipMalloc(&dx, n * 8));
    CHECK(hipMalloc(&dy, n * 8));
    CHECK(hipMalloc(&dout, n * 8));
    CHECK(hipMemcpy(dx, x.data(), n * 8, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dy, y.empty() ? x.data() : y.data(), n * 8, hipMemcpyHostToDevice));
    apply<F><<<(unsigned)((n + 255) / 256), 256>>>(dx, dy, dout, n);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<double> got(n);
    CHECK(hipMemcpy(got.data(), dout, n * 8, hipMemcpyDeviceToHost));
    CHECK(hipFree(dx));
    CHECK(hipFree(dy));
    CHECK(hipFree(dout));
    long double worst = 0, worst_den = 0;
    size_t at = 0, at_den = 0, n_den = 0, n_bad = 0;
    for (size_t i = 0; i < n; ++i) {
        const long double ref = reference(F, x[i], y.empty() ? 0.0 : y[i]);
        const long double aref = fabsl(ref);
        if (ref != ref || aref > 1.7976931348623157e308L) {
            n_bad += !((ref != ref && got[i] != got[i]) || got[i] == (double)ref);
        } else if (aref < 2.2250738585072014e-308L) {
            const long double e = ldexpl(fabsl((long double)got[i] - ref), 1074);
            ++n_den;
            if (e > worst_den) worst_den = e, at_den = i;
        } else {
            const long double e = fabsl((long double)got[i] - ref) * ldexpl(1.0L, 52 - ilogbl(ref));
            if (e > worst) worst = e, at = i;
        }
    }
    std::printf("%-12s %9zu arguments: normal results worst %.4Lf ulp at x = %.17g", name, n, worst, x[at]);
    if (F == F_DIV) std::printf(" / %.17g", y[at]);
    std::printf("\n");
    if (n_den) std::printf("             %9zu results below 2^-1022: worst %.2Lf units of 2^-1074 at x = %.17g\n", n_den, worst_den, x[at_den]);
    std::printf("             results past DBL_MAX / NaN: %s\n", n_bad ? "MISMATCH" : "all as the long double function rounds");
    return 0;
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    std::printf("f64_intrinsics: %s (%s), against the long double functions on the host\n", prop.name, prop.gcnArchName);
    const size_t N = 1u << 20;
    std::vector<double> x, y;
    int rc = 0;
    for (size_t i = 0; i < N; ++i) x.push_back(-745.2 + 833.2 * uniform());
    for (size_t i = 0; i < N / 4; ++i) x.push_back((uniform() < 0.5 ? -1.0 : 1.0) * log_uniform(-12, 0));
    edges(x, -40, 9, -1.0, -745.2, 88.0);
    edges(x, -40, 6, 1.0, -745.2, 88.0);
    rc |= run<F_EXP>("exp", x, y);
    x.clear();
    for (size_t i = 0; i < N; ++i) x.push_back(-708.0 * uniform());
    for (size_t i = 0; i < N / 4; ++i) x.push_back(-log_uniform(-12, 0));
    edges(x, -40, 9, -1.0, -708.0, 0.0);
    rc |= run<F_EXPNP>("exp_nonpos", x, y);
    x.clear();
    for (size_t i = 0; i < N; ++i) x.push_back(1.0 + log_uniform(-16, 9));
    edges(x, 0, 30, 1.0, 1.0, 2e9);
    rc |= run<F_LOG>("log", x, y);
    x.clear();
    for (size_t i = 0; i < N; ++i) x.push_back(log_uniform(-300, 300));
    edges(x, -1000, 1000, 1.0, 1e-300, 1e300);
    rc |= run<F_SQRT>("sqrt", x, y);
    rc |= run<F_LOG10>("log10", x, y);
    x.clear();
    for (size_t i = 0; i < N; ++i) {
        x.push_back((uniform() < 0.5 ? -1.0 : 1.0) * log_uniform(-150, 150));
        y.push_back(log_uniform(-150, 150));
    }
    rc |= run<F_DIV>("div", x, y);
    x.clear();
    y.clear();
    for (size_t i = 0; i < N; ++i) x.push_back(2.0 * uniform() - 1.0);
    for (int e = 1; e <= 53; ++e)
        for (double s : {-1.0, 1.0}) {
            x.push_back(s * (1.0 - std::ldexp(1.0, -e)));
            x.push_back(s * std::ldexp(1.0, -e));
        }
    x.push_back(1.0);
    x.push_back(-1.0);
    x.push_back(0.0);
    rc |= run<F_ACOS>("acos", x, y);
    return rc;
}
