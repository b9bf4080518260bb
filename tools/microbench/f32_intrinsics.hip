// Worst errors, in float ulps, of the single-precision functions the fp32 model (csrc/pem_model_f32.h) is built from, as this
// ROCm compiles them for gfx950: __builtin_amdgcn_rcpf (v_rcp_f32), __builtin_amdgcn_sqrtf (v_sqrt_f32), __expf, __logf (v_exp_f32 /
// v_log_f32 and the scaling multiply around them) and acosf.  Each function is swept over EVERY finite float of its domain -- all
// positive finite floats (both signs for __expf; [-1, 1] for acosf) -- and compared on the device with the fp64 function of the
// widened argument, which is 2^-29 finer than a float ulp.  One launch per function, a max-reduction per bin.
//   error [ulp] = |got - ref| / 2^(ilogb(ref) - 23), scored where ref is a normal float; where |ref| < 2^-126 the error is scored
//   in units of 2^-149 (the denormal spacing; a flush to zero shows as up to 2^23 of them) and where ref overflows got must be inf.
//   v_rcp_f32 and v_sqrt_f32 read a denormal argument as zero: those arguments are listed on a line of their own.
// __expf's error grows with |x| (the product x * log2(e) is rounded before v_exp_f32 sees it), so it is reported per binade of |x|.
// tests/hp_fp32.py holds the figures, rounded up to the next half ulp; profiles/fp32_intrinsics_r01.txt is this program's output.
// Build + run on the GPU box:  hipcc --offload-arch=gfx950 -O3 tools/microbench/f32_intrinsics.hip -o /tmp/f32i && /tmp/f32i
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

enum { F_RCP, F_SQRT, F_EXP, F_EXP_NEG, F_LOG, F_ACOS, F_ACOS_NEG, NFUNC };
constexpr int NBIN = 16;          // 0..9: normal results per binade of |x| (F_EXP*) or bin 0; 13: denormal arguments of the raw
                                  // instructions (they flush); 14: wrong special value; 15: results in the denormal range

#define CHECK(call)                                                                      \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess) {                                                          \
            std::printf("%s failed: %s\n", #call, hipGetErrorString(e_));                \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

template <int F>
__device__ __forceinline__ void eval(float x, float& got, double& ref) {
    const double xd = (double)x;
    if (F == F_RCP) { got = __builtin_amdgcn_rcpf(x); ref = 1.0 / xd; }
    if (F == F_SQRT) { got = __builtin_amdgcn_sqrtf(x); ref = sqrt(xd); }
    if (F == F_EXP || F == F_EXP_NEG) { got = __expf(x); ref = exp(xd); }
    if (F == F_LOG) { got = __logf(x); ref = log(xd); }
    if (F == F_ACOS || F == F_ACOS_NEG) { got = acosf(x); ref = acos(xd); }
}

// bits first .. last (inclusive) are the positive floats swept; NEG sweeps their negatives
template <int F>
__global__ __launch_bounds__(256) void sweep(uint32_t first, uint32_t last, unsigned long long* worst /* [NBIN] double bits */,
                                             uint32_t* worst_arg /* [NBIN] */, int pass) {
    __shared__ unsigned long long lmax[NBIN];
    if (threadIdx.x < NBIN) lmax[threadIdx.x] = pass == 0 ? 0ull : worst[threadIdx.x];
    __syncthreads();
    constexpr bool NEG = F == F_EXP_NEG || F == F_ACOS_NEG;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256;
    for (unsigned long long b = (unsigned long long)first + blockIdx.x * 256ull + threadIdx.x; b <= last; b += stride) {
        const uint32_t bits = (uint32_t)b | (NEG ? 0x80000000u : 0u);
        const float x = __uint_as_float(bits);
        float got;
        double ref;
        eval<F>(x, got, ref);
        int bin = 0;
        double err;
        const double aref = fabs(ref);
        if ((F == F_RCP || F == F_SQRT) && (bits & 0x7fffffffu) < 0x00800000u) {   // v_rcp_f32 / v_sqrt_f32 read a denormal as zero
            bin = 13;
            err = fabs((double)got - ref) * ldexp(1.0, 23 - ilogb(ref));
        } else if (aref > 3.4028234663852886e38 || ref != ref) {               // past FLT_MAX (rounds to inf from 3.40282357e38 on: within an ulp)
            bin = 14;
            err = (aref < 3.4028235677973366e38 || got == (float)ref || (ref != ref && got != got)) ? 0.0 : 1.0;
        } else if (aref < 1.1754943508222875e-38) {                     // denormal range (and ref == 0)
            bin = 15;
            err = fabs((double)got - ref) * 0x1p149;
        } else {
            err = fabs((double)got - ref) * ldexp(1.0, 23 - ilogb(ref));
            if (F == F_EXP || F == F_EXP_NEG) {
                const int e = ilogb((double)fabsf(x)) + 1;              // |x| < 1: 0, [1, 2): 1, [2, 4): 2 ... [64, 128): 7
                bin = e < 0 ? 0 : (e > 9 ? 9 : e);
            }
        }
        const unsigned long long eb = (unsigned long long)__double_as_longlong(err);        // err >= 0: ordered as integers
        if (pass == 0) {
            if (eb > lmax[bin]) atomicMax(&lmax[bin], eb);
        } else if (eb == lmax[bin] && eb != 0ull) {
            worst_arg[bin] = bits;                                      // any one argument that attains the maximum
        }
    }
    __syncthreads();
    if (pass == 0 && threadIdx.x < NBIN) atomicMax(&worst[threadIdx.x], lmax[threadIdx.x]);
}

static float x0(uint32_t bits) {
    float x;
    std::memcpy(&x, &bits, 4);
    return x;
}

template <int F>
int run(const char* name, uint32_t first, uint32_t last, unsigned long long* d_worst, uint32_t* d_arg) {
    CHECK(hipMemset(d_worst, 0, NBIN * sizeof(unsigned long long)));
    CHECK(hipMemset(d_arg, 0, NBIN * sizeof(uint32_t)));
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    CHECK(hipEventRecord(a));
    sweep<F><<<2048, 256>>>(first, last, d_worst, d_arg, 0);
    CHECK(hipEventRecord(b));
    sweep<F><<<2048, 256>>>(first, last, d_worst, d_arg, 1);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    float ms = 0.0f;
    CHECK(hipEventElapsedTime(&ms, a, b));
    unsigned long long w[NBIN];
    uint32_t arg[NBIN];
    CHECK(hipMemcpy(w, d_worst, sizeof(w), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(arg, d_arg, sizeof(arg), hipMemcpyDeviceToHost));
    std::printf("%-28s %10llu arguments, bits 0x%08x .. 0x%08x%s, %.1f ms\n", name, (unsigned long long)last - first + 1, first, last,
                (F == F_EXP_NEG || F == F_ACOS_NEG) ? " negated" : "", ms);
    for (int i = 0; i < NBIN; ++i) {
        double e;
        std::memcpy(&e, &w[i], 8);
        if (w[i] == 0ull && !(i == 0 || i >= 14)) continue;
        if (i == 13) {
            std::printf("    denormal arguments (not scored above): worst %.4g ulp at x = %.9g (0x%08x)\n", e, x0(arg[i]), arg[i]);
            continue;
        }
        float x;
        std::memcpy(&x, &arg[i], 4);
        if (i < 14) {
            if (F == F_EXP || F == F_EXP_NEG)
                std::printf("    |x| %s: worst %.4f ulp at x = %.9g (0x%08x)\n",
                            i == 0 ? "< 1       " : (i == 1 ? "in [1, 2) " : (i == 2 ? "in [2, 4) " : (i == 3 ? "in [4, 8) " : (i == 4 ? "in [8, 16)" :
                            (i == 5 ? "in [16,32)" : (i == 6 ? "in [32,64)" : "in [64, ..)")))))), e, x, arg[i]);
            else
                std::printf("    normal results: worst %.4f ulp at x = %.9g (0x%08x)\n", e, x, arg[i]);
        } else if (i == 14) {
            std::printf("    results past FLT_MAX / NaN: %s\n", e == 0.0 ? "all as the fp64 function rounds" : "MISMATCH");
        } else {
            std::printf("    results below 2^-126: worst %.1f units of 2^-149 at x = %.9g (0x%08x)\n", e, x, arg[i]);
        }
    }
    return 0;
}

int main() {
    unsigned long long* d_worst;
    uint32_t* d_arg;
    CHECK(hipMalloc(&d_worst, NBIN * sizeof(unsigned long long)));
    CHECK(hipMalloc(&d_arg, NBIN * sizeof(uint32_t)));
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    std::printf("f32_intrinsics: %s (%s), exhaustive sweeps against the fp64 functions on the device\n", prop.name, prop.gcnArchName);
    const uint32_t one = 0x3f800000u, fmax = 0x7f7fffffu;
    int rc = 0;
    rc |= run<F_RCP>("rcp  (v_rcp_f32)", 1u, fmax, d_worst, d_arg);
    rc |= run<F_SQRT>("sqrt (v_sqrt_f32)", 1u, fmax, d_worst, d_arg);
    rc |= run<F_EXP>("__expf(+x)", 1u, fmax, d_worst, d_arg);
    rc |= run<F_EXP_NEG>("__expf(-x)", 1u, fmax, d_worst, d_arg);
    rc |= run<F_LOG>("__logf", 1u, fmax, d_worst, d_arg);
    rc |= run<F_ACOS>("acosf(+x), x <= 1", 0u, one, d_worst, d_arg);
    rc |= run<F_ACOS_NEG>("acosf(-x), x <= 1", 0u, one, d_worst, d_arg);
    CHECK(hipFree(d_worst));
    CHECK(hipFree(d_arg));
    return rc;
}
