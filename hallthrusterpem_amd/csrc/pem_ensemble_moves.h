// pem_ensemble_moves.h -- the stretch and DE moves of the ensemble samplers, shared by pem_ensemble.hip (one ensemble per
// workgroup) and pem_tempering.hip (a ladder of tempered ensembles per workgroup): the Philox purposes, the draws of one moving
// walker and the proposed coordinate.  Every sum and product is rounded separately (no FMA), which the numpy restatements
// (tests/ensemble_np.py, tests/tempering_np.py) rely on.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pem_philox.h"

namespace pem {
namespace ens {

constexpr int DRAW_COLS = 6;   // move, z or g, j1, j2, u_acc, u_move

constexpr uint32_t PURPOSE_MOVE = 0x454E0000u;
constexpr uint32_t PURPOSE_PROPOSE = 0x454E0001u;
constexpr uint32_t PURPOSE_ACCEPT = 0x454E0002u;
constexpr uint32_t PURPOSE_SWAP = 0x454E0003u;   // replica exchange only (pem_tempering.hip)

// a standard normal from pem::u_open: never +-inf.  Out of line, a leaf: with the library normcdfinv body inlined into the
// propose loop the kernel is allocated 418 vector registers instead of 56.
static __device__ __attribute__((noinline)) double normal_of(uint32_t hi, uint32_t lo) { return normcdfinv(u_open(hi, lo)); }

// log(x) that a host restates bit for bit: the argument reduction and the degree-14 polynomial of the freely distributable fdlibm
// e_log.c (x = 2^k (1 + f), sqrt(2) / 2 < 1 + f < sqrt(2); s = f / (2 + f); log(1 + f) = f - (f^2 / 2 - s (f^2 / 2 + R(s^2)))),
// error below 1 ulp, written as IEEE sums, products and one division in a fixed order (tests/tempering_np.py: log_restated).  The
// library log is as accurate but its last bit is its own: it and numpy's disagree on one argument in fifty.  An x that is not
// positive, finite and normal goes to the library (a stretch variable z = t^2 / a is: 1 <= t <= a).
__device__ __forceinline__ double log_restatable(double x) {
#pragma clang fp contract(off)
    if (!(x >= 0x1.0p-1022 && x < INFINITY)) return log(x);
    const double ln2_hi = 0x1.62e42fee00000p-1, ln2_lo = 0x1.a39ef35793c76p-33;
    const double Lg1 = 0x1.5555555555593p-1, Lg2 = 0x1.999999997fa04p-2, Lg3 = 0x1.2492494229359p-2, Lg4 = 0x1.c71c51d8e78afp-3,
                 Lg5 = 0x1.7466496cb03dep-3, Lg6 = 0x1.39a09d078c69fp-3, Lg7 = 0x1.2f112df3e5244p-3;
    const uint64_t bits = (uint64_t)__double_as_longlong(x);
    int hx = (int)(bits >> 32);
    int k = (hx >> 20) - 1023;
    hx &= 0x000fffff;
    const int i = (hx + 0x95f64) & 0x100000;                  // 1 + f >= sqrt(2): halve it and count the factor in k
    k += i >> 20;
    const double m = __longlong_as_double((long long)(((uint64_t)(uint32_t)(hx | (i ^ 0x3ff00000)) << 32) | (bits & 0xffffffffull)));
    const double f = m - 1.0, dk = (double)k;
    if ((0x000fffff & (2 + hx)) < 3) {                        // |f| < 2^-20
        if (f == 0.0) return k == 0 ? 0.0 : dk * ln2_hi + dk * ln2_lo;
        const double R = f * f * (0.5 - 0.33333333333333333 * f);
        return k == 0 ? f - R : dk * ln2_hi - ((R - dk * ln2_lo) - f);
    }
    const double s = f / (2.0 + f), z = s * s, w = z * z;
    const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6)), t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
    const double R = t2 + t1;
    if (((hx - 0x6147a) | (0x6b851 - hx)) > 0) {
        const double hfsq = 0.5 * f * f;
        return k == 0 ? f - (hfsq - s * (hfsq + R)) : dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
    }
    return k == 0 ? f - s * (f - R) : dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f);
}

struct Move {
    double coef, log_q;   // z (stretch) or g (DE) of the moving walker, and the log of the proposal's weight
    int j1, j2;           // its partners in the complement; j2 = -1 for the stretch
};

// the draws of moving walker m of ensemble e at half-step s, for the move that u_move picked for the whole half; log q of the
// stretch through the library log, or with RESTATABLE through log_restatable
template <bool RESTATABLE = false>
__device__ __forceinline__ Move draw_move(uint32_t e, uint32_t s, uint32_t m, int H, int d, bool de, double a, double g0, double sigma,
                                          uint32_t k0, uint32_t k1) {
#pragma clang fp contract(off)
    const Philox4 r = philox4x32_10(e, s, PURPOSE_PROPOSE, m, k0, k1);
    Move mv;
    mv.j1 = (int)(((uint64_t)r.x * (uint64_t)H) >> 32);
    mv.j2 = -1;
    if (de) {
        mv.j2 = (int)(((uint64_t)r.y * (uint64_t)(H - 1)) >> 32);
        if (mv.j2 >= mv.j1) mv.j2 += 1;
        mv.coef = g0 * (1.0 + sigma * normal_of(r.z, r.w));
        mv.log_q = 0.0;
    } else {
        const double t = (a - 1.0) * u53(r.z, r.w) + 1.0;
        mv.coef = t * t / a;
        mv.log_q = (double)(d - 1) * (RESTATABLE ? log_restatable(mv.coef) : log(mv.coef));
    }
    return mv;
}

__device__ __forceinline__ double stretch_point(double c, double xw, double x1) {
#pragma clang fp contract(off)
    return x1 + c * (xw - x1);
}

__device__ __forceinline__ double de_point(double c, double xw, double x1, double x2) {
#pragma clang fp contract(off)
    return xw + c * (x1 - x2);
}

}  // namespace ens
}  // namespace pem
