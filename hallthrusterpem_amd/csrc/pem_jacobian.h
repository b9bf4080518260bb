// pem_jacobian.h -- the coupled fp64 model with its exact first derivative, one lane per sample: the three reduced QoIs of
// Model64::eval (pem_saltelli_model.h) and d f_q / d x_i on the branch that evaluation takes.  Used by pem_jacobian.hip.
//
// The chain (reference lines at the stage functions of pem_model.h):
//   cathode    V = V_vac + T_e log(1 + PB / PT) - T_e PB / (PT + PS), PB = P_b k, PS = Pstar k, PT = P_T k
//                dV/dV_vac = 1                                       dV/dT_e = log(1 + PB / PT) - PB / (PT + PS)
//                dV/dP_b = k T_e (PS - PB) / ((PT + PB)(PT + PS))    dV/dPstar = k T_e PB / (PT + PS)^2
//                dV/dP_T = k T_e PB (1 / (PT + PS)^2 - 1 / (PT (PT + PB)))
//              V < 0: V_cc = 0 and the row is zero;  then V_cc > V_a: V_cc = V_a and the row is the unit vector of V_a
//   thruster   v = sqrt(2 q (V_a - V_cc) / m), T = mdot v:  dT/dy = (I_B0 / v) (dV_a/dy - dV_cc/dy), exactly 0 where the bracket is
//              exactly 0 (V_cc clamped to V_a: T = 0 on the whole branch);  dT/dmdot = v
//   plume      a1 = min(c2 PB + c3, pi/2): no derivative where clipped;  a2 = a1 / c1;  A1 = (1 - c0) / D(a1), A2 = c0 / D(a2)
//              cos_div = (A1 Qn(a1) + A2 Qn(a2)) / (A1 Qd(a1) + A2 Qd(a2)): the common factor `base` of both sums cancels, so
//              mdot_a, c4, c5 and sigma_cex have exactly zero entries in div_angle, and a_1 in every row
//              Q(a) = sum_k C_k e_k, e_k = exp(-(alpha_k / a)^2):   Q'(a) = (2 / a) sum_k C_k e_k (alpha_k / a)^2  -- the literal
//              91 terms (beam_sums), for `plain` samples and the others alike: the derivative of the literal sums
//              D(a) = 2 pi Int_0^{pi/2} exp(-(t / a)^2) sin t dt; integrating t^2 exp(-(t / a)^2) sin t by parts twice gives
//                  a D'(a) = D + (a^2 / 2)(2 pi - D) - pi^2 exp(-(pi / (2 a))^2)
//              so D' costs one exponential beside the tabulated D (no cancellation inside the priors: the three terms are
//              of one size only for |a| >> pi/2, where D' itself vanishes like a^-3)
//   div_angle = acos(cos_div): d = -dcos / sqrt((1 - cos)(1 + cos));    T_c = T cos_div: d = dT cos + T dcos
//
// The QoIs are Model64::eval's: the same stage functions, the tables for `plain` samples and literal_sums() for the others.
// Nothing here is contracted: every product and sum rounds on its own, in both kernels that inline this code.
#pragma once
#include "pem_saltelli_model.h"

namespace {

struct BeamSums {            // Qd, Qn and their derivatives with respect to the beam width
    double d, n, dd, dn;
};

__device__ __forceinline__ BeamSums beam_sums(const double2* simpson, double a) {
#pragma clang fp contract(off)
    using namespace pem_model;
    const double inv = 1.0 / a;
    BeamSums o{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int kk = 0; kk < NANG; ++kk) {
        const double alpha = kk == NANG - 1 ? HALF_PI : (double)kk * GRID_H;
        const double r = alpha * inv;
        const double t = r * r;
        const double e = exp_nonpos(-t);
        const double et = e == 0.0 ? 0.0 : e * t;
        const double2 c = simpson[kk];
        o.d = __builtin_fma(c.x, e, o.d);
        o.n = __builtin_fma(c.y, e, o.n);
        o.dd = __builtin_fma(c.x, et, o.dd);
        o.dn = __builtin_fma(c.y, et, o.dn);
    }
    o.dd *= 2.0 * inv;
    o.dn *= 2.0 * inv;
    return o;
}

// D'(a) / D(a) from the tabulated D
__device__ __forceinline__ double dlog_normaliser(double a, double D) {
#pragma clang fp contract(off)
    using namespace pem_model;
    const double r = HALF_PI / a;
    const double dD = (D + (0.5 * a * a) * (2.0 * PEM_PI - D) - (PEM_PI * PEM_PI) * exp_nonpos(-(r * r))) / a;
    return dD / D;
}

struct Jac {
    double f[NQ];            // V_cc, div_angle, T_c
    double dV[6];            // dV_cc / d(P_b, V_a, T_e, V_vac, Pstar, P_T)
    double dC[5];            // dcos_div / d(P_b, c0, c1, c2, c3)
    double tf, v, T, cos_div, dacos;
    bool bad_thruster, invalid;

    // d f_q / d x_i, q = 0..2, for one input, and x_i itself (`xi`: only for an input with an entry that is not structurally zero,
    // 1 otherwise); `i` is wave-uniform: the switch is a scalar branch, and no register array is indexed
    __device__ __forceinline__ void entries(int i, const double (&x)[NIN], double (&e)[NQ], double& xi) const {
#pragma clang fp contract(off)
        double dv = 0.0, dc = 0.0;
        bool cathode = false, plume = false;
        xi = 1.0;
        switch (i) {
            case 0: dv = dV[0]; dc = dC[0]; xi = x[0]; cathode = plume = true; break;
            case 1: dv = dV[1]; xi = x[1]; cathode = true; break;
            case 2: dv = dV[2]; xi = x[2]; cathode = true; break;
            case 3: dv = dV[3]; xi = x[3]; cathode = true; break;
            case 4: dv = dV[4]; xi = x[4]; cathode = true; break;
            case 5: dv = dV[5]; xi = x[5]; cathode = true; break;
            case 6: xi = x[6]; break;
            case 8: dc = dC[1]; xi = x[8]; plume = true; break;
            case 9: dc = dC[2]; xi = x[9]; plume = true; break;
            case 10: dc = dC[3]; xi = x[10]; plume = true; break;
            case 11: dc = dC[4]; xi = x[11]; plume = true; break;
            default: break;
        }
        double dT = 0.0;
        if (cathode) {
            const double dd = (i == 1 ? 1.0 : 0.0) - dv;
            dT = dd == 0.0 ? 0.0 : tf * dd;
        } else if (i == 6) {
            dT = v;
        }
        e[0] = dv;
        e[1] = plume ? dacos * dc : 0.0;
        e[2] = (cathode || i == 6) ? dT * cos_div : 0.0;
        if (plume) e[2] = e[2] + T * dc;
    }
};

__device__ __forceinline__ Jac jacobian(const Model64& m, const double (&x)[NIN]) {
#pragma clang fp contract(off)
    using namespace pem_model;
    Jac o;
    // ---- cathode: cathode_vcc's operations, then the derivative of the branch taken
    const double k = m.k;
    const double PB = x[0] * k, PS = x[4] * k, PT = x[5] * k;
    const double lg = log(1.0 + PB / PT);
    const double s = PT + PS;
    double V = x[3] + x[2] * lg;
    V = V - (x[2] / s) * PB;
    const double ts = k * x[2];
    o.dV[0] = ts * (PS - PB) / ((PT + PB) * s);
    o.dV[1] = 0.0;
    o.dV[2] = lg - PB / s;
    o.dV[3] = 1.0;
    o.dV[4] = ts * PB / (s * s);
    o.dV[5] = ts * PB * (1.0 / (s * s) - 1.0 / (PT * (PT + PB)));
    if (V < 0.0) {
        V = 0.0;
#pragma unroll
        for (int y = 0; y < 6; ++y) o.dV[y] = 0.0;
    }
    if (V > x[1]) {
        V = x[1];
#pragma unroll
        for (int y = 0; y < 6; ++y) o.dV[y] = y == 1 ? 1.0 : 0.0;
    }
    // ---- thruster
    const ThrusterQoI th = thruster_stage(x[1], V, x[6], x[7]);
    o.T = th.T;
    o.v = th.v_exh;
    o.tf = th.I_B0 / th.v_exh;
    // ---- plume: the lines of Model64::eval
    const PlumeSetup ps = plume_setup(x[0], x[9], x[10], x[11], x[12], x[13], k);
    const bool clipped = x[10] * PB + x[11] > HALF_PI;
    const double a1 = ps.a1, a2 = ps.a2;
    const double u1 = 1.0 / (a1 * a1), u2 = 1.0 / (a2 * a2);
    const double D1 = normaliser(a1, u1, m.dpoly), D2 = normaliser(a2, u2, m.dpoly);
    const double A1 = (1.0 - x[8]) / D1;
    const double A2 = x[8] / D2;
    const double decay = exp(-m.rad * ps.n_neutral * x[14]);
    const double j_cex = th.I_B0 * (1.0 - decay) * m.inv_2pi_r2;
    const double base = th.I_B0 * decay * m.inv_r2;
    const double X1a = base * A1, X2a = base * A2;
    const bool plain = fabs(a1) >= PEM_QA_MIN && fabs(a2) >= PEM_QA_MIN && X1a >= 0.0 && X2a >= 0.0 && j_cex > 0.0 &&
                       (fmax(X1a, X2a) >= 1e-280 || (X1a == 0.0 && X2a == 0.0));
    double d1, n1, d2, n2;
    simpson_functionals(m.qpoly, fabs(a1), u1, d1, n1);
    simpson_functionals(m.qpoly, fabs(a2), u2, d2, n2);
    double den = __builtin_fma(X1a, d1, X2a * d2), num = __builtin_fma(X1a, n1, X2a * n2);
    bool invalid = a1 <= 0.0;
    if (!plain) {
        const LiteralSums ls = literal_sums(m.simpson, X1a, X2a, j_cex, a1, a2);
        den = ls.den;
        num = ls.num;
        invalid = invalid || ls.lo <= 0.0;
    }
    double cos_div = num / den;
    if (cos_div == __builtin_inf()) cos_div = __builtin_nan("");
    o.cos_div = cos_div;
    o.f[0] = V;
    o.f[1] = acos(cos_div);
    o.f[2] = th.T * cos_div;
    o.bad_thruster = th.T < 0.0 || th.I_B0 < 0.0;
    o.invalid = invalid;
    // ---- d cos_div: the literal sums of each beam and their derivatives, one consistent set
    const BeamSums b1 = beam_sums(m.simpson, a1), b2 = beam_sums(m.simpson, a2);
    const double L1 = dlog_normaliser(a1, D1), L2 = dlog_normaliser(a2, D2);
    const double dsum = A1 * b1.d + A2 * b2.d;
    const double cs = (A1 * b1.n + A2 * b2.n) / dsum;
    const double G1 = A1 * ((b1.dn - b1.n * L1) - cs * (b1.dd - b1.d * L1)) / dsum;
    const double G2 = A2 * ((b2.dn - b2.n * L2) - cs * (b2.dd - b2.d * L2)) / dsum;
    const double H = clipped ? 0.0 : G1 + G2 / x[9];
    o.dC[0] = H * (x[10] * k);
    o.dC[1] = ((b2.n / D2 - b1.n / D1) - cs * (b2.d / D2 - b1.d / D1)) / dsum;
    o.dC[2] = -G2 * (a2 / x[9]);
    o.dC[3] = H * PB;
    o.dC[4] = H;
    o.dacos = -1.0 / sqrt((1.0 - cos_div) * (1.0 + cos_div));
    return o;
}

}  // namespace
