"""High-precision references for csrc/pem_sampler.hip.  TEST INFRASTRUCTURE.

The Saltelli partial sums (pem_sobol_partial_f64_dev) in np.longdouble with a bound of the form 1.01 C u S (tests/hp_reference.py:
u = 2^-53, S the same sum over absolute terms, C the roundings a term can pass through), and the normal quantile at 40 digits
(mpmath) for the tails of the design's normal dimensions."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SOBOL_BLOCK = 256      # threads of a workgroup of sobol_partial_kernel
assert np.finfo(LD).nmant >= 63, 'the reference needs an 80-bit long double'


def sobol_roundings(m, n_blocks, with_ab):
    """C of the two sums (index 0, 1) of sobol_partial_kernel, derived from the kernel.

    A thread adds one term per pass of its grid-stride loop, L = ceil(m / (n_blocks * 256)) passes; the wave's 64 values are
    then added in 6 shuffle steps and the workgroup's 4 wave values in a loop of 4 adds (`t = 0.0; t += red[w]`), each add one
    rounding of the running sum: L + 6 + 4.  The caller's sum over workgroups is taken in long double here and costs nothing.
    Forming the term adds, per mode and sum:
      fAB == NULL, sum 0   `s0 += a + b`: a + b is rounded once before it enters the chain                              -> 1
      fAB == NULL, sum 1   `s1 = fma(a, a, fma(b, b, s1))`: the products are exact inside the fma, but a pass is two chain
                           steps instead of one, so a term can pass through L more roundings                          -> L
      fAB given,   sum 0   `fma(b, ab - a, s0)`: ab - a is rounded once, the product is exact inside the fma           -> 1
      fAB given,   sum 1   `fma(a - ab, a - ab, s1)`: the rounded difference enters squared, (1 + d)^2                 -> 2
    (the second-order terms are covered by the factor 1.01, as in hp_reference.py)."""
    chain = -(-m // (n_blocks * SOBOL_BLOCK))
    common = chain + 6 + 4
    return (common + 1, common + 2) if with_ab else (common + 1, common + chain)


def sobol_partial_ref(fA, fB, fAB, n_blocks):
    """(sums [nq][2], bound [nq][2]) of the kernel's partials summed over workgroups; fA, fB, fAB [nq][m] float64, fAB or None."""
    a, b = np.asarray(fA, dtype=np.float64).astype(LD), np.asarray(fB, dtype=np.float64).astype(LD)
    if fAB is None:
        t0, t1 = a + b, a * a + b * b
        s0, s1 = np.abs(a) + np.abs(b), t1
    else:
        ab = np.asarray(fAB, dtype=np.float64).astype(LD)
        t0, t1 = b * (ab - a), (a - ab) * (a - ab)
        s0, s1 = np.abs(b) * np.abs(ab - a), t1
    c0, c1 = sobol_roundings(a.shape[1], n_blocks, fAB is not None)
    want = np.stack([t0.sum(axis=1), t1.sum(axis=1)], axis=1)
    bound = np.stack([1.01 * c0 * U * s0.sum(axis=1), 1.01 * c1 * U * s1.sum(axis=1)], axis=1)
    return want, bound


def ndtri_mp(u, digits=40):
    """the standard normal quantile of every double in u, correct to well beyond a long double (mpmath at `digits` digits:
    Newton's iteration on the normal cdf from scipy's double, until the step is below 10^-(digits - 5))"""
    import mpmath
    from scipy.special import ndtri
    out = np.empty(len(u), dtype=LD)
    with mpmath.workdps(digits):
        tol = mpmath.mpf(10) ** -(digits - 5)
        for i, ui in enumerate(np.asarray(u, dtype=np.float64)):
            p, z = mpmath.mpf(float(ui)), mpmath.mpf(float(ndtri(ui)))
            for _ in range(8):
                step = (mpmath.ncdf(z) - p) / mpmath.npdf(z)
                z -= step
                if abs(step) < tol:
                    break
            else:
                raise AssertionError(f'no convergence at u = {ui!r}')
            out[i] = LD(mpmath.nstr(z, 25))
    return out
