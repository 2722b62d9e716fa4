"""Coefficients of composite_core.h's h(x) = erfc(x)/2 = 2^Q(x'), x' = x*sqrt(log2 e), x in [0, 5].
Weighted (Lawson) minimax fit of log2(erfc/2) so that the ABSOLUTE error of 2^Q is minimised;
the fp32 Horner/fma evaluation is emulated to report the error the kernel actually sees.

For every degree the TAIL is reported too: what 2^Q does for x' past the fitted range, through +inf.  A fit whose
leading coefficient is negative keeps falling out there, so the kernel may evaluate it at any x' >= 0 without a
clamp; one whose leading coefficient is positive turns up again and diverges, and needs min(x', range)."""
import numpy as np
from numpy.polynomial import chebyshev as C
from scipy.special import erfc

c = np.sqrt(np.log2(np.e))


def fit(n, xmax, iters=40):
    xs = np.cos(np.linspace(0, np.pi, 6001)) * xmax / 2 + xmax / 2
    g = np.log2(erfc(xs / c) / 2)
    h = erfc(xs / c) / 2
    lw = np.ones_like(xs)
    for _ in range(iters):
        cc = C.chebfit(2 * xs / xmax - 1, g, n, w=h * lw)
        err = np.abs(C.chebval(2 * xs / xmax - 1, cc) - g) * h
        lw = lw * (err / err.max() + 1e-3)
        lw /= lw.mean()
    P = np.polynomial.Polynomial(C.cheb2poly(cc))(np.polynomial.Polynomial([-1, 2 / xmax]))
    return P.coef


def horner_fma32(coef, x):
    x = x.astype(np.float32).astype(np.float64)
    acc = np.full_like(x, np.float64(np.float32(coef[-1])))
    with np.errstate(over="ignore", invalid="ignore"):
        for cf in coef[-2::-1]:
            acc = (acc * x + np.float64(np.float32(cf))).astype(np.float32).astype(np.float64)
        return np.exp2(acc).astype(np.float32)


def tail_points(xmax, step=64):
    """Every `step`-th non-negative fp32 bit pattern from the end of the fitted range through +inf (inclusive)."""
    lo = int(np.float32(xmax).view(np.uint32))
    hi = int(np.float32(np.inf).view(np.uint32))
    bits = np.arange(lo, hi, step, dtype=np.uint32)
    return np.concatenate([bits, np.array([hi], np.uint32)]).view(np.float32)


def tail_report(coef, xmax, step=64):
    """(largest 2^Q past the range, all finite, non-increasing, value at +inf) in the fp32 emulation."""
    v = horner_fma32(coef, tail_points(xmax, step)).astype(np.float64)
    finite = bool(np.isfinite(v).all())
    mono = bool(finite and (np.diff(v) <= 0).all())
    return float(np.nanmax(v)), finite, mono, float(v[-1])


if __name__ == "__main__":
    xmax = 5.0 * c
    for n in (5, 6, 7, 8):
        coef = fit(n, xmax)
        x = np.linspace(0, xmax, 400001)
        e32 = np.abs(horner_fma32(coef, x).astype(np.float64) - erfc(x / c) / 2)
        print(n, "max abs err (fp32 eval) %.3e" % e32.max(), " h(0) =", horner_fma32(coef, np.zeros(1))[0])
        print("   ", ", ".join("%.9ef" % np.float32(v) for v in coef))
        top, finite, mono, at_inf = tail_report(coef, xmax)
        print("    leading coefficient %+.3e (%s);  past the range: max 2^Q = %.3e, finite: %s, non-increasing: %s, at +inf: %g"
              "  -> %s" % (coef[-1], "negative" if coef[-1] < 0 else "positive", top, finite, mono, at_inf,
                           "no clamp needed" if (coef[-1] < 0 and finite and mono and at_inf == 0.0) else "needs the clamp"))
