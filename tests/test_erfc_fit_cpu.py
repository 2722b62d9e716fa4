"""The erfc evaluator of the composite walks (voge_amd/csrc/composite_core.h: h_pair) as the kernels evaluate it, on the CPU:
kQ0..kQ5 are read from the header, evaluated by the fp32 Horner emulation of tools/fit_erfc.py (a rounding after every
multiply-add) and held against scipy's erfc in fp64 -- inside the fitted range for the error, and over every 64th fp32 value
from the end of the range through +inf for what lets h_pair go without a range clamp: finite, falling, zero at +inf."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "voge_amd", "csrc", "composite_core.h")
sys.path.insert(0, os.path.join(ROOT, "tools"))

C = np.sqrt(np.log2(np.e))
XMAX = 5.0 * C
ERR_MAX = 6.5e-7      # 5.97e-7 measured for this fit against scipy (tools/fit_erfc.py), plus sampling margin
TAIL_MAX = 4e-13      # 3.6e-13 measured at the range's end


@pytest.fixture(scope="module")
def source():
    with open(HEADER) as f:
        return f.read()


@pytest.fixture(scope="module")
def coef(source):
    """kQ0..kQ5 as the header spells them (and no kQ6: the degree is part of the contract)."""
    got = {int(m.group(1)): float(m.group(2)) for m in re.finditer(r"\bkQ(\d)\s*=\s*([-+0-9.eE]+)f", source)}
    assert sorted(got) == [0, 1, 2, 3, 4, 5], sorted(got)
    return np.array([got[i] for i in range(6)], np.float64)


@pytest.fixture(scope="module")
def fit_erfc():
    import fit_erfc
    return fit_erfc


def test_error_inside_the_fitted_range(coef, fit_erfc):
    from scipy.special import erfc
    x = np.linspace(0.0, XMAX, 400001)
    h = fit_erfc.horner_fma32(coef, x).astype(np.float64)
    err = np.abs(h - erfc(x / C) / 2)                                               # the tool's own measure
    err32 = np.abs(h - erfc(x.astype(np.float32).astype(np.float64) / C) / 2)      # against erfc at the fp32 argument actually evaluated
    print(f"max |2^Q - erfc/2| on [0, 5 sqrt(log2 e)], 400001 points, fp32 Horner: {err.max():.3e} "
          f"(at the rounded argument: {err32.max():.3e}; bound {ERR_MAX:.1e})")
    assert err.max() <= ERR_MAX and err32.max() <= ERR_MAX, (err.max(), err32.max())


def test_h_of_zero(coef, fit_erfc):
    h0 = float(fit_erfc.horner_fma32(coef, np.zeros(1))[0])
    assert h0 == float(np.exp2(np.float32(coef[0])).astype(np.float32))      # exp2(kQ0): what the kernels use for the self term
    assert abs(h0 - 0.5) <= ERR_MAX, h0


def test_tail_needs_no_clamp(coef, fit_erfc):
    assert coef[-1] < 0.0      # the leading coefficient: Q falls past the range
    x = fit_erfc.tail_points(XMAX, 64)
    assert x[0] == np.float32(XMAX) and np.isposinf(x[-1]) and (np.diff(x.view(np.uint32).astype(np.int64)) > 0).all()
    v = fit_erfc.horner_fma32(coef, x).astype(np.float64)
    assert not np.isnan(v).any()
    assert np.isfinite(v).all()
    assert (np.diff(v) <= 0.0).all(), "2^Q turns up again past the range"
    print(f"max 2^Q past the range: {v.max():.3e} (bound {TAIL_MAX:.0e}); at +inf: {v[-1]}")
    assert v.max() <= TAIL_MAX, v.max()
    assert v[-1] == 0.0
    # the same through the tool's own report
    top, finite, mono, at_inf = fit_erfc.tail_report(coef, XMAX, 64)
    assert finite and mono and at_inf == 0.0 and top == v.max()


def test_refit_reproduces_the_header(coef, fit_erfc):
    """The header's numbers are the tool's degree-5 fit, not hand-edited."""
    again = fit_erfc.fit(5, XMAX)
    assert np.array_equal(np.float32(again), np.float32(coef)), (again, coef)


def test_h_pair_has_no_clamp(source):
    m = re.search(r"v2f h_pair\(.*?\)\s*\{(.*?)\n\}", source, flags=re.S)
    assert m, "h_pair not found"
    body = m.group(1)
    assert "fminf" not in body and "kXcap" not in source and "kQ6" not in source
    assert len(re.findall(r"\bpk_fma\(", body)) == 5 and len(re.findall(r"exp2f\(", body)) == 2
