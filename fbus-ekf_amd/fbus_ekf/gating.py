"""Chi-square gate tables for BatchedFilter.set_gate (fbus_ekf_set_gate): thr[d] = the prob quantile of chi-square with d degrees
of freedom, thr[0] = inf.  Pure numpy/math (no scipy): the regularised lower incomplete gamma function P(a, x) by its series or
continued fraction (Numerical Recipes' gser / gcf split at x = a + 1), inverted by bracketing plus Newton steps."""
import math

import numpy as np

from .capi import GATE_MAX_DOF


def _gammp(a, x):
    """P(a, x), the regularised lower incomplete gamma function"""
    if x <= 0.0:
        return 0.0
    lg = a * math.log(x) - x - math.lgamma(a)
    if x < a + 1.0:                          # series: P = e^-x x^a / Gamma(a + 1) sum x^n / ((a+1)..(a+n))
        term = total = 1.0 / a
        ap = a
        for _ in range(100000):
            ap += 1.0
            term *= x / ap
            total += term
            if abs(term) < abs(total) * 1e-17:
                break
        return total * math.exp(lg)
    # continued fraction for Q = 1 - P (modified Lentz)
    tiny = 1e-300
    b = x + 1.0 - a
    c = 1.0 / tiny
    d = 1.0 / b
    h = d
    for i in range(1, 100000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-17:
            break
    return 1.0 - math.exp(lg) * h


def chi2_ppf(prob, d):
    """the prob quantile of chi-square with d > 0 degrees of freedom, to ~1e-12 relative"""
    if not 0.0 < prob < 1.0:
        raise ValueError("prob must be in (0, 1)")
    a = 0.5 * d
    # bracket [lo, hi] with P(a, lo / 2) <= prob <= P(a, hi / 2)
    lo, hi = 0.0, max(1.0, float(d))
    while _gammp(a, 0.5 * hi) < prob:
        lo, hi = hi, 2.0 * hi
    x = 0.5 * (lo + hi)
    for _ in range(200):
        f = _gammp(a, 0.5 * x) - prob
        if f > 0.0:
            hi = x
        else:
            lo = x
        # Newton on F(x) - prob with the chi-square density; a step that leaves the bracket is replaced by bisection
        logpdf = (a - 1.0) * math.log(0.5 * x) - 0.5 * x - math.lgamma(a) - math.log(2.0)
        pdf = math.exp(logpdf)
        xn = x - f / pdf if pdf > 0.0 else 0.5 * (lo + hi)
        if not lo < xn < hi:
            xn = 0.5 * (lo + hi)
        if abs(xn - x) <= 1e-14 * x or hi - lo <= 1e-14 * hi:
            return xn
        x = xn
    return x


def search_window(cov, prob=0.997):
    """the half-widths (..., 2) of the axis-aligned box around the prob ellipse of a predicted image point: cov (..., 3) =
    (S_uu, S_uv, S_vv) as BatchedFilter.project_markers returns it -> sqrt(chi2_ppf(prob, 2) (S_uu, S_vv)); 0 where the covariance
    is 0 (a projection that is not in view).  numpy array or torch tensor, returned in kind."""
    k = chi2_ppf(prob, 2)
    if hasattr(cov, "data_ptr"):
        import torch
        return torch.sqrt(k * cov[..., [0, 2]])
    return np.sqrt(k * np.asarray(cov, np.float64)[..., [0, 2]])


def chi2_gate(prob, max_dof=GATE_MAX_DOF):
    """the gate table of max_dof + 1 entries: thr[d] = chi2_ppf(prob, d), thr[0] = inf (a filter without rows is never rejected)"""
    thr = np.empty(int(max_dof) + 1, np.float64)
    thr[0] = np.inf
    for d in range(1, int(max_dof) + 1):
        thr[d] = chi2_ppf(prob, d)
    return thr
