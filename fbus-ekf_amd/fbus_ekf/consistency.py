"""Consistency of a bank of filters against a known state: what to hold BatchedFilter.nees() against (pure numpy / math).

Under a consistent filter -- truth ~ N(estimate, P) -- a column of nees is chi-square with the block's degrees of freedom, and the
average over n independent filters times n is chi-square with n dof: the ANEES test of Bar-Shalom, Li and Kirubarajan, Estimation
with Applications to Tracking and Navigation, section 5.4.  A mean above the interval says P is too small (over-confident), one
below it that P is too large.

The way back -- states DRAWN from N(estimate, P) on the device, BatchedFilter.sample() -- takes its coordinates from here: sigma_points()
and draw().
"""
import numpy as np

from .capi import NEES_COLS, SAMPLE_MAX
from .gating import chi2_ppf

NEES_NAMES = ("full", "pose", "p", "v", "theta", "ba", "bg", "g")      # the columns of fbus_ekf_nees, in order
assert len(NEES_NAMES) == NEES_COLS


def nees_dof(nstate):
    """the degrees of freedom of the 8 columns (g: 0 for nstate 15, where the column is written as 0)"""
    if nstate not in (15, 18):
        raise ValueError("nstate must be 15 or 18")
    return (nstate, 6, 3, 3, 3, 3, 3, 3 if nstate == 18 else 0)


def anees_interval(dof, n, prob=0.95):
    """the two-sided chi-square interval (lo, hi) that holds the average of n independent NEES values of `dof` degrees of freedom
    with probability prob: chi2_ppf((1 -+ prob) / 2, n dof) / n"""
    if dof <= 0 or n <= 0:
        raise ValueError("dof and n must be positive")
    if not 0.0 < prob < 1.0:
        raise ValueError("prob must be in (0, 1)")
    d = float(n) * float(dof)
    return chi2_ppf(0.5 * (1.0 - prob), d) / n, chi2_ppf(0.5 * (1.0 + prob), d) / n


def anees(nees, skip=None):
    """(mean[8], left_out[8]): the column means of nees (B, 8) over the filters that are finite in that column and not skipped, and
    how many filters each column left out.  A column without a filter left has mean NaN."""
    a = np.asarray(nees, np.float64)
    if a.ndim != 2 or a.shape[1] != NEES_COLS:
        raise ValueError(f"nees must be (B, {NEES_COLS}), got {a.shape}")
    use = np.isfinite(a)
    if skip is not None:
        use &= (np.asarray(skip).reshape(-1, 1) == 0)
    cnt = use.sum(axis=0)
    tot = np.where(use, a, 0.0).sum(axis=0)
    mean = np.where(cnt > 0, tot / np.maximum(cnt, 1), np.nan)
    return mean, a.shape[0] - cnt


def summary(nees, nstate, prob=0.95, skip=None):
    """per column name: {"mean", "dof", "n", "lo", "hi", "inside"} -- the ANEES of the filters that count (anees) against
    anees_interval for that many.  A column without degrees of freedom (g for nstate 15) or without a filter left has
    lo = hi = NaN and inside = None."""
    mean, out = anees(nees, skip)
    B = np.asarray(nees).shape[0]
    res = {}
    for c, (name, dof) in enumerate(zip(NEES_NAMES, nees_dof(nstate))):
        n = int(B - out[c])
        if dof > 0 and n > 0:
            lo, hi = anees_interval(dof, n, prob)
            inside = bool(lo <= mean[c] <= hi)
        else:
            lo = hi = float("nan")
            inside = None
        res[name] = {"mean": float(mean[c]), "dof": dof, "n": n, "lo": lo, "hi": hi, "inside": inside}
    return res


def sigma_points(nstate, kappa=0.0):
    """(xi (2N + 1, N), weights (2N + 1,)): the symmetric sigma-point set in the coordinates BatchedFilter.sample() takes -- the centre,
    then +sqrt(N + kappa) e_i and -sqrt(N + kappa) e_i for i = 0 .. N - 1 -- with the weights kappa / (N + kappa) and 1 / (2 (N + kappa)):
    sum w = 1, sum w xi = 0, sum w xi xi' = I, so the drawn states have the filter's own mean and covariance.  Broadcast xi over the
    batch -- np.broadcast_to(xi[:, None, :], (2N + 1, B, N)) -- for sample()."""
    if nstate not in (15, 18):
        raise ValueError("nstate must be 15 or 18")
    N, c = nstate, float(nstate) + float(kappa)
    if not c > 0.0:
        raise ValueError("nstate + kappa must be positive")
    if 2 * N + 1 > SAMPLE_MAX:
        raise ValueError("more sigma points than one sample() call takes")
    r = np.sqrt(c)
    xi = np.zeros((2 * N + 1, N))
    xi[1 + np.arange(N), np.arange(N)] = r
    xi[1 + N + np.arange(N), np.arange(N)] = -r
    w = np.full(2 * N + 1, 0.5 / c)
    w[0] = float(kappa) / c
    return xi, w


def draw(flt, S, generator=None):
    """S states per filter drawn from N(estimate, P): torch.randn on the filter's device (generator: a torch.Generator of that device)
    through flt.sample().  Returns (state (S, B, 19), xi (S, B, N)), float64 device tensors; nees(state[s]) is chi-square by
    construction: FULL = |xi[s]|^2."""
    import torch
    xi = torch.randn((int(S), flt.B, flt.N), dtype=torch.float64, device=torch.device("cuda", flt.device), generator=generator)
    return flt.sample(xi), xi


def observe(truth_filter, ids, sigma, generator=None, cameras=2):
    """The pixels a frame would hold if truth_filter's states were the truth: project_markers() on that handle plus N(0, sigma^2) per
    coordinate, on the device.  ids: (B, M) int32 device tensor of the markers asked for.  Returns (ids_seen, left, right): ids_seen =
    ids with -1 where a marker does not have all 4 x cameras corners in view, left / right (right None for cameras=1) in the record
    type -- ready inputs for correct_pixels on ANOTHER handle of the same batch and record type.  With draw() and nees() this closes
    the Monte-Carlo loop on the device: sample -> set_state on a truth handle -> observe -> correct_pixels -> nees."""
    import torch
    left, right, view, _, _ = truth_filter.project_markers(ids, cameras=cameras, cov=False)
    full = 0xFF if cameras == 2 else 0x0F
    ids_seen = torch.where(view == full, ids, torch.full_like(ids, -1))
    noisy = lambda a: a + float(sigma) * torch.randn(a.shape, dtype=a.dtype, device=a.device, generator=generator)
    return ids_seen, noisy(left), (noisy(right) if right is not None else None)
