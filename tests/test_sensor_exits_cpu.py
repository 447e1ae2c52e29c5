"""CPU companion of tests/test_sensor_exits_gpu.py: the lane plan of tests/exits_plan.py meets its own counts, the threshold chooser finds
its gap on the restatements' nis, and the three restatements (depth_ref, velocity_ref, rows_ref) hold ONE rule for a lane that is not
applied -- a pivot that is not > 0, or nis <= thr false (a NaN among them)."""
import numpy as np
import pytest

import depth_ref
import exits_plan as X
import rows_ref as W
import velocity_ref as V
from support import state_batch

FAMILIES = [("depth", 1), ("velocity", 3), ("rows", 1), ("rows", 2), ("rows", 3)]


@pytest.mark.parametrize("name,m", FAMILIES)
def test_the_lane_plan_meets_its_own_counts(name, m):
    kinds, planted = X.lane_plan(name)
    assert len(kinds) == X.B == 321
    X.plan_conditions(name, kinds, planted)
    b = np.arange(X.B)
    for k in X.kinds_of(name):                                        # every kind has its lanes in the mixed tiles (tile 1 aside, for skip)
        assert ((kinds == k) & (b // 64 != 1)).sum() >= 6, X.KIND_NAMES[k]
    assert (kinds[64:128] == X.SKIP).all() and (kinds[192:256] == X.CLEAN).all() and planted[192:256].all()
    assert kinds[320] == X.CLEAN and not planted[320]
    assert not (planted & (kinds != X.CLEAN)).any()
    if name == "depth":
        assert not (kinds == X.EXTRA).any()
    # the unusable lanes sit where sensor_families.Rows.mixed puts them
    mixed = (b // 64 != 1) & (b // 64 != 3)
    un = ~X.usable_kind(kinds) & mixed
    assert np.array_equal(un, mixed & (np.isin(b % 16, (3, 7, 11, 15)) | np.isin(b % 32, (5, 13, 21, 29))))


def test_the_threshold_chooser_on_a_known_sample():
    v = np.concatenate([np.linspace(1.0, 2.0, 85), [2.5, 2.6, 2.7], np.linspace(3.0, 4.0, 12)])
    thr, half = X.choose_threshold(np.random.default_rng(0).permutation(v))
    assert thr == pytest.approx(2.25) and half == pytest.approx(0.25 / 2.25)          # the gap 2.0 .. 2.5 lies in the 0.80 .. 0.95 band
    assert (np.abs(v - thr) >= half * thr * (1 - 1e-12)).all()


@pytest.mark.parametrize("n", [18, 15])
@pytest.mark.parametrize("name,m", FAMILIES)
def test_the_threshold_on_the_restatements_nis(name, m, n):
    """state_batch states (without the device's predicts), fp32-representable inputs: the gap is there, and the restatement's own
    partition at the threshold keeps >= 64 applied and >= 10 rejected lanes"""
    fam = X.family(name, m)
    prm, nom, rot, P, prev = state_batch(X.B, X.DIALECT[n], n)
    case = X.prepare(fam, (nom, rot, P, prev), 32, n, fam.aux_cpu(X.B, n, nom))
    print(f"{fam} N={n}: thr {case.thr:.6g}, relative half-width {case.half:.3e}, applied {int(case.gated[1].sum())}")
    assert case.half >= X.HALF_WIDTH
    X.reference_conditions(fam, case)
    pool = (case.kinds == X.CLEAN) & ~case.planted
    nis = case.free[2][pool]
    assert (np.abs(nis - case.thr) >= case.half * case.thr * (1 - 1e-12)).all()
    app = case.gated[1].astype(bool)
    assert app.sum() >= 64 and ((case.kinds == X.CLEAN) & ~app).sum() >= 10 + 64       # (tile 3 is rejected whole)


def _same(a, b):
    """(applied, nis, dof) of two restatements: the flags and dof equal, nis equal to rounding, NaN where the other is NaN"""
    assert a[0] == b[0] and a[2] == b[2], (a, b)
    assert (np.isnan(a[1]) and np.isnan(b[1])) or abs(a[1] - b[1]) <= 1e-13 * abs(b[1]), (a, b)


@pytest.mark.parametrize("n", [18, 15])
def test_the_three_restatements_agree_on_the_rule(n):
    """the depth row through rows_ref.correct_rows and through depth_ref.correct_depth: the same (applied, nis, dof) on a healthy state,
    on a state of NaN (nis is NaN: not applied, dof 1) and on one with a negated covariance (S < 0: not applied, dof 1), without a gate
    and with one on either side of nis; and the velocity rows through rows_ref and velocity_ref likewise"""
    D, VS = X.Depth(), X.Velocity()
    prm, nom, rot, P, prev = state_batch(8, X.DIALECT[n], n)
    gyro = VS.aux_cpu(8, n, nom)
    a = depth_ref.unit(D.AXIS)
    seen = set()
    for form in ("healthy", "nan", "negated"):
        for b in range(8):
            s = V.states_of((nom, rot, P, prev), n)[b]
            z = depth_ref.h(s, a, D.OFFSET, D.LEVER) + 0.01 * (1 + b)
            zv = V.h(s, VS.MOUNT, VS.LEVER, gyro[b]) + 0.01 * (1 + b)
            # the caller of correct_rows forms its rows at the nominal state it read: the healthy one (a NaN residual is an unusable input)
            H, res = depth_ref.H_row(s, n, a, D.LEVER), z - depth_ref.h(s, a, D.OFFSET, D.LEVER)
            Hv, resv = V.H_rows(s, n, VS.MOUNT, VS.LEVER, gyro[b]), zv - V.h(s, VS.MOUNT, VS.LEVER, gyro[b])
            if form == "nan":
                s.p, s.v, s.q, s.ba, s.bg, s.g, s.R, s.P = (np.full_like(x, np.nan) for x in (s.p, s.v, s.q, s.ba, s.bg, s.g, s.R, s.P))
            elif form == "negated":
                s.P = -s.P
            var = 2.5e-5                                                # below H P H' (1e-4): the negated covariance gives S < 0
            with np.errstate(all="ignore"):
                free = depth_ref.correct_depth(_copy(s, n), n, z, var, D.AXIS, D.OFFSET, D.LEVER)
                for thr in (np.inf,) if np.isnan(free[1]) else (np.inf, 0.5 * abs(free[1]), 2.0 * abs(free[1])):
                    d = depth_ref.correct_depth(_copy(s, n), n, z, var, D.AXIS, D.OFFSET, D.LEVER, thr)
                    r = W.correct_rows(_copy(s, n), n, [res], H, [var], thr)
                    _same(d[:3], r[:3])
                    assert d[2] == 1
                    assert d[0] == (form == "healthy" and d[1] <= thr)
                    seen.add((form, bool(d[0])))
                    if form == "negated":
                        assert d[3] < 0 and d[1] < 0                     # S < 0, so nis < 0 <= thr: the lane the old rule applied
                v = V.correct_velocity(_copy(s, n), n, zv, VS.VAR, gyro[b], VS.MOUNT, VS.LEVER)
                r = W.correct_rows(_copy(s, n), n, resv, Hv, VS.VAR)
            assert v[0] == r[0] == (form == "healthy") and v[2] == r[2] == 3
            assert (np.isnan(v[1]) and np.isnan(r[1])) or abs(v[1] - r[1]) <= 1e-9 * abs(r[1])
    assert seen == {("healthy", True), ("healthy", False), ("nan", False), ("negated", False)}


def _copy(s, n):
    import ekf_oracle_np as E
    c = E.State(n)
    c.p, c.v, c.q, c.ba, c.bg, c.g, c.R, c.P, c.prev_id = tuple(np.array(x) for x in (s.p, s.v, s.q, s.ba, s.bg, s.g, s.R, s.P)) + (s.prev_id,)
    return c
