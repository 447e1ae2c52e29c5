"""GPU suite of the re-acquisition regime: ONE update of every kind against a prior whose position and velocity sigmas have grown by
s = 1, 10, 100 (tests/reacq_ref.py: grown), through the per-call NIS entry points, B = 193 (three 64-filter tiles and a tile of one).
The reference is the fp64 restatement of the kind (depth_ref, velocity_ref, the oracle) in Joseph's form, run on the handle's own state.

The figure that counts here is reacq_ref.meas_err, the relative error of the posterior along the measured rows: it is where
P - u u' / S cancels when H P H' >> R, and util.cov_rel_err_blockwise cannot see it for an update that is not of full rank
(tests/test_reacquisition_cpu.py pins that).  Both figures are held, per cell and rung, to

  (a) forms whose covariance arithmetic is double with one rounding per element (depth and velocity, fp32 records):
      max(COV_BLOCK_TOL, FLOOR_FACTOR x record_floor) -- a double result rounded once IS the fp64 reference rounded once, up to the way
      single roundings fall;
  (b) fp64 records: max(F64_TOL for meas_err / COV_BLOCK_TOL_F64 for cov-block, 2 x the disagreement of the reference's own two forms,
      (I - K H) P and Joseph's) -- that disagreement is how ill-conditioned the rung is in double, the 2 is for summation order;
  (c) fp32 arithmetic (pose, pixels, corners): max(COV_BLOCK_TOL, 2 x the same figure of reacq_ref.seq32 on the same inputs) -- seq32 is
      what float32 arithmetic of the stacked update achieves, the 2 covers fma contraction and the kernels' summation order;
  (d) the returned P is positive definite in every filter ((a), (b): every rung; (c): s <= 10, the count is printed at s = 100) and
      symmetric to the bit;
  (e) util.state_rel_err <= STATE_TOL (fp64: F64_TOL) at EVERY rung, s = 1, 10 and 100: a large prior moves the state by a large K r, the
      sigma-aware denominator accounts for that, and the parity held there when it was first measured (fp32 <= 1.1e-6, fp64 <= 1.6e-14).

Every cell prints one line per rung: figure, bound, kernel / floor."""
import numpy as np
import pytest

import reacq_ref as Q
from fbus_ekf import BatchedFilter
from support import DT, make_filter, update_call
from util import COV_BLOCK_TOL, COV_BLOCK_TOL_F64, F64_TOL, FLOOR_FACTOR, STATE_TOL, cov_rel_err_blockwise, state_rel_err

pytestmark = pytest.mark.gpu


def handle_of(c):
    """the cell's handle as the kind's own suite builds it; depth and velocity: three predicts behind set_state (the carried rotation is
    the stale one) and the sensor set"""
    if c.kind in ("depth", "velocity"):
        f = BatchedFilter(c.B, c.prm, device=0, dtype=c.dtype, nstate=c.n)
        f.set_state(*c.state)
        for k in range(3):
            f.predict(c.acc[k], c.gyr[k], DT)
        if c.kind == "depth":
            f.set_depth_sensor(Q.DEPTH["axis"], Q.DEPTH["offset"], Q.DEPTH["lever"])
        else:
            f.set_velocity_sensor(Q.VELOCITY["mount"], Q.VELOCITY["lever"])
        return f
    return make_filter(c.B, c.prm, c.dtype, c.n, c.state)


def update(f, c):
    if c.kind == "depth":
        f.correct_depth_nis(c.z, Q.DEPTH["var"])
    elif c.kind == "velocity":
        f.correct_velocity_nis(c.z, Q.VELOCITY["var"], c.w)
    elif c.kind in ("pose_nearest", "pose_stacked"):
        update_call(f, "pose", c.ids, c.a, c.b, nis=True, mode=c.mode)
    else:
        update_call(f, c.kind, c.ids, c.a, c.b, nis=True)
    f.sync()


def run_cell(kind, dtype, n, form, joseph=False):
    c = Q.setup(kind, dtype, n, joseph)
    what = f"{kind} f{dtype} N={n}" + (" cov_form Joseph" if joseph else "")
    with handle_of(c) as f:
        st0 = f.get_state()
        Q.measure(c, st0)
        Hs, rs = Q.rows(c, st0)                                       # (the rows do not depend on P)
        for s in Q.LADDER:
            st = Q.grown(st0, s)
            f.set_state(*st)
            update(f, c)
            got, app = f.get_state(), f.applied()
            assert app.all(), (what, s)
            (r_nom, _, r_P, r_prev), r_app = Q.reference(c, st, joseph=True)
            assert r_app.all()
            g_P = np.asarray(got[2], np.float64)
            e = {"meas": Q.meas_err(g_P, r_P, Hs), "cov_block": cov_rel_err_blockwise(g_P, r_P)}
            fl = Q.record_floor(r_P, Hs)
            if form == "a":
                assert dtype == 32
                bound = {k: max(COV_BLOCK_TOL, FLOOR_FACTOR * fl[k]) for k in e}
                base = {k: FLOOR_FACTOR * fl[k] for k in e}
            elif form == "b":
                assert dtype == 64
                alt = Q.reference(c, st, joseph=False)[0][2]
                base = {"meas": Q.meas_err(alt, r_P, Hs), "cov_block": cov_rel_err_blockwise(alt, r_P)}
                bound = {"meas": max(F64_TOL, 2 * base["meas"]), "cov_block": max(COV_BLOCK_TOL_F64, 2 * base["cov_block"])}
            else:
                assert dtype == 32
                S = Q.seq32_batch(st[2], Hs, rs)
                base = {"meas": Q.meas_err(S, r_P, Hs), "cov_block": cov_rel_err_blockwise(S, r_P)}
                bound = {k: max(COV_BLOCK_TOL, 2 * base[k]) for k in e}
                # the domain of the floor, on the handle's own state (tests/test_reacquisition_cpu.py checks it on the initial states)
                assert (Q.min_eig(r_P.astype(np.float32)) > 0).all() and fl["meas"] < 0.05
            es, blk = state_rel_err(got[0], r_nom, r_P)
            pd = int((Q.min_eig(g_P) > 0).sum())
            of = {"a": "its 1.5 x floor", "b": "(I - K H) P vs Joseph", "c": "seq32"}[form]
            print(f"[reacq] {what} s={s} ({form}): meas_err {e['meas']:.2e} (bound {bound['meas']:.2e}, {of} {base['meas']:.2e}, "
                  f"fp32-record floor {fl['meas']:.2e}, kernel / floor {e['meas'] / fl['meas']:.2f})  cov block-wise {e['cov_block']:.2e} "
                  f"(bound {bound['cov_block']:.2e}, {of} {base['cov_block']:.2e}, kernel / floor {e['cov_block'] / fl['cov_block']:.2f})  "
                  f"state {es:.2e} ({blk})  positive definite {pd} of {c.B}")
            assert e["meas"] <= bound["meas"], f"{what} s={s}: meas_err {e['meas']:.3g} > {bound['meas']:.3g}"
            assert e["cov_block"] <= bound["cov_block"], f"{what} s={s}: block-wise covariance rel err {e['cov_block']:.3g} > {bound['cov_block']:.3g}"
            assert np.array_equal(got[2], np.swapaxes(got[2], 1, 2)), f"{what} s={s}: covariance not exactly symmetric"
            if form != "c" or s <= 10:
                assert pd == c.B, f"{what} s={s}: P positive definite in {pd} of {c.B} filters"
            assert es <= (STATE_TOL if dtype == 32 else F64_TOL), f"{what} s={s}: state rel err {es:.3g} in block {blk}"
            assert np.array_equal(got[3], r_prev), f"{what} s={s}: prev marker id"


@pytest.mark.parametrize("kind", ["depth", "velocity"])
@pytest.mark.parametrize("dtype,n,form", [(32, 18, "a"), (64, 15, "b")])
def test_depth_and_velocity_against_a_grown_prior(kind, dtype, n, form):
    run_cell(kind, dtype, n, form)


@pytest.mark.parametrize("joseph", [False, True])
@pytest.mark.parametrize("kind", ["pose_nearest", "pose_stacked"])
def test_pose_rows_against_a_grown_prior(kind, joseph):
    run_cell(kind, 32, 18, "c", joseph)


def test_stacked_pose_rows_fp64_against_a_grown_prior():
    run_cell("pose_stacked", 64, 15, "b")


@pytest.mark.parametrize("kind", ["left", "stereo", "corners"])
def test_image_rows_against_a_grown_prior(kind):
    run_cell(kind, 32, 18, "c")


def test_corner_rows_fp64_against_a_grown_prior():
    run_cell("corners", 64, 15, "b")
