"""GPU suite of the body-velocity (DVL) update (include/fbus_ekf.h, fbus_ekf_correct_velocity*; csrc/ekf_velocity.hpp) against
tests/velocity_ref.py, the fp64 restatement on ekf_oracle_np.State: the parity of one update (the body is sensor_families.one_update,
which the three streamed sensor updates share) and of a chain, and the refusals.  NIS / gate / untouched lanes, the five forms and a
captured graph, per-filter variance, the likelihood sums and independence of the neighbours are in tests/test_sensor_suite_gpu.py, once
for the three updates.
B = 193 (three 64-filter tiles and a tile of one) unless stated.

Why the fp32 kernel does its covariance arithmetic in double (measured on an MI355X).  support.state_batch behind three predicts carries a
prior velocity variance of 0.12 .. 0.18 (m/s)^2 -- the gravity prior of 100 reaches v through the predicts -- and the update takes it to
the order of var, 2.5e-5 .. 4e-4: a factor of 500 .. 2000 in one step.  With P - u u' / s in fp32 the block-wise covariance figure of
these cases came out at 1.9e-5 .. 3.45e-4 against COV_BLOCK_TOL = 1e-5, and diag(H P+ H') / var at 1.0008 after the chain's first update
(exact: 1 - 1e-3); a numpy emulation of the sequential and of the joint form in fp32 gave the same 4.0e-4.  With the joint form in double
and one rounding per element the same cases read 5.8e-8 .. 1.6e-7."""
import ctypes as C

import numpy as np
import pytest

import depth_ref
import oracle_capi as oc
import velocity_ref as V
from fbus_ekf import BatchedFilter, capi, synth
from sensor_families import Depth, Velocity, one_update
from support import B_IND, DT, imu_of, markers_of, r32, same_state, state_batch, to_device
from util import assert_window_parity

pytestmark = pytest.mark.gpu

B = B_IND
MOUNT, LEVER, VAR = Velocity.MOUNT, Velocity.LEVER, Velocity.VAR


# ---- parity ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,n,dialect", [(d, n, dl) for d in (32, 64) for n in (18, 15) for dl in (0, 1)])
def test_one_update_against_the_restatement(dtype, n, dialect):
    one_update(Velocity(), dtype, n, dialect)


@pytest.mark.parametrize("n,dialect", [(18, 1), (15, 0)])
def test_a_chain_of_predicts_velocity_depth_and_pose_updates(n, dialect):
    """12 x (predict_n K = 7, correct_velocity), a stacked pose update every fourth step and a depth update every third, free-running
    against the oracle + depth_ref + velocity_ref"""
    K, STEPS = 7, 12
    AXIS, OFFSET, DLEVER, DVAR = Depth.AXIS, Depth.OFFSET, Depth.LEVER, Depth.SENSOR_VAR
    prm, nom, rot, P, prev = state_batch(B, dialect, n)
    orc = oc.Oracle(dialect, n)
    ref = [np.array(nom), np.array(rot), np.array(P), np.array(prev)]
    Cm = V.mount_of(MOUNT)
    worst = []
    with BatchedFilter(B, prm, device=0, dtype=32, nstate=n) as f:
        f.set_state(nom, rot, P, prev)
        f.set_velocity_sensor(MOUNT, LEVER)
        f.set_depth_sensor(AXIS, OFFSET, DLEVER)
        for step in range(STEPS):
            acc, gyr = imu_of(0, B, step * K, K, nom)
            f.predict_n(acc, gyr, np.repeat(DT, K))
            for k in range(K):
                orc.predict(*ref, acc[k], gyr[k], DT)
            if step % 4 == 3:
                ids, pos, quat = markers_of(0, B, step, 4, nom, prm)
                f.correct(ids, pos, quat, capi.MODE_STACKED)
                orc.correct(*ref, ids, pos, quat, oc.STACKED)
            if step % 3 == 2:
                zd = r32(synth.depth(0, B, step, nom, rot, axis=AXIS, offset=OFFSET, lever=DLEVER, noise=0.01))
                f.correct_depth(zd, DVAR)
                ss = V.states_of(ref, n)
                for b, s in enumerate(ss):
                    assert depth_ref.correct_depth(s, n, float(zd[b]), DVAR, AXIS, OFFSET, DLEVER)[0]
                ref = list(V.arrays_of(ss))
            w = gyr[K - 1]
            z = r32(synth.velocity(0, B, step, nom, rot, w, mount=MOUNT, lever=LEVER, noise=0.01))
            before = f.get_state()
            f.correct_velocity(z, VAR, w)
            after = f.get_state()
            assert f.applied().all()
            ref = list(Velocity().ref(ref, n, dict(z=z, var=VAR, gyro=w))[0])
            # the update shrinks the variance along its own rows: diag(H P+ H') < var (H P+ H' = R - R S^-1 R for the joint update), and
            # the velocity block does not grow
            R0, nom0 = np.asarray(before[1], np.float64).reshape(B, 3, 3), np.asarray(before[0], np.float64)
            H = np.zeros((B, 3, n))
            H[:, :, 3:6] = np.einsum("km,bjm->bkj", Cm, R0)
            wv = np.einsum("bji,bj->bi", R0, nom0[:, 3:6])
            H[:, :, 6:9] = np.einsum("km,bmj->bkj", Cm, np.array([depth_skew(x) for x in wv]))
            H[:, :, 12:15] = Cm @ depth_skew(LEVER)
            hph = np.einsum("bki,bij,bkj->bk", H, np.asarray(after[2], np.float64), H)
            tr = [np.trace(np.asarray(st[2], np.float64)[:, 3:6, 3:6], axis1=1, axis2=2) for st in (before, after)]
            worst.append(((hph / VAR).max(), (tr[1] / tr[0]).max()))
        got = f.get_state()
    for step, (rows, trace) in enumerate(worst):
        print(f"step {step}: max diag(H P+ H') / var = {rows:.6f}, max trace P_vv after / before = {trace:.6f}")
    try:
        assert_window_parity(got, ref, f"velocity chain N={n} dialect {dialect}", dialect, n)
    finally:
        for step, (rows, trace) in enumerate(worst):
            assert rows < 1.0, (step, rows)
            assert trace <= 1 + 1e-4, (step, trace)


def depth_skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_launch_nothing():
    prm, nom, rot, P, prev = state_batch(B, 1, 18)
    with BatchedFilter(B, prm, device=0, dtype=32, nstate=18) as f:
        f.set_state(nom, rot, P, prev)
        st0 = f.get_state()
        z, var = np.zeros((B, 3), np.float32), np.tile(VAR, (B, 1))
        dz, dv = to_device(z), to_device(var)
        last = lambda: f._lib.fbus_ekf_last_error(f._h).decode()
        for name, call in (("fbus_ekf_correct_velocity", lambda: f.correct_velocity(z, VAR)),
                           ("fbus_ekf_correct_velocity_dev", lambda: f.correct_velocity(dz, dv)),
                           ("fbus_ekf_correct_velocity_async", lambda: f.correct_velocity_async(z, VAR)),
                           ("fbus_ekf_correct_velocity_nis", lambda: f.correct_velocity_nis(z, VAR)),
                           ("fbus_ekf_correct_velocity_nis_dev", lambda: f.correct_velocity_nis(dz, dv))):
            with pytest.raises(capi.FbusError) as e:                 # before set_velocity_sensor
                call()
            assert e.value.code == 1 and "fbus_ekf_set_velocity_sensor" in str(e.value) and name + ":" in str(e.value), str(e.value)
        skewed, nan_mount = MOUNT.copy(), MOUNT.copy()
        skewed[0, 1] += 1e-3                                          # max |C C' - I| ~ 1e-3
        nan_mount[2, 2] = np.nan
        for mount, lever in ((skewed, None), (2.0 * np.eye(3), None), (nan_mount, None), (np.full((3, 3), np.inf), None),
                             (MOUNT, [0.0, np.nan, 0.0])):
            with pytest.raises(capi.FbusError) as e:
                f.set_velocity_sensor(mount, lever)
            assert e.value.code == 1 and "fbus_ekf_set_velocity_sensor" in str(e.value)
        with pytest.raises(capi.FbusError):                           # (a refused setter sets nothing)
            f.correct_velocity(z, VAR)
        f.set_velocity_sensor(MOUNT, LEVER)
        vp = lambda t: C.c_void_p(t.data_ptr())
        for name in ("fbus_ekf_correct_velocity_dev", "fbus_ekf_correct_velocity_nis_dev"):
            tail = (None, None) if "nis" in name else ()
            assert getattr(f._lib, name)(f._h, vp(dz), None, vp(dv), 2, None, *tail) == 1
            assert name in last() and "var_per_filter" in last()
            assert getattr(f._lib, name)(f._h, None, None, vp(dv), 0, None, *tail) == 1
            assert name in last()
            assert getattr(f._lib, name)(f._h, vp(dz), None, None, 0, None, *tail) == 1
            assert name in last()
        # inside a capture: the setter and the host form
        f._check(f._lib.fbus_ekf_graph_begin(f._h), "graph_begin")
        try:
            mt = (C.c_double * 9)(*np.eye(3).ravel())
            assert f._lib.fbus_ekf_set_velocity_sensor(f._h, mt, None) == 1
            assert "fbus_ekf_set_velocity_sensor" in last()
            hz, hv = z.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p)
            assert f._lib.fbus_ekf_correct_velocity(f._h, hz, None, hv, 1, None) == 1
            assert "fbus_ekf_correct_velocity:" in last()
            assert f._lib.fbus_ekf_correct_velocity_nis(f._h, hz, None, hv, 1, None, None, None) == 1
            assert "fbus_ekf_correct_velocity_nis:" in last()
        finally:
            gid = C.c_int(-1)
            f._lib.fbus_ekf_graph_end(f._h, C.byref(gid))
        f.sync()
        assert same_state(st0, f.get_state()) and (f.applied() == 0).all()
        # the refused setter inside the capture kept the sensor: the bits of a handle that was given the tilted mount and nothing else
        zr = Velocity().readings(st0, 32, None, Velocity.MOUNT_ONLY)["z"]
        f.correct_velocity(zr, VAR)
        got = f.get_state()
    with BatchedFilter(B, prm, device=0, dtype=32, nstate=18) as f:
        f.set_state(nom, rot, P, prev)
        f.set_velocity_sensor(MOUNT, LEVER)
        f.correct_velocity(zr, VAR)
        assert same_state(got, f.get_state()) and not same_state(got, st0)
