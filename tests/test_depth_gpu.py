"""GPU suite of the depth (pressure) sensor update (include/fbus_ekf.h, fbus_ekf_correct_depth*; csrc/ekf_depth.hpp) against
tests/depth_ref.py, the fp64 restatement on ekf_oracle_np.State: the parity of one update (the body is sensor_families.one_update, which
the three streamed sensor updates share) and of a chain, and the refusals.  NIS / gate / untouched lanes, the five forms and a captured
graph, per-filter variance, the likelihood sums and independence of the neighbours are in tests/test_sensor_suite_gpu.py, once for the
three updates.
B = 193 (three 64-filter tiles and a tile of one) unless stated."""
import ctypes as C

import numpy as np
import pytest

import depth_ref
import oracle_capi as oc
from fbus_ekf import BatchedFilter, capi, synth
from sensor_families import Depth, one_update
from support import B_IND, DT, imu_of, markers_of, r32, same_state, state_batch, to_device
from util import assert_window_parity

pytestmark = pytest.mark.gpu

B = B_IND
AXIS, LEVER, OFFSET, VAR = Depth.AXIS, Depth.LEVER, Depth.OFFSET, Depth.SENSOR_VAR


# ---- parity ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,n,dialect", [(d, n, dl) for d in (32, 64) for n in (18, 15) for dl in (0, 1)])
def test_one_update_against_the_restatement(dtype, n, dialect):
    one_update(Depth(), dtype, n, dialect)


@pytest.mark.parametrize("n,dialect", [(18, 1), (15, 0)])
def test_a_chain_of_predicts_depth_updates_and_pose_updates(n, dialect):
    """12 x (predict_n K = 7, correct_depth), a stacked pose update every fourth step, free-running against the oracle + depth_ref"""
    K, STEPS = 7, 12
    prm, nom, rot, P, prev = state_batch(B, dialect, n)
    a_unit = depth_ref.unit(AXIS)
    orc = oc.Oracle(dialect, n)
    ref = [np.array(nom), np.array(rot), np.array(P), np.array(prev)]
    with BatchedFilter(B, prm, device=0, dtype=32, nstate=n) as f:
        f.set_state(nom, rot, P, prev)
        f.set_depth_sensor(AXIS, OFFSET, LEVER)
        for step in range(STEPS):
            acc, gyr = imu_of(0, B, step * K, K, nom)
            f.predict_n(acc, gyr, np.repeat(DT, K))
            for k in range(K):
                orc.predict(*ref, acc[k], gyr[k], DT)
            if step % 4 == 3:
                ids, pos, quat = markers_of(0, B, step, 4, nom, prm)
                f.correct(ids, pos, quat, capi.MODE_STACKED)
                orc.correct(*ref, ids, pos, quat, oc.STACKED)
            z = r32(synth.depth(0, B, step, nom, rot, axis=AXIS, offset=OFFSET, lever=LEVER, noise=0.01))
            before = f.get_state()
            f.correct_depth(z, VAR)
            after = f.get_state()
            assert f.applied().all()
            ref = list(Depth().ref(ref, n, dict(z=z, var=VAR))[0])
            # the update shrinks the variance along its own row: H P H' < var afterwards, and never above its value before
            hph = []
            for st in (before, after):
                R, Pm = np.asarray(st[1], np.float64).reshape(B, 3, 3), np.asarray(st[2], np.float64)
                H = np.zeros((B, n))
                H[:, 0:3] = a_unit
                H[:, 6:9] = np.cross(LEVER, np.einsum("bji,j->bi", R, a_unit))
                hph.append(np.einsum("bi,bij,bj->b", H, Pm, H))
            assert (hph[1] < VAR).all(), (step, hph[1].max())
            assert (hph[1] <= hph[0] * (1 + 1e-4)).all(), step
        got = f.get_state()
    assert_window_parity(got, ref, f"depth chain N={n} dialect {dialect}", dialect, n)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_launch_nothing():
    prm, nom, rot, P, prev = state_batch(B, 1, 18)
    with BatchedFilter(B, prm, device=0, dtype=32, nstate=18) as f:
        f.set_state(nom, rot, P, prev)
        st0 = f.get_state()
        z, var = np.zeros(B, np.float32), np.full(B, VAR)
        dz, dv = to_device(z), to_device(var)
        for name, call in (("fbus_ekf_correct_depth", lambda: f.correct_depth(z, VAR)),
                           ("fbus_ekf_correct_depth_dev", lambda: f.correct_depth(dz, dv)),
                           ("fbus_ekf_correct_depth_async", lambda: f.correct_depth_async(z, VAR)),
                           ("fbus_ekf_correct_depth_nis", lambda: f.correct_depth_nis(z, VAR)),
                           ("fbus_ekf_correct_depth_nis_dev", lambda: f.correct_depth_nis(dz, dv))):
            with pytest.raises(capi.FbusError) as e:                 # before set_depth_sensor
                call()
            assert e.value.code == 1 and "fbus_ekf_set_depth_sensor" in str(e.value) and name + ":" in str(e.value), str(e.value)
        for axis in ([0.0, 0.0, 0.0], [np.nan, 0.0, 1.0], [np.inf, 0.0, 0.0]):
            with pytest.raises(capi.FbusError) as e:
                f.set_depth_sensor(axis)
            assert e.value.code == 1 and "fbus_ekf_set_depth_sensor" in str(e.value)
        with pytest.raises(capi.FbusError):                           # (a refused setter sets nothing)
            f.correct_depth(z, VAR)
        f.set_depth_sensor(AXIS, OFFSET, LEVER)
        vp = lambda t: C.c_void_p(t.data_ptr())
        for name in ("fbus_ekf_correct_depth_dev", "fbus_ekf_correct_depth_nis_dev"):
            tail = (None, None) if "nis" in name else ()
            assert getattr(f._lib, name)(f._h, vp(dz), vp(dv), 2, None, *tail) == 1
            assert name in f._lib.fbus_ekf_last_error(f._h).decode() and "var_per_filter" in f._lib.fbus_ekf_last_error(f._h).decode()
            assert getattr(f._lib, name)(f._h, None, vp(dv), 0, None, *tail) == 1
            assert name in f._lib.fbus_ekf_last_error(f._h).decode()
        f.sync()
        assert same_state(st0, f.get_state()) and (f.applied() == 0).all()
