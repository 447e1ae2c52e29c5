"""CPU suite: the scene of tests/imu_edges.py is what it claims to be, and the parity gate sees what the scene is there to find.

  * the plain numpy restatement of ImuUpdate equals the C oracle on the scene (two separately written fp64 texts of the same lines);
  * the reference is finite on every class after every sample and its covariance positive definite;
  * every class stands in every full wave at every sample index; enough samples realise a denormal-square and an exact zero rate;
  * an exact-arithmetic filter with fp32 records stays a factor of ten inside every gate over the K samples -- a condition on the
    INPUTS: a kernel that misses a gate on this scene cannot blame its record type;
  * each wrong variant of the step (imu_edges.MUTANTS) run through the scene is refused by util.assert_parity -- by the fp32 gate, or
    where fp32 cannot see it by the fp64 gate; the table (mutant -> gate, figure, class) is printed."""
import numpy as np
import pytest

import imu_edges as ie
from util import assert_parity, parity_errors

CASES = [(18, 0), (18, 1), (15, 0), (15, 1)]
ids = lambda c: f"n{c[0]}-d{c[1]}"


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_the_restatement_equals_the_oracle(case):
    s = ie.scene(*case)
    for stream in ie.STREAMS:
        ref, got = ie.reference(*case, stream), ie.restated_run(s, stream)
        for k in range(ie.K + 1):
            assert np.abs(got[k][0] - ref[k][0]).max() <= 1e-12 and np.abs(got[k][1] - ref[k][1]).max() <= 1e-12, (stream, k)
            scale = np.sqrt(np.einsum("bii->bi", ref[k][2]))
            assert (np.abs(got[k][2] - ref[k][2]) / (scale[:, :, None] * scale[:, None, :])).max() <= 1e-12, (stream, k)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_the_reference_is_finite_and_positive_definite_on_every_class(case):
    for stream in ie.STREAMS:
        for k, (nom, rot, P, _) in enumerate(ie.reference(*case, stream)):
            assert np.isfinite(nom).all() and np.isfinite(rot).all() and np.isfinite(P).all(), (stream, k)
            assert np.linalg.eigvalsh(P).min() > 0, (stream, k)
            assert np.abs(np.linalg.norm(nom[:, 6:10], axis=1) - 1).max() < (1e-7 if k == 0 else 1e-12), (stream, k)   # (k = 0: rounded to fp32)


def test_the_substitute_moves_the_matlab_reference_by_less_than_1e_13():
    """the zero-rate samples of the Matlab dialect against the C++ dialect's own small-rate formula is no test of the substitute; its size
    is: 1e-12 rad/s over at most 1 s turns the attitude by 1e-12 rad, half of that in the quaternion"""
    s = ie.scene(18, 0)
    sub = (s.gyr_oracle != s.gyr).any(axis=2)
    assert sub.sum() >= 100 and (s.w2[sub] < ie.DENORMAL).all() and (s.w2[~sub] >= ie.DENORMAL).all()
    assert np.abs(s.gyr_oracle - s.gyr).max() <= 1e-12 + 3e-20
    assert (ie.scene(18, 1).gyr_oracle == ie.scene(18, 1).gyr).all()             # the C++ dialect: none


def test_class_counts():
    s = ie.scene(18, 0)
    assert s.cls.shape == (ie.K, ie.B) and ie.B == 193 and ie.K == 7 and ie.C == 16
    for k in range(ie.K):
        for wave in range(ie.B // 64):
            assert set(s.cls[k, 64 * wave:64 * wave + 64]) == set(range(ie.C)), (k, wave)
    for case in CASES:
        s = ie.scene(*case)
        denormal = (s.w2 > 0) & (s.w2 < 1.17549435e-38)
        print(f"n{case[0]} d{case[1]}: {denormal.sum()} denormal-square samples, {(s.w2 == 0).sum()} exact zero rates")
        assert denormal.sum() >= 10 and (s.w2 == 0).sum() >= 100
        assert (denormal <= (s.cls == 1)).all()
        # every filter changes class from sample to sample, and the realised rates lie on the side of the guard the class names
        assert (np.diff(s.cls, axis=0) % ie.C == 1).all()
        rate = np.sqrt(s.w2)
        for c, (r, _, _) in enumerate(ie.CLASSES):
            if r > 1e-6:
                assert np.abs(rate[s.cls == c] / r - 1).max() < 1e-3, c
        assert (rate[np.isin(s.cls, (2, 3, 9, 10, 15))] < 10e-5).all() and (rate[s.cls == 4] > 10e-5).all()
        half = rate * np.abs(s.dt["per"]) / 2
        assert (half[s.cls == 6] < 0.5).all() and (half[np.isin(s.cls, (7, 8))] > 0.5).all()


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_fp32_records_stay_a_tenth_inside_every_gate(case):
    for stream in ie.STREAMS:
        fl = ie.record_floor(*case, stream)
        print(f"[floor] n{case[0]} d{case[1]} {stream}: " + "  ".join(f"{k} {fl[k]:.1e}" for k in ie.GATES))
        for name, gate in ie.GATES.items():
            assert fl[name] <= gate / 10, (stream, name, fl[name])


# mutant -> (the gate that has to refuse it, on the scene or on the guard probe).  Every mutant but (c) is refused by the fp32 gate on the
# scene's per-filter stream.  (c) moves the guard from 1e-4 to 1e-5 rad/s: the rates in between then take the exact increment in place of
# the first-order one, and the two differ in the third order of the angle -- 6e-14 rad at 9e-5 rad/s over 1 s, which neither gate sees
# on the scene (asserted below: should that change, this table is stale).  The fp64 gate refuses it on imu_edges.guard_probe.
EXPECTED = {"a": (32, False), "b": (32, False), "c": (64, True), "d": (32, False), "e": (32, False), "f": (32, False)}


def _carrier(s, stream, dialect, mutant, guard, gates):
    """the class whose single step, re-seeded from the reference, carries the mutant's error: (its name, figure, value)"""
    if guard:
        return f"the guard probe ({ie.GUARD_PROBE[0]:g} rad/s, dt {ie.GUARD_PROBE[1]:g} s)", None, None
    q = list(s.prm.q_diag)
    per_class = ie.step_class_figures(s, stream, lambda st, k: ie.imu_update(
        st[0], st[1], st[2], s.acc[k], s.gyr_oracle[k], np.broadcast_to(ie.period_of(s, stream, k), (ie.B,)), dialect, q, mutant), gates)
    c = max(per_class, key=lambda k: per_class[k][2])
    return ie.class_name(c, stream), per_class[c][0], per_class[c][1]


@pytest.mark.parametrize("mutant", sorted(ie.MUTANTS))
def test_the_gate_catches_the_mutant(mutant):
    gate, on_probe = EXPECTED[mutant]
    for dialect in ((1,) if mutant in ie.CPP_ONLY else (0, 1)):
        caught = {}
        for guard in (False, True) if on_probe else (False,):
            s = (ie.guard_probe if guard else ie.scene)(18, dialect)
            for stream in ie.STREAMS:
                ref, got = ie.reference(18, dialect, stream, guard)[-1], ie.restated_run(s, stream, mutant)[-1]
                for dtype in (32, 64):
                    try:
                        assert_parity(got, ref, dtype, f"mutant ({mutant})", verbose=False)
                    except AssertionError as e:
                        name, fig, val = _carrier(s, stream, dialect, mutant, guard, ie.GATES if dtype == 32 else ie.GATES_F64)
                        caught[guard, stream] = dtype
                        print(f"[mutant] ({mutant}) {ie.MUTANTS[mutant]}: dialect {dialect} stream {stream}: refused by the fp{dtype} gate: "
                              f"{str(e).split(': ', 1)[1]}; carried by {name}" + (f": {fig} {val:.2e} in one step" if fig else ""))
                        break
                else:
                    fig, val, ratio = ie.worst_figure(parity_errors(got, ref), ie.GATES_F64)
                    print(f"[mutant] ({mutant}) {ie.MUTANTS[mutant]}: dialect {dialect} stream {stream}{' (guard probe)' if guard else ''}: "
                          f"seen by neither gate: worst {fig} {val:.2e} = {ratio:.1e} x the fp64 gate")
        assert caught.get((on_probe, "per")) == gate and caught.get((on_probe, "shared")) is not None, (mutant, dialect, caught)
        if on_probe:
            assert (False, "per") not in caught and (False, "shared") not in caught, caught
        s = (ie.guard_probe if on_probe else ie.scene)(18, dialect)
        with pytest.raises(AssertionError):
            assert_parity(ie.restated_run(s, "per", mutant)[-1], ie.reference(18, dialect, "per", on_probe)[-1], gate, "mutant", verbose=False)
        # ... and the restatement without a mutant passes the gate that refused the mutant
        assert_parity(ie.restated_run(s, "per")[-1], ie.reference(18, dialect, "per", on_probe)[-1], gate, "no mutant", verbose=False)
