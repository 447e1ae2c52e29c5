"""CPU suite: the promises of tests/support.py that the GPU modules lean on without checking -- cached scenes cannot be written, r32
is float64-valued, env() puts the environment back, same_state() sees one bit in any element."""
import os

import numpy as np
import pytest

import marker_maps as mm
from support import env, r32, same_state, truth_scene


def test_cached_scenes_refuse_writes_and_repeat():
    a, b = truth_scene(8, 2, 3, 5e-4), truth_scene(8, 2, 3, 5e-4)
    assert len(a) == 8 and all(np.array_equal(x, y) for x, y in zip(a, b))
    for x in a:
        assert not x.flags.writeable
        with pytest.raises(ValueError):
            x[0] = 0
    s = mm.pose_scene(Bn=8, M=1)
    for x in s.state + (s.ids, s.pos, s.quat, s.acc, s.gyr, s.dt):
        with pytest.raises(ValueError):
            x[0] = 0
    assert all(np.array_equal(x, y) for x, y in zip(s.state, mm.pose_scene(Bn=8, M=1).state))


def test_r32_is_float64_valued_and_idempotent():
    x = np.array([0.1, 1.0 / 3.0, 1e-9, 123456.789])
    y = r32(x)
    assert y.dtype == np.float64 and not np.array_equal(x, y)
    assert np.array_equal(y, y.astype(np.float32)) and np.array_equal(r32(y), y)
    assert r32([0.1]).dtype == np.float64 and r32(np.float32(0.1)).dtype == np.float64


def test_env_restores_set_and_unset_variables_also_when_the_body_raises():
    os.environ["FBUS_SUPPORT_TEST_SET"] = "before"
    os.environ.pop("FBUS_SUPPORT_TEST_UNSET", None)
    try:
        with env(FBUS_SUPPORT_TEST_SET=1, FBUS_SUPPORT_TEST_UNSET="x"):
            assert os.environ["FBUS_SUPPORT_TEST_SET"] == "1" and os.environ["FBUS_SUPPORT_TEST_UNSET"] == "x"
        assert os.environ["FBUS_SUPPORT_TEST_SET"] == "before" and "FBUS_SUPPORT_TEST_UNSET" not in os.environ
        with pytest.raises(KeyError):
            with env(FBUS_SUPPORT_TEST_SET=2, FBUS_SUPPORT_TEST_UNSET="y"):
                raise KeyError("from the body")
        assert os.environ["FBUS_SUPPORT_TEST_SET"] == "before" and "FBUS_SUPPORT_TEST_UNSET" not in os.environ
    finally:
        os.environ.pop("FBUS_SUPPORT_TEST_SET", None)


def _state(B=6, N=18):
    rng = np.random.default_rng(0)
    return (rng.normal(size=(B, 19)).astype(np.float32), rng.normal(size=(B, 9)).astype(np.float32),
            rng.normal(size=(B, N, N)).astype(np.float32), np.arange(B, dtype=np.int32), np.ones(B, np.uint8))


@pytest.mark.parametrize("k", range(5))
def test_same_state_sees_one_bit_in_every_element(k, capsys):
    a, b = _state(), _state()
    assert same_state(a, b) and same_state(a[:4], b[:4])
    flat = b[k].reshape(len(b[k]), -1)                       # (a view: the write lands in b[k])
    bits = flat[4:5, -1:].view({4: np.uint32, 1: np.uint8}[flat.itemsize])
    bits ^= 1                                                # the lowest bit of one value of filter 4
    assert not same_state(a, b)
    assert ("nominal", "rot", "P", "prev", "applied")[k] in capsys.readouterr().out
    assert same_state(a[:k], b[:k]) and same_state(a, b, rows=slice(0, 4)) and same_state(a, b, rows=[0, 5])
    assert not same_state(a, b, rows=[4])
