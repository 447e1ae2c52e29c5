"""GPU suite: every form of an update -- device pointers (_dev), host pointers (staged and waited), the asynchronous ring (_async) and
the _nis twins -- computes the same bits and refuses the same calls with the same status.  Only the public ABI and the Python mirror
are used.

Shapes: B = 130 (two full 64-filter tiles and a two-filter tail: a partial wave, and the team / split routes of a small launch),
M = 2 (the smallest M at which the divided pixel / corner updates engage), N = 18, fp32 and fp64 records, pose rows in the C++ dialect
(which writes prev_id), skip = (arange(B) % 5 == 1).

The refused calls follow the status table of the entry points: 1 = FBUS_ERR_INVALID, 4 = FBUS_ERR_UNSUPPORTED.  The single-frame forms
have no kcount array: their bad sample count is K = -1 where a window gets a kcount entry of 256."""
import ctypes as C

import numpy as np
import pytest
import torch

from fbus_ekf import BatchedFilter, capi, gating, synth
from support import frozen, perturbed_setup, same_state, to_device

pytestmark = pytest.mark.gpu
B, M, N = 130, 2, 18
SKIP = (np.arange(B) % 5 == 1).astype(np.uint8)
NPD = {32: np.float32, 64: np.float64}
_CACHE = {}


def _pose_inputs(dtype):
    """state, IMU samples and one marker frame (C++ dialect) in the record type"""
    if ("pose", dtype) not in _CACHE:
        c = lambda a: np.ascontiguousarray(a, NPD[dtype])
        prm = capi.default_params(1)
        nom, rot, P, prev = synth.initial_state(0, B, list(prm.p0_diag), N, mixed_cov=True)
        acc, gyr = synth.imu_samples(0, B, 0, 3, nom)
        ids, pos, quat = synth.marker_frame(0, B, 0, M, nom, prm)
        _CACHE["pose", dtype] = frozen((prm, (c(nom), c(rot), c(P), prev), c(acc), c(gyr), np.ascontiguousarray(ids, np.int32), c(pos), c(quat)))
    return _CACHE["pose", dtype]


def _image_inputs(dtype, kind):
    """kind "stereo": pixel rows left / right (B, M, 8); "corners": left = (B, M, 12) corner positions"""
    if (kind, dtype) not in _CACHE:
        c = lambda a: np.ascontiguousarray(a, NPD[dtype])
        prm, nom, rot, P, prev, ids, left, right = perturbed_setup(B, dtype, N, 1, kind, M=M, n=B)
        _CACHE[kind, dtype] = frozen((prm, (c(nom), c(rot), c(P), prev), np.ascontiguousarray(ids, np.int32), c(left), c(right)))
    return _CACHE[kind, dtype]


def _snapshot(f):
    """(records, applied) of a handle, complete"""
    return f.get_state() + (f.applied(),)


# ---- the transports are bit-equal ---------------------------------------------------------------------------------------------------
# (method, arrays, trailing arguments, the form has an _async twin)
def _update_cases(dtype):
    prm, state, _, _, ids, pos, quat = _pose_inputs(dtype)
    ppx, spx, ipx, lpx, rpx = _image_inputs(dtype, "stereo")
    pc3, sc3, ic3, lc3, _ = _image_inputs(dtype, "corners")
    return {
        "pose stacked": (prm, state, "correct", (ids, pos, quat), (capi.MODE_STACKED,), True),
        "pose nearest": (prm, state, "correct", (ids, pos, quat), (capi.MODE_NEAREST,), True),
        "pixels left": (ppx, spx, "correct_pixels", (ipx, lpx, None), (), True),
        "pixels stereo": (ppx, spx, "correct_pixels", (ipx, lpx, rpx), (), True),
        "corners 3d": (pc3, sc3, "correct_corners", (ic3, lc3, None), (capi.VIS_CORNERS3D, capi.MODE_STACKED), False),
        "corners refractive": (ppx, spx, "correct_corners", (ipx, lpx, rpx), (capi.VIS_REFRACTIVE, capi.MODE_STACKED), False),
    }


@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("case", ["pose stacked", "pose nearest", "pixels left", "pixels stereo", "corners 3d", "corners refractive"])
def test_update_transports_are_bit_equal(case, dtype):
    prm, state, method, arrays, tail, has_async = _update_cases(dtype)[case]

    def run(transport, nis=False, gate=None):
        with BatchedFilter(B, prm, dtype=dtype, nstate=N) as f:
            f.set_state(*state)
            if gate is not None:
                f.set_gate(gate)
            name = method + ("_nis" if nis else "") + ("_async" if transport == "async" else "")
            conv = to_device if transport == "dev" else (lambda a: a)
            args = [conv(a) for a in arrays]
            out = getattr(f, name)(*args, *tail, skip=conv(SKIP))
            f.sync()
            if nis:
                out = tuple(o.cpu().numpy() if transport == "dev" else o for o in out)
            return _snapshot(f), out

    ref, _ = run("dev")
    applied = ref[-1]
    assert applied.any() and not applied[SKIP == 1].any() and (SKIP == 1).any()
    assert not same_state(ref[:4], state)                                       # (the update moved the records)
    assert same_state(run("host")[0], ref), "host-pointer form"
    if has_async:
        assert same_state(run("async")[0], ref), "_async form"
    for gate in (None, gating.chi2_gate(0.999, 64)):
        sd, (nis_d, dof_d) = run("dev", nis=True, gate=gate)
        sh, (nis_h, dof_h) = run("host", nis=True, gate=gate)
        assert same_state(sd, sh), "_nis host-pointer form"
        assert np.array_equal(nis_d, nis_h) and np.array_equal(dof_d, dof_h)
        assert sd[-1].any() and not sd[-1][SKIP == 1].any()
        assert np.isfinite(nis_d[sd[-1] == 1]).all() and (dof_d[sd[-1] == 1] > 0).all()


@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("K,per", [(1, 0), (3, 0), (3, 1)])
def test_predict_transports_are_bit_equal(K, per, dtype):
    prm, state, acc, gyr, _, _, _ = _pose_inputs(dtype)
    dt = np.full((K, B) if per else (K,), 0.005, NPD[dtype])
    if per:
        dt *= 1.0 + 0.01 * (np.arange(B) % 3)
    got = []
    for transport in ("dev", "host", "async"):
        with BatchedFilter(B, prm, dtype=dtype, nstate=N) as f:
            f.set_state(*state)
            if transport == "dev":
                f.predict_n(to_device(acc[:K]), to_device(gyr[:K]), to_device(dt), K=K)
            elif transport == "host":
                (f.predict if K == 1 else f.predict_n)(acc[:K], gyr[:K], dt)
            else:
                f.predict_async(acc[:K], gyr[:K], dt, K=K)
            f.sync()
            got.append(f.get_state())
    assert not same_state(got[0], state)
    assert same_state(got[1], got[0]), "host-pointer form"
    assert same_state(got[2], got[0]), "_async form"


# ---- every form refuses the same calls the same way ------------------------------------------------------------------------------------
class _Forms:
    """One handle and the raw entry points of one update.  A call is the valid call's named arguments with a few replaced; `dev` and
    `host` hold each array on the device and on the host."""

    def __init__(self, flt, host, order):
        self.f, self.lib, self.h = flt, flt._lib, flt._h
        self.host = host
        self.dev = {k: to_device(v) if isinstance(v, np.ndarray) else v for k, v in host.items()}
        self.order = order                          # {form name: its parameters behind the handle, in order}
        self.table = np.zeros(B * capi.NOISE_COLS, np.float64)

    @staticmethod
    def _arg(v):
        if v is None or isinstance(v, int):
            return v
        return C.c_void_p(v.data_ptr()) if hasattr(v, "data_ptr") else v.ctypes.data_as(C.c_void_p)

    def call(self, form, **bad):
        vals = dict(self.dev if form.endswith("_dev") else self.host)
        vals.update(bad)
        return getattr(self.lib, "fbus_ekf_" + form)(self.h, *[self._arg(vals[k]) for k in self.order[form]])

    def message(self):
        return self.lib.fbus_ekf_last_error(self.h).decode()

    def refuses(self, form, status, message=None, **bad):
        """the bad call returns `status` (with `message` in last_error), changes nothing and queues nothing; the valid call then runs"""
        f = self.f
        before, calls = _snapshot(f), f.async_stats()["calls"]
        # (no noise table is set: this puts a known text into last_error, which a successful call leaves as it is)
        assert self.lib.fbus_ekf_get_noise(self.h, self.table.ctypes.data_as(C.POINTER(C.c_double))) == 1
        rc = self.call(form, **bad)
        assert rc == status, (form, bad.keys(), rc)
        if message is not None:
            assert message in self.message(), (form, self.message())
        f.sync()
        assert same_state(_snapshot(f), before), (form, "a refused call changed the handle")
        assert f.async_stats()["calls"] == calls
        if not self.broken:
            assert self.call(form) == 0, (form, self.message())
            f.sync()

    broken = False                                  # (True while the valid call itself is refused: r_pix = 0, a short gate table)


def _stem(form):
    """the name the messages carry: the entry point without its transport suffix"""
    for suffix in ("_dev", "_async"):
        form = form[:-len(suffix)] if form.endswith(suffix) else form
    return "fbus_ekf_" + form


def _offset_view(a):
    """the same values in device memory one element behind a 16-byte boundary"""
    t = torch.empty(a.size + 4, dtype=torch.from_numpy(a).dtype, device="cuda")
    v = t[1:1 + a.size]
    v.copy_(torch.from_numpy(a).reshape(-1))
    assert v.data_ptr() % 16 != 0
    return v


MEAS = ["M", "ids", "a", "b"]


@pytest.mark.parametrize("dtype", [32, 64])
def test_predict_forms_refuse_alike(dtype):
    prm, state, acc, gyr, _, _, _ = _pose_inputs(dtype)
    one, n = ["accel", "gyro", "dt", "per"], ["K", "accel", "gyro", "dt", "per"]
    order = {"predict_dev": one, "predict": one, "predict_async": one, "predict_n_dev": n, "predict_n": n, "predict_n_async": n}
    with BatchedFilter(B, prm, dtype=dtype, nstate=N) as f:
        f.set_state(*state)
        x = _Forms(f, {"K": 1, "accel": acc[0], "gyro": gyr[0], "dt": np.array([0.005], NPD[dtype]), "per": 0}, order)
        for form in order:
            for name in ("accel", "gyro", "dt"):
                x.refuses(form, 1, **{name: None})
            if "_n" in form:
                x.refuses(form, 1, K=0)


@pytest.mark.parametrize("dtype", [32, 64])
def test_pose_forms_refuse_alike(dtype):
    prm, state, _, _, ids, pos, quat = _pose_inputs(dtype)
    plain, nis = MEAS + ["mode", "skip"], MEAS + ["mode", "skip", "nis", "dof"]
    order = {"correct_dev": plain, "correct": plain, "correct_async": plain, "correct_nis_dev": nis, "correct_nis": nis}
    with BatchedFilter(B, prm, dtype=dtype, nstate=N) as f:
        f.set_state(*state)
        x = _Forms(f, {"M": M, "ids": ids, "a": pos, "b": quat, "mode": capi.MODE_STACKED, "skip": SKIP,
                       "nis": np.zeros(B, NPD[dtype]), "dof": np.zeros(B, np.int32)}, order)
        for form in order:
            for name in ("ids", "a", "b"):
                x.refuses(form, 1, **{name: None})
            x.refuses(form, 1, M=0)
            x.refuses(form, 1, M=capi.MAX_VISIBLE + 1)
            x.refuses(form, 4, mode=7)
            x.refuses(form, 1, a=None, mode=7)                               # the null test comes first
        x.broken = True
        f.set_gate(gating.chi2_gate(0.999, 7 * M - 1))                       # 7 rows per marker in the C++ dialect: dof 14 has no entry
        for form in ("correct_nis_dev", "correct_nis"):
            x.refuses(form, 1, _stem(form))
            x.refuses(form, 4, mode=7)                                       # the mode test comes before the gate's
            assert x.call(form, mode=capi.MODE_NEAREST) == 0                 # (nearest: dof 7 at the most)
        for form in ("correct_dev", "correct", "correct_async"):
            assert x.call(form) == 0                                         # (the plain updates ignore the table)
        f.sync()


@pytest.mark.parametrize("dtype", [32, 64])
def test_pixel_forms_refuse_alike(dtype):
    prm, state, ids, left, right = _image_inputs(dtype, "stereo")
    plain, nis = MEAS + ["skip"], MEAS + ["skip", "nis", "dof"]
    order = {"correct_pixels_dev": plain, "correct_pixels": plain, "correct_pixels_async": plain,
             "correct_pixels_nis_dev": nis, "correct_pixels_nis": nis}
    host = {"M": M, "ids": ids, "a": left, "b": right, "skip": SKIP, "nis": np.zeros(B, NPD[dtype]), "dof": np.zeros(B, np.int32)}
    with BatchedFilter(B, prm, dtype=dtype, nstate=N) as f:
        f.set_state(*state)
        x = _Forms(f, host, order)
        for form in order:
            for name in ("ids", "a"):
                x.refuses(form, 1, **{name: None})
            x.refuses(form, 1, M=0)
            x.refuses(form, 1, M=capi.MAX_VISIBLE + 1)
            if form.endswith("_dev"):
                x.refuses(form, 1, _stem(form), a=_offset_view(left))
                x.refuses(form, 1, _stem(form), b=_offset_view(right))
        x.broken = True
        f.set_gate(gating.chi2_gate(0.999, 8 * M))                           # stereo reaches dof 16 M, the left camera alone 8 M
        for form in ("correct_pixels_nis_dev", "correct_pixels_nis"):
            x.refuses(form, 1, _stem(form))
            assert x.call(form, b=None) == 0
        f.sync()
    p0 = capi.default_params(1)
    C.memmove(C.byref(p0), C.byref(prm), C.sizeof(prm))
    p0.r_pix = 0.0
    with BatchedFilter(B, p0, dtype=dtype, nstate=N) as f:
        f.set_state(*state)
        x = _Forms(f, host, order)
        x.broken = True
        for form in order:
            x.refuses(form, 1, "r_pix must be positive")
            x.refuses(form, 1, a=None)                                       # (the null test comes first: no message is asked for)


@pytest.mark.parametrize("dtype", [32, 64])
def test_corner_forms_refuse_alike(dtype):
    prm, state, ids, left, right = _image_inputs(dtype, "stereo")
    plain = MEAS + ["geometry", "mode", "skip"]
    nis = plain + ["nis", "dof"]
    order = {"correct_corners_dev": plain, "correct_corners": plain, "correct_corners_nis_dev": nis, "correct_corners_nis": nis}
    with BatchedFilter(B, prm, dtype=dtype, nstate=N) as f:
        f.set_state(*state)
        x = _Forms(f, {"M": M, "ids": ids, "a": left, "b": right, "geometry": capi.VIS_REFRACTIVE, "mode": capi.MODE_STACKED,
                       "skip": SKIP, "nis": np.zeros(B, NPD[dtype]), "dof": np.zeros(B, np.int32)}, order)
        for form in order:
            for name in ("ids", "a"):
                x.refuses(form, 1, **{name: None})
            x.refuses(form, 1, M=0)
            x.refuses(form, 1, M=capi.MAX_VISIBLE + 1)
            x.refuses(form, 4, geometry=9)
            x.refuses(form, 1, b=None)                                       # a stereo geometry without the right camera
            x.refuses(form, 1, b=None, geometry=capi.VIS_PINHOLE)
            x.refuses(form, 4, mode=7)
            x.refuses(form, 1, a=None, mode=7)                               # precedence: the null test, then geometry, then mode
            x.refuses(form, 4, geometry=9, mode=7)
            x.refuses(form, 4, geometry=9, b=None)
            if form.endswith("_dev"):
                x.refuses(form, 1, _stem(form), a=_offset_view(left))
                x.refuses(form, 1, _stem(form), b=_offset_view(right))
        x.broken = True
        f.set_gate(gating.chi2_gate(0.999, 12 * M - 1))                      # stacked reaches dof 12 M, nearest 12
        for form in ("correct_corners_nis_dev", "correct_corners_nis"):
            x.refuses(form, 1, _stem(form))
            x.refuses(form, 4, mode=7)
            assert x.call(form, mode=capi.MODE_NEAREST) == 0
        f.sync()


@pytest.mark.parametrize("dtype", [32, 64])
def test_frame_forms_refuse_alike(dtype):
    prm, state, acc, gyr, ids, pos, quat = _pose_inputs(dtype)
    pc3, sc3, ic3, lc3, _ = _image_inputs(dtype, "corners")
    F, kcount = 2, np.array([1, 2], np.int32)
    two = lambda a: np.ascontiguousarray(np.stack([a, a]))
    imu, pose = ["accel", "gyro", "dt", "per"], ["M", "ids", "a", "b", "mode", "skip"]
    meas = ["kind", "M", "ids", "a", "b", "geometry", "mode", "skip"]
    traj = ["nom", "pdiag", "app"]
    common = {"K": 3, "F": F, "kcount": kcount, "accel": acc, "gyro": gyr, "dt": np.full(3, 0.005, NPD[dtype]), "per": 0, "M": M,
              "mode": capi.MODE_STACKED, "nom": np.zeros((F, B, 19), NPD[dtype]), "pdiag": np.zeros((F, B, N), NPD[dtype]),
              "app": np.zeros((F, B), np.uint8)}
    one = {"ids": ids, "a": pos, "b": quat, "skip": SKIP}
    win = {k: two(v) for k, v in one.items()}
    one3 = {"ids": ic3, "a": lc3, "b": None, "skip": SKIP, "kind": capi.MEAS_CORNERS, "geometry": capi.VIS_CORNERS3D}
    win3 = {k: two(v) if isinstance(v, np.ndarray) else v for k, v in one3.items()}
    # every form here takes device pointers whatever its name ends in: the arrays go to the device for all of them
    groups = [
        (prm, state, {**common, **one}, {"frame_dev": ["K"] + imu + pose, "frame_fused_dev": ["K"] + imu + pose}),
        (prm, state, {**common, **win}, {"frames_fused_dev": ["F", "kcount"] + imu + pose,
                                          "frames_fused_traj_dev": ["F", "kcount"] + imu + pose + traj}),
        (pc3, sc3, {**common, **one3}, {"frame_meas_fused_dev": ["K"] + imu + meas}),
        (pc3, sc3, {**common, **win3}, {"frames_meas_fused_dev": ["F", "kcount"] + imu + meas}),
    ]
    for p, st, host, order in groups:
        with BatchedFilter(B, p, dtype=dtype, nstate=N) as f:
            f.set_state(*st)
            x = _Forms(f, host, order)
            x.dev["kcount"] = kcount                                         # (kcount is a host array)
            for form in order:
                x.refuses(form, 1, gyro=None)
                x.refuses(form, 4, mode=7)
                if "kcount" in order[form]:
                    x.refuses(form, 1, kcount=np.array([1, 256], np.int32))
                    if "kind" not in order[form]:                            # pose windows: the mode test comes before kcount's entries
                        x.refuses(form, 4, kcount=np.array([1, 256], np.int32), mode=7)
                else:
                    x.refuses(form, 1, K=-1)
