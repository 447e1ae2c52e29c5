"""BatchedFilter: the reference filter's predict()/correct() contract for B filters on one GPU.

Mirrors `State = ImuUpdate(State, accel, gyro, dt)` (matlab/ImuUpdate.m:36) and
`State = MeasureUpdate(State, visionMeas, markerMap, cameraInfo)`
(matlab/MeasureUpdate.m:37) / FILTER::UpdateCovariance+UpdateNominalState and
FILTER::ObservationUpdate (C++/src/filter.cpp:588-616,533-582,622-754), with the
state owned by the object as in the C++ FILTER class.  All arithmetic happens in
libfbus_ekf.so; this class only converts arguments.

Host (numpy) arrays go through the staging entry points; device arrays (anything
with `.data_ptr()`, e.g. torch tensors on the handle's GPU) go to the `_dev` entry
points without copies.
"""
import ctypes as C

import numpy as np

from . import capi
from . import noise
from .noise import COLUMNS


def _is_dev(x):
    return hasattr(x, "data_ptr")


class BatchedFilter:
    def __init__(self, batch, params=None, dialect=capi.DIALECT_MATLAB, device=0, dtype=32, nstate=18,
                 stream=None, order_streams=True):
        self._lib = capi.load_library()
        self._h = C.c_void_p()
        self.params = params if params is not None else capi.default_params(dialect)
        self.B, self.device, self.dtype, self.N = int(batch), int(device), int(dtype), int(nstate)
        self.np_dtype = np.float32 if dtype == 32 else np.float64
        rc = self._lib.fbus_ekf_create_checked(C.byref(self._h), C.byref(self.params), C.sizeof(capi.FbusParams), capi.ABI_VERSION,
                                               self.B, self.device, self.dtype, self.N)
        if rc != 0:
            self._h = C.c_void_p()
            raise capi.FbusError(rc, "fbus_ekf_create", self._lib.fbus_status_string(rc).decode())
        self._keep = []          # device arrays that must outlive asynchronous launches
        self._async_inputs = []  # host inputs of correct_depth_async / correct_velocity_async (pinned ones are DMA'd in place): until async_inputs_consumed() / sync()
        # The handle starts on its own NON-BLOCKING stream: device arrays handed to predict/correct/frame must be
        # complete before the call and results are complete after sync() (or order the streams with
        # wait_stream()/signal_stream(), or share the caller's stream with set_stream()).
        self._own_stream = True
        # order_streams (default): while the handle runs on its own stream, every device-array call first makes that
        # stream wait for the caller's current torch stream (inputs produced there, e.g. an upload or a .to(dtype), are
        # complete before a kernel reads them) and afterwards makes the caller's stream wait for the call (results are
        # visible to work queued there).  A caller that synchronises by itself (bench.py's timed region) switches it
        # off: the two event markers per call cost launch-stream time.
        self.order_streams = bool(order_streams)
        self._capturing = False
        if stream is not None:
            self.set_stream(stream)

    # ---- plumbing -------------------------------------------------------------
    def _check(self, rc, where):
        if rc != 0:
            detail = self._lib.fbus_ekf_last_error(self._h).decode() or self._lib.fbus_status_string(rc).decode()
            raise capi.FbusError(rc, where, detail)

    def close(self):
        if self._h:
            self._lib.fbus_ekf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, stream):
        """stream: an int/hipStream_t handle or an object with `.cuda_stream` (torch.cuda.Stream); the handle is passed
        as it is -- 0 is HIP's legacy default stream (what torch.cuda.current_stream() is unless the caller switched
        streams), so the launches are ordered with the caller's own work.  stream=None restores the handle's own stream."""
        if stream is None:
            handle = capi.STREAM_OWN
        else:
            handle = int(getattr(stream, "cuda_stream", stream))
        self._check(self._lib.fbus_ekf_set_stream(self._h, C.c_void_p(handle)), "set_stream")
        self._own_stream = stream is None

    def set_team(self, predict_roles=0, correct_roles=0):
        """waves per 64-filter tile of predict / correct: 0 = chosen per launch (default), 1 = one wave per tile, 2..4 fixed.
        predict_roles also governs predict_n and the fused frame / frame window entry points (the four-role pipeline), correct_roles also
        correct_corners (stacked mode) and correct_pixels (2 = two waves per tile, 3..4 = four) -- include/fbus_ekf.h, DESIGN.md 4.5"""
        self._check(self._lib.fbus_ekf_set_team(self._h, int(predict_roles), int(correct_roles)), "set_team")

    def set_policy_batch(self, total_filters):
        """the batch the automatic kernel-family choice is keyed on: the WHOLE job when this handle holds one shard of it
        (every shard layout then runs the same kernels: bit-equal results); 0 = this handle's own batch"""
        self._check(self._lib.fbus_ekf_set_policy_batch(self._h, int(total_filters)), "fbus_ekf_set_policy_batch")

    def launch_info(self, what, arg=0):
        v = C.c_int(0)
        self._check(self._lib.fbus_ekf_launch_info(self._h, int(what), int(arg), C.byref(v)), "fbus_ekf_launch_info")
        return v.value

    def launch_policy(self, M=4, K=7):
        """the handle's launch policy as a dict (what bench.py records beside its numbers)"""
        c = capi
        return {"simds": self.launch_info(c.INFO_SIMDS), "one_round_filters": self.launch_info(c.INFO_ONE_ROUND_FILTERS),
                "two_wave_min_b": self.launch_info(c.INFO_TWO_WAVE_MIN_B), "big_records_MB": self.launch_info(c.INFO_BIG_RECORDS_MB),
                "mall_MB": self.launch_info(c.INFO_MALL_MB), "l2_KB": self.launch_info(c.INFO_L2_KB),
                "policy_batch": self.launch_info(c.INFO_POLICY_BATCH), "roles_predict": self.launch_info(c.INFO_ROLES_PREDICT, 1),
                "roles_predict_n": self.launch_info(c.INFO_ROLES_PREDICT, K), "roles_meas": self.launch_info(c.INFO_ROLES_MEAS, M),
                "team_frames": bool(self.launch_info(c.INFO_TEAM_FRAMES)), "meas_split": self.launch_info(c.INFO_MEAS_SPLIT, M)}

    def wait_stream(self, stream):
        """work submitted to this filter from now on starts after everything already queued on `stream`"""
        self._check(self._lib.fbus_ekf_wait_stream(self._h, C.c_void_p(int(getattr(stream, "cuda_stream", stream)))), "wait_stream")

    def signal_stream(self, stream):
        """work submitted to `stream` from now on starts after everything already queued on this filter"""
        self._check(self._lib.fbus_ekf_signal_stream(self._h, C.c_void_p(int(getattr(stream, "cuda_stream", stream)))), "signal_stream")

    def sync(self):
        self._check(self._lib.fbus_ekf_sync(self._h), "sync")
        self._keep.clear()
        self._async_inputs.clear()

    def _order_in(self, *arrays):
        """own stream + order_streams: wait for the caller's current stream; returns it for _order_out (else None)"""
        if not (self._own_stream and self.order_streams) or self._capturing:
            return None
        dev = next((a for a in arrays if a is not None and _is_dev(a) and hasattr(a, "device")), None)
        if dev is None:
            return None
        try:
            import torch
            cur = torch.cuda.current_stream(dev.device)
        except Exception:           # a non-torch device array: the caller orders the streams
            return None
        self.wait_stream(cur)
        return cur

    def _order_out(self, cur):
        if cur is not None:
            self.signal_stream(cur)

    def _host(self, a, shape, dtype=None):
        a = np.ascontiguousarray(a, dtype or self.np_dtype)
        if a.size != int(np.prod(shape)):
            raise ValueError(f"expected {shape}, got {a.shape}")
        return a

    @staticmethod
    def _p(a):
        if a is None:
            return None
        if _is_dev(a):
            return C.c_void_p(a.data_ptr())
        return a.ctypes.data_as(C.c_void_p)

    def _dev_checked(self, a, numel, what):
        if a.numel() != numel:
            raise ValueError(f"{what}: expected {numel} elements, got {a.numel()}")
        if hasattr(a, "is_contiguous") and not a.is_contiguous():
            raise ValueError(f"{what}: device array must be contiguous")
        self._keep.append(a)
        return a

    # ---- state ----------------------------------------------------------------
    def set_state(self, nominal=None, rot=None, P=None, prev_id=None):
        B, N = self.B, self.N
        if any(_is_dev(x) for x in (nominal, rot, P, prev_id) if x is not None):
            cur = self._order_in(nominal, rot, P, prev_id)
            rc = self._lib.fbus_ekf_set_state_dev(self._h, self._p(nominal), self._p(rot), self._p(P), self._p(prev_id))
            self._check(rc, "set_state_dev")
            return self._order_out(cur)
        nominal = None if nominal is None else self._host(nominal, (B, 19))
        rot = None if rot is None else self._host(rot, (B, 9))
        P = None if P is None else self._host(P, (B, N, N))
        prev_id = None if prev_id is None else self._host(prev_id, (B,), np.int32)
        rc = self._lib.fbus_ekf_set_state(self._h, self._p(nominal), self._p(rot), self._p(P), self._p(prev_id))
        self._check(rc, "set_state")

    def get_state(self):
        B, N = self.B, self.N
        nominal = np.empty((B, 19), self.np_dtype)
        rot = np.empty((B, 9), self.np_dtype)
        P = np.empty((B, N, N), self.np_dtype)
        prev = np.empty(B, np.int32)
        rc = self._lib.fbus_ekf_get_state(self._h, self._p(nominal), self._p(rot), self._p(P), self._p(prev))
        self._check(rc, "get_state")
        return nominal, rot, P, prev

    def get_state_dev(self, cov=False):
        """The state as torch tensors on the handle's device, stream-ordered, without a trip to the host (fbus_ekf_get_state_dev):
        (nominal (B, 19), rot (B, 9)) -- the linearisation point of correct_rows, rot being the CARRIED rotation -- and, with
        cov=True, (nominal, rot, P (B, N, N), prev_id (B,))."""
        import torch
        dev = torch.device("cuda", self.device)
        tt = torch.float32 if self.dtype == 32 else torch.float64
        out = [torch.empty((self.B, 19), dtype=tt, device=dev), torch.empty((self.B, 9), dtype=tt, device=dev)]
        if cov:
            out += [torch.empty((self.B, self.N, self.N), dtype=tt, device=dev), torch.empty(self.B, dtype=torch.int32, device=dev)]
        self._keep.extend(out)
        cur = self._order_in(*out)
        self._check(self._lib.fbus_ekf_get_state_dev(self._h, *(self._p(o) for o in out), *([] if cov else [None, None])), "get_state_dev")
        self._order_out(cur)
        return tuple(out)

    def reset_cov(self):
        self._check(self._lib.fbus_ekf_reset_cov(self._h), "reset_cov")

    def records(self):
        """(device pointer, bytes per filter, total bytes) of the packed records."""
        ptr, bpf, tot = C.c_void_p(), C.c_size_t(), C.c_size_t()
        self._check(self._lib.fbus_ekf_records(self._h, C.byref(ptr), C.byref(bpf), C.byref(tot)), "records")
        return ptr.value, bpf.value, tot.value

    def attach_records(self, dev_array):
        """Make the handle keep its records inside a caller-owned device array (e.g. a torch uint8 tensor)."""
        nbytes = dev_array.numel() * dev_array.element_size()
        self._check(self._lib.fbus_ekf_attach_records(self._h, self._p(dev_array), nbytes), "attach_records")
        self._records_owner = dev_array

    # ---- multi-GPU: the one collective (RCCL inside the library) -------------------------------
    @staticmethod
    def comm_unique_id():
        """128-byte ncclUniqueId (bytes): rank 0 creates it, every rank passes it to comm_init"""
        lib = capi.load_library()
        buf = C.create_string_buffer(128)
        rc = lib.fbus_ekf_comm_unique_id(C.cast(buf, C.c_void_p))
        if rc != 0:
            raise capi.FbusError(rc, "comm_unique_id", lib.fbus_status_string(rc).decode())
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._check(self._lib.fbus_ekf_comm_init(self._h, C.cast(buf, C.c_void_p), int(rank), int(world)), "comm_init")

    def copy_records(self, dst, dst_device=0, byte_offset=0):
        """this handle's packed records into device memory `dst` (+ byte_offset) on `dst_device`, on the handle's stream
        (fbus_ekf_copy_records: the peer-copy form of the gather, what fbus::NodeFilter::gather_to issues per shard).
        dst: a device tensor or a raw device pointer (int)."""
        ptr = dst if isinstance(dst, int) else dst.data_ptr()
        if not isinstance(dst, int):
            self._keep.append(dst)
        self._check(self._lib.fbus_ekf_copy_records(self._h, C.c_void_p(ptr + int(byte_offset)), int(dst_device)), "copy_records")

    def gather(self, out, bytes_of_rank=None):
        """all ranks' packed records into the device array `out` (uint8, sum of the ranks' record bytes) on every rank"""
        arr = None
        if bytes_of_rank is not None:
            arr = (C.c_size_t * len(bytes_of_rank))(*[int(x) for x in bytes_of_rank])
        self._keep.append(out)
        self._check(self._lib.fbus_ekf_gather(self._h, self._p(out), arr), "gather")

    # ---- predict == ImuUpdate -----------------------------------------------------
    def predict(self, accel, gyro, dt):
        return self.predict_n(accel, gyro, dt, K=1)

    def _imu(self, accel, gyro, dt, K=None, what="K", exact=False):
        """(K, per) of the IMU samples of a device-array call, accel / gyro / dt checked and kept alive.  K: the sample count (None: what
        accel holds); per: dt has one entry per sample and filter.  exact: dt may not be longer than K either (predict_n)"""
        B = self.B
        if K is None:
            K = accel.numel() // (3 * B) if accel is not None else 0
        if K <= 0 and not exact:
            return K, 0
        n = dt.numel()
        per = 1 if (n == K * B and B > 1) else 0
        if not per and (n != K if exact else n < K):
            raise ValueError(f"dt must have {what} or {what}*B elements")
        self._dev_checked(accel, K * B * 3, "accel"); self._dev_checked(gyro, K * B * 3, "gyro")
        self._dev_checked(dt, n, "dt")
        return K, per

    def _imu_host(self, accel, gyro, dt, K, conv):
        """(K, accel, gyro, dt, per) of a host-array predict; conv: _host or _host_any"""
        B = self.B
        if K is None:
            accel = np.ascontiguousarray(accel, self.np_dtype)
            K = accel.size // (3 * B)
        accel, gyro = conv(accel, (K, B, 3)), conv(gyro, (K, B, 3))
        dt = np.ascontiguousarray(np.atleast_1d(dt), self.np_dtype)
        per = 1 if (dt.size == K * B and B > 1) else 0
        if not per and dt.size != K:
            raise ValueError("dt must have K or K*B elements")
        return K, accel, gyro, dt, per

    def predict_n(self, accel, gyro, dt, K=None):
        if _is_dev(accel):
            K, per = self._imu(accel, gyro, dt, K, exact=True)
            cur = self._order_in(accel, gyro, dt)
            rc = self._lib.fbus_ekf_predict_n_dev(self._h, K, self._p(accel), self._p(gyro), self._p(dt), per)
            self._check(rc, "predict_n_dev")
            return self._order_out(cur)
        K, accel, gyro, dt, per = self._imu_host(accel, gyro, dt, K, self._host)
        rc = self._lib.fbus_ekf_predict_n(self._h, K, self._p(accel), self._p(gyro), self._p(dt), per)
        self._check(rc, "predict_n")

    # ---- the host-pointer calls without the wait (fbus_ekf_*_async) --------------------------------
    def _host_any(self, x, shape, dtype=None):
        """numpy array or a CPU torch tensor (pinned tensors are transferred in place by the library)"""
        if _is_dev(x):
            if x.is_cuda:
                raise ValueError("the _async calls take HOST arrays (device arrays go to predict / correct: already asynchronous)")
            x = x.numpy()              # shares the (possibly pinned) memory
        return self._host(x, shape, dtype)

    def predict_async(self, accel, gyro, dt, K=1):
        """fbus_ekf_predict_n_async: host arrays taken by value, nothing waits for the device (results: sync() / get_state())"""
        K, accel, gyro, dt, per = self._imu_host(accel, gyro, dt, K, self._host_any)
        self._check(self._lib.fbus_ekf_predict_n_async(self._h, K, self._p(accel), self._p(gyro), self._p(dt), per), "predict_n_async")

    def correct_async(self, ids, pos, quat, mode=capi.MODE_NEAREST, skip=None):
        self._update("correct", ids, self._pose_arrays(pos, quat), (mode,), skip, transport="_async")

    def correct_pixels_async(self, ids, left, right=None, skip=None):
        self._update("correct_pixels", ids, self._image_arrays(left, right), (), skip, transport="_async")

    def async_inputs_consumed(self):
        """every H2D copy of the _async calls so far is done: pinned input arrays may be rewritten"""
        self._check(self._lib.fbus_ekf_async_inputs_consumed(self._h), "async_inputs_consumed")
        self._async_inputs.clear()

    def async_stats(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.fbus_ekf_async_stats(self._h, C.byref(a), C.byref(b), C.byref(c)), "async_stats")
        return {"calls": a.value, "waits": b.value, "direct_pieces": c.value}

    # ---- correct == MeasureUpdate -----------------------------------------------------
    def _rows_checked(self, n, M, ids, arrays, skip):
        """the device arrays of n filter-frames of M marker slots, checked and kept alive: ids n * M, every (array, width, name, optional)
        n * M * width elements, skip n"""
        self._dev_checked(ids, n * M, "ids")
        for a, w, name, optional in arrays:
            if a is not None or not optional:
                self._dev_checked(a, n * M * w, name)
        if skip is not None:
            self._dev_checked(skip, n, "skip")

    def _update(self, stem, ids, arrays, tail=(), skip=None, nis=False, transport=None):
        """One measurement update through fbus_ekf_<stem>[_nis]<transport>.  arrays: (array, elements per marker slot, name, optional)
        behind ids; tail: the int arguments behind them; nis: the _nis form, returns its (nis, dof).  transport None: "_dev" for device
        arrays (no copy, ordered with the caller's stream), "" for host arrays (staged, waits); "_async": host arrays, no wait"""
        B = self.B
        cur, out = None, ()
        if transport is None and _is_dev(ids):
            transport, M = "_dev", ids.numel() // B
            self._rows_checked(B, M, ids, arrays, skip)
            arrs = [a for a, _, _, _ in arrays]
            if nis:
                out = self._nis_outputs(ids)
                self._keep += list(out)
            cur = self._order_in(ids, *arrs, skip)
        else:
            conv = self._host_any if transport else self._host
            transport = transport or ""
            ids = np.ascontiguousarray(ids.numpy() if _is_dev(ids) else ids, np.int32).reshape(B, -1)
            M = ids.shape[1]
            arrs = [None if (a is None and optional) else conv(a, (B, M, w)) for a, w, _, optional in arrays]
            skip = None if skip is None else self._host(skip, (B,), np.uint8)
            if nis:
                out = self._nis_outputs(None)
        name = stem + ("_nis" if nis else "") + transport
        rc = getattr(self._lib, "fbus_ekf_" + name)(self._h, M, self._p(ids), *[self._p(a) for a in arrs], *tail, self._p(skip),
                                                    *[self._p(o) for o in out])
        self._check(rc, name)
        self._order_out(cur)
        return out if nis else None

    def correct(self, ids, pos, quat, mode=capi.MODE_NEAREST, skip=None):
        self._update("correct", ids, self._pose_arrays(pos, quat), (mode,), skip)

    def correct_corners(self, ids, left, right=None, geometry=capi.VIS_REFRACTIVE, mode=capi.MODE_NEAREST, skip=None):
        """correct() from stereo corners (north-star extension, no reference counterpart): the corners are
        triangulated on the device and each corner position is a 3-row measurement (12 rows per marker).
        left/right: (B, M, 8) normalised corner coordinates, or left = (B, M, 12) with VIS_CORNERS3D."""
        self._update("correct_corners", ids, self._image_arrays(left, right, capi.MEAS_CORNERS, geometry), (geometry, mode), skip)

    def correct_pixels(self, ids, left, right=None, skip=None):
        """correct() from corner PIXELS (north-star extension, no reference counterpart): the flat-port reprojection of
        the four corners of every visible marker, 2 rows per corner (left camera) or 4 (left and right).
        left/right: (B, M, 8) normalised image points x0 y0 .. x3 y3."""
        self._update("correct_pixels", ids, self._image_arrays(left, right), (), skip)

    @staticmethod
    def _pose_arrays(pos, quat):
        return [(pos, 3, "pos", False), (quat, 4, "quat", False)]

    @staticmethod
    def _image_arrays(left, right, kind=capi.MEAS_PIXELS, geometry=capi.VIS_REFRACTIVE):
        """left / right of the pixel and corner rows: 8 elements per marker slot, left 12 (corner positions) with VIS_CORNERS3D"""
        w = 12 if (kind == capi.MEAS_CORNERS and geometry == capi.VIS_CORNERS3D) else 8
        return [(left, w, "left", False), (right, 8, "right", True)]

    # ---- NIS and chi-square gating of the measurement updates (include/fbus_ekf.h) --------------------------------
    def set_gate(self, thresholds=None):
        """The gate table thr[dof] (e.g. gating.chi2_gate(0.999)); None or empty: no gate.  The *_nis updates leave a filter
        untouched (applied = 0) when its nis > thr[dof]; the other updates ignore the table."""
        if thresholds is None or len(thresholds) == 0:
            return self._check(self._lib.fbus_ekf_set_gate(self._h, 0, None), "set_gate")
        thr = np.ascontiguousarray(thresholds, np.float64).ravel()
        self._check(self._lib.fbus_ekf_set_gate(self._h, int(thr.size), thr.ctypes.data_as(C.POINTER(C.c_double))), "set_gate")

    def set_noise(self, table=None):
        """Per-filter process and measurement noise (fbus_ekf_set_noise): a (B, 7) table, columns noise.COLUMNS (q_v q_theta q_ba q_bg
        r_pos r_quat r_pix, the fbus_params fields of the same names); row b replaces those fields for filter b.  A numpy array (or
        anything np.asarray takes) goes through the host form, which validates every entry; a contiguous float64 device tensor through
        the device form, validated here with torch first.  None: no table (back to the handle's parameters).
        With a table the updates and predicts take the one-wave kernels; frames() / frames_meas() and the fused single frames run the
        resident window kernels that read the table while launch_info(capi.INFO_NOISE_RESIDENT) is 1 (fp32 records, likelihood sums off,
        policy batch above half a chip), and frame by frame through the per-call kernels otherwise."""
        if table is None:
            return self._check(self._lib.fbus_ekf_set_noise(self._h, None), "set_noise")
        B, NC = self.B, capi.NOISE_COLS
        if _is_dev(table):
            import torch
            if table.dtype != torch.float64 or tuple(table.shape) != (B, NC) or not table.is_contiguous():
                raise ValueError(f"set_noise: expected a contiguous float64 ({B}, {NC}) tensor, got {table.dtype} {tuple(table.shape)}")
            bad = ~torch.isfinite(table)
            bad[:, :4] |= table[:, :4] < 0
            bad[:, 4:] |= table[:, 4:] <= 0
            if bool(bad.any()):
                r, c = (int(v) for v in bad.nonzero()[0])
                raise ValueError(f"set_noise: row {r} column {c} ({COLUMNS[c]}) = {float(table[r, c])}: must be finite and "
                                 f"{'>= 0' if c < 4 else '> 0'}")
            self._keep.append(table)
            cur = self._order_in(table)
            self._check(self._lib.fbus_ekf_set_noise_dev(self._h, self._p(table)), "set_noise_dev")
            self._order_out(cur)
            return
        t = np.ascontiguousarray(table, np.float64)
        if t.shape != (B, NC):
            raise ValueError(f"set_noise: expected ({B}, {NC}), got {t.shape}")
        self._check(self._lib.fbus_ekf_set_noise(self._h, t.ctypes.data_as(C.POINTER(C.c_double))), "set_noise")

    def get_noise(self):
        """The current noise table, (B, 7) float64; raises FbusError when none is set."""
        t = np.empty((self.B, capi.NOISE_COLS), np.float64)
        self._check(self._lib.fbus_ekf_get_noise(self._h, t.ctypes.data_as(C.POINTER(C.c_double))), "get_noise")
        return t

    # ---- per-filter innovation log-likelihood sums (include/fbus_ekf.h) --------------------------------------------
    def loglik_enable(self, on=True):
        """Switch the accumulation of ll = -1/2 (nis + log det S + rows ln 2 pi) over every applied measurement update on or off
        (the sums are kept when it goes off).  While on the updates take the one-wave routes, as with a noise table."""
        self._check(self._lib.fbus_ekf_loglik_enable(self._h, 1 if on else 0), "loglik_enable")

    def loglik_reset(self):
        """Zero the sums (stream-ordered)."""
        self._check(self._lib.fbus_ekf_loglik_reset(self._h), "loglik_reset")

    def loglik(self, device=False):
        """(ll float64, rows int64, applied int32, rejected int32), B entries each: numpy arrays (waits for the handle's stream), or
        with device=True torch tensors on the handle's device, stream-ordered."""
        B = self.B
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            out = (torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int64, device=dev),
                   torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
            self._keep += list(out)
            cur = self._order_in(*out)
            self._check(self._lib.fbus_ekf_loglik_get_dev(self._h, *(self._p(o) for o in out)), "loglik_get_dev")
            self._order_out(cur)
            return out
        out = (np.empty(B, np.float64), np.empty(B, np.int64), np.empty(B, np.int32), np.empty(B, np.int32))
        self._check(self._lib.fbus_ekf_loglik_get(self._h, *(self._p(o) for o in out)), "loglik_get")
        return out

    # ---- hypothesis groups: evidence-weighted fusion and collapse (include/fbus_ekf.h) ------------------------------------
    def _group_count(self, G, where):
        G = int(G)
        if not 2 <= G <= capi.GROUP_MAX or self.B % G:
            # (the library refuses the same values; asked first because the output shapes below depend on them)
            self._check(self._lib.fbus_ekf_group_collapse_dev(self._h, G, None), where)
            raise ValueError(f"{where}: G = {G} does not divide the batch of {self.B} into groups of 2..{capi.GROUP_MAX}")
        return G, self.B // G

    def _group_logw(self, logw, dev, where):
        """logw of a group call on the device: None stays None (the handle's likelihood sums), a float64 device tensor is checked,
        anything else is staged"""
        import torch
        if logw is None:
            return None
        if _is_dev(logw):
            if logw.dtype != torch.float64 or not logw.is_cuda:
                raise ValueError(f"{where}: logw must be a float64 device tensor, got {logw.dtype} on {logw.device}")
        else:
            logw = torch.from_numpy(np.ascontiguousarray(logw, np.float64).ravel()).to(dev)
        return self._dev_checked(logw, self.B, "logw")

    def _report_call(self, stem, head, inputs, outputs, device=None):
        """One call of fbus_ekf_<stem>[_dev] that reads its inputs and fills fresh outputs (the group, NEES and sample families), in the
        manner of _sensor_update.  head: the integer arguments in front.  inputs: (name, value, shape, dtype) in call order; a value
        of None is an absent array, a shape of None a device tensor the caller has checked already.  A float64 input must come as
        float64 (tested, never converted), any other is converted on the host branch and taken as it is on the device.  The first
        input decides the branch: a device tensor takes the stream-ordered _dev form, anything else is staged -- unless `device` is
        given, which takes the _dev form on that device.  outputs: (shape, dtype or None for the record type, wanted) in call order.
        Returns the outputs as a tuple, None for one that is not wanted."""
        lead, cur = inputs[0][1], None
        if device is not None or _is_dev(lead):
            import torch
            transport, device = "_dev", lead.device if device is None else device
            for name, a, shape, dtype in inputs:
                if a is None or shape is None:
                    continue
                if dtype is np.float64 and a.dtype != torch.float64:
                    raise ValueError(f"{stem}: {name} must be float64, got {a.dtype}")
                self._dev_checked(a, int(np.prod(shape, dtype=np.int64)), name)
            vals = [a for _, a, _, _ in inputs]
            out = tuple(torch.empty(shape, dtype=getattr(torch, np.dtype(dt or self.np_dtype).name), device=device) if want else None
                        for shape, dt, want in outputs)
            self._keep += [o for o in out if o is not None]
            cur = self._order_in(*vals, *out)
        else:
            transport, vals = "", []
            for name, a, shape, dtype in inputs:
                if a is not None and dtype is np.float64 and np.asarray(a).dtype != np.float64:
                    raise ValueError(f"{stem}: {name} must be float64, got {np.asarray(a).dtype}")
                vals.append(None if a is None else self._host(a, shape, dtype))
            out = tuple(np.empty(shape, dt or self.np_dtype) if want else None for shape, dt, want in outputs)
        name = stem + transport
        rc = getattr(self._lib, "fbus_ekf_" + name)(self._h, *head, *[self._p(a) for a in vals], *[self._p(o) for o in out])
        self._check(rc, name)
        self._order_out(cur)
        return out

    def group_fuse(self, G, logw=None, full_cov=True):
        """Evidence-weighted, moment-matched fusion of every contiguous group of G filters (fbus_ekf_group_fuse_dev): returns
        (weight (B,) float64, best (B/G,) int32, nominal (B/G, 19), P (B/G, N, N) or None, pdiag (B/G, N)), torch tensors on the
        handle's device, stream-ordered.  logw: the per-filter log-weights -- None: the handle's likelihood sums (loglik_enable), a
        float64 device tensor, or anything np.asarray takes (staged to the device).  full_cov=False: the diagonal alone.
        The records are not touched; noise.group_weights is the numpy twin of (weight, best)."""
        import torch
        G, NG = self._group_count(G, "group_fuse_dev")
        dev = torch.device("cuda", self.device)
        logw = self._group_logw(logw, dev, "group_fuse")
        B, N, f64 = self.B, self.N, np.float64
        return self._report_call("group_fuse", (G,), [("logw", logw, None, f64)],
                                 [((B,), f64, True), ((NG,), np.int32, True), ((NG, 19), None, True), ((NG, N, N), None, full_cov),
                                  ((NG, N), None, True)], device=dev)

    def group_collapse(self, G, src):
        """Overwrite every member of group j with the record of its member src[j], bit for bit (fbus_ekf_group_collapse): nominal state,
        carried rotation, covariance and prev_id.  src: (B/G,) member indices; a negative entry skips its group, so group_fuse's `best`
        can be passed straight in.  A device int32 tensor goes through the device form, which inspects nothing (an entry outside
        0..G-1 leaves its group alone); anything else through the host form, which refuses an entry >= G.  Not copied: the applied
        flags, the likelihood sums, the noise table and the carried IMU-EMA sample."""
        G, NG = self._group_count(G, "group_collapse")
        if _is_dev(src):
            import torch
            if src.dtype != torch.int32 or not src.is_cuda:
                raise ValueError(f"group_collapse: src must be an int32 device tensor, got {src.dtype} on {src.device}")
            self._dev_checked(src, NG, "src")
            cur = self._order_in(src)
            self._check(self._lib.fbus_ekf_group_collapse_dev(self._h, G, self._p(src)), "group_collapse_dev")
            return self._order_out(cur)
        src = self._host(src, (NG,), np.int32)
        self._check(self._lib.fbus_ekf_group_collapse(self._h, G, self._p(src)), "group_collapse")

    def group_mix(self, G, trans, logw=None):
        """The IMM mixing step on every contiguous group of G filters, in place (fbus_ekf_group_mix_dev): every member is re-initialised
        from the mixture of its group's members with the weights W_ij = trans[i][j] mu_i / c_j, in the chart of the best member.
        Returns (weight (B,) float64 = mu, logc (B,) float64 = log c_j, the predicted model probabilities), torch tensors on the
        handle's device, stream-ordered.  logw as in group_fuse.  trans: (G, G), trans[i][j] = the probability that model i is
        followed by model j (noise.imm_transition) -- a float64 device tensor goes in as it is, uninspected; anything np.asarray takes
        is held to the host form's rule (finite, >= 0, rows summing to 1: noise.check_transition) and then staged.  A target nothing
        leads to (c_j = 0) and a group without a usable member keep their bytes, logc = -inf; trans = I changes nothing.  prev_id,
        the applied flags, the likelihood sums and the noise table are not touched.  The cycle, all on the device:

            logc = log prior
            loop:
                loglik_reset()
                a window of frames
                logw = logc + loglik(device=True)[0]
                group_fuse(G, logw)                      -> the output estimate
                weight, logc = group_mix(G, trans, logw)
        """
        import torch
        G, _ = self._group_count(G, "group_mix_dev")
        dev = torch.device("cuda", self.device)
        if trans is None:
            self._check(self._lib.fbus_ekf_group_mix_dev(self._h, G, None, None, None, None), "group_mix_dev")
        if _is_dev(trans):
            if trans.dtype != torch.float64 or not trans.is_cuda:
                raise ValueError(f"group_mix: trans must be a float64 device tensor, got {trans.dtype} on {trans.device}")
        else:
            trans = torch.from_numpy(noise.check_transition(trans, G)).to(dev)
        self._dev_checked(trans, G * G, "trans")
        logw = self._group_logw(logw, dev, "group_mix")
        return self._report_call("group_mix", (G,), [("logw", logw, None, np.float64), ("trans", trans, None, np.float64)],
                                 [((self.B,), np.float64, True)] * 2, device=dev)

    # ---- depth (pressure) sensor update (include/fbus_ekf.h; no reference counterpart) ---------------------------------------
    def set_depth_sensor(self, axis, offset=0.0, lever=None):
        """The handle's depth sensor (fbus_ekf_set_depth_sensor): axis = the world-frame direction along which the reading grows
        (normalised by the library; zero or non-finite is refused), offset = the reading at the world origin, lever = the sensor's
        position in the IMU frame (None: 0).  A captured graph keeps the values it was captured with.  No correct_depth* form runs
        before this has been called."""
        ax = (C.c_double * 3)(*np.asarray(axis, np.float64).reshape(3))
        lv = None if lever is None else (C.c_double * 3)(*np.asarray(lever, np.float64).reshape(3))
        self._check(self._lib.fbus_ekf_set_depth_sensor(self._h, ax, float(offset), lv), "fbus_ekf_set_depth_sensor")

    def _sensor_update(self, stem, arrays, var, m, skip, nis, transport, head=()):
        """One streamed sensor update through fbus_ekf_correct_<stem>[_nis]<transport>, on _update's device / host / async branch.
        arrays: the update's own inputs in call order, each (name, value, per-filter shape, may be None); the first one decides the
        branch.  var: m variances or B x m of them, always float64.  head: the integer arguments in front of the arrays."""
        B = self.B
        lead = arrays[0][1]
        counts = f"{m} or {B}" + ("" if arrays[0][2] == () else f" x {m}")
        cur, out = None, ()
        if transport is None and _is_dev(lead):
            import torch
            transport = "_dev"
            for name, a, shape, optional in arrays:
                if not (optional and a is None):
                    self._dev_checked(a, B * int(np.prod(shape, dtype=np.int64)), name)
            vals = [a for _, a, _, _ in arrays]
            if not _is_dev(var):
                var = torch.as_tensor(np.ascontiguousarray(var, np.float64).ravel()).to(lead.device)
            if var.dtype != torch.float64 or var.numel() not in (m, m * B):
                raise ValueError(f"correct_{stem}: var must be float64 with {counts} elements, got {var.dtype} x {var.numel()}")
            self._dev_checked(var, var.numel(), "var")
            if skip is not None:
                self._dev_checked(skip, B, "skip")
            if nis:
                out = self._nis_outputs(lead)
                self._keep += list(out)
            cur = self._order_in(*vals, var, skip)
            per = 1 if (var.numel() == m * B and B > 1) else 0
        else:
            conv = self._host_any if transport else self._host
            transport = transport or ""
            vals = [None if (optional and a is None) else conv(a, (B,) + tuple(shape)) for _, a, shape, optional in arrays]
            var = np.ascontiguousarray(var.numpy() if _is_dev(var) else var, np.float64).ravel()
            if var.size not in (m, m * B):
                raise ValueError(f"correct_{stem}: var must have {counts} elements, got {var.size}")
            per = 1 if (var.size == m * B and B > 1) else 0
            skip = None if skip is None else self._host(skip, (B,), np.uint8)
            if transport == "_async":       # pinned inputs are transferred in place: they live until async_inputs_consumed() / sync()
                self._async_inputs += vals + [var, skip]
            if nis:
                out = self._nis_outputs(None)
        name = f"correct_{stem}" + ("_nis" if nis else "") + transport
        rc = getattr(self._lib, "fbus_ekf_" + name)(self._h, *head, *[self._p(a) for a in vals], self._p(var), per, self._p(skip),
                                                    *[self._p(o) for o in out])
        self._check(rc, name)
        self._order_out(cur)
        return out if nis else None

    def _depth(self, z, var, skip, nis=False, transport=None):
        """One depth update: one variance or B of them."""
        return self._sensor_update("depth", [("z", z, (), False)], var, 1, skip, nis, transport)

    def correct_depth(self, z, var, skip=None):
        """The depth (pressure) sensor update, one scalar row per filter: h = axis . (p + R lever) + offset, dx = P H' (z - h) / S,
        P <- P - P H' H P / S (set_depth_sensor first).  z: (B,) readings in the handle's dtype; var: the reading's variance, one
        float64 or (B,) of them; skip: (B,) uint8.  A filter that is skipped, whose z is not finite or whose var is not a finite
        number > 0 is left untouched; otherwise the update is applied iff S > 0 and nis <= thr[1] of the gate table (set_gate), both
        false for a NaN, as correct_velocity and correct_rows decide: a record of NaN or with S <= 0 is not applied.  Meant for the sensor's own
        rate, between camera frames:  loop { predict_n(imu since the last reading); correct_depth(z, var) }."""
        self._depth(z, var, skip)

    def correct_depth_nis(self, z, var, skip=None):
        """correct_depth() that also returns (nis, dof) per filter: nis = (z - h)^2 / S, dof = 1 (0 and 0 for an untouched filter)."""
        return self._depth(z, var, skip, nis=True)

    def correct_depth_async(self, z, var, skip=None):
        """correct_depth() on host arrays without the wait (fbus_ekf_correct_depth_async)."""
        self._depth(z, var, skip, transport="_async")

    # ---- body-velocity (DVL, zero-velocity) update (include/fbus_ekf.h; no reference counterpart) ------------------------------------
    def set_velocity_sensor(self, mount=None, lever=None):
        """The handle's velocity sensor (fbus_ekf_set_velocity_sensor): mount = the rotation C from the IMU frame to the instrument frame
        (3 x 3, row-major; None: the identity; refused unless max |C C' - I| <= 1e-6), lever = the instrument's position in the IMU
        frame (None: 0).  A captured graph keeps the values it was captured with.  No correct_velocity* form runs before this has
        been called."""
        mt = None if mount is None else (C.c_double * 9)(*np.asarray(mount, np.float64).reshape(9))
        lv = None if lever is None else (C.c_double * 3)(*np.asarray(lever, np.float64).reshape(3))
        self._check(self._lib.fbus_ekf_set_velocity_sensor(self._h, mt, lv), "fbus_ekf_set_velocity_sensor")

    def _velocity(self, z, gyro, var, skip, nis=False, transport=None):
        """One velocity update: three variances or B x 3 of them."""
        return self._sensor_update("velocity", [("z", z, (3,), False), ("gyro", gyro, (3,), True)], var, 3, skip, nis, transport)

    def correct_velocity(self, z, var, gyro=None, skip=None):
        """The body-velocity update (a Doppler velocity log; with z = 0 a zero-velocity update), three rows per filter:
        h = C (R' v + (gyro - bg) x lever), dx = P H' S^-1 (z - h), P <- P - P H' S^-1 H P (set_velocity_sensor first).  z: (B, 3)
        in the handle's dtype, the velocity in the instrument frame; var: the three variances, float64, (3,) or (B, 3); gyro: (B, 3),
        the raw rate sample predict takes (None: the lever term is dropped and the gyro bias is not observed); skip: (B,) uint8.  A
        filter that is skipped, has a non-finite z or gyro component or a variance that is not a finite number > 0 is left untouched;
        the gate table's thr[3] (set_gate) rejects as in the *_nis updates.  Meant for the instrument's own rate, between camera
        frames:  loop { predict_n(imu since the last reading); correct_velocity(z, var, gyro) }."""
        self._velocity(z, gyro, var, skip)

    def correct_velocity_nis(self, z, var, gyro=None, skip=None):
        """correct_velocity() that also returns (nis, dof) per filter: nis = res' S^-1 res, dof = 3 (0 and 0 for an untouched filter)."""
        return self._velocity(z, gyro, var, skip, nis=True)

    def correct_velocity_async(self, z, var, gyro=None, skip=None):
        """correct_velocity() on host arrays without the wait (fbus_ekf_correct_velocity_async)."""
        self._velocity(z, gyro, var, skip, transport="_async")

    # ---- the general linearised measurement update (include/fbus_ekf.h; no reference counterpart) ------------------------------------
    def _rows(self, res, H, var, skip, nis=False):
        """One row update, device or host form (there is no async one).  m is read off res.shape[1]; m variances or B x m of them."""
        B, N = self.B, self.N
        if getattr(res, "ndim", 0) != 2 or res.shape[0] != B:
            raise ValueError(f"correct_rows: res must be ({B}, m), got {tuple(getattr(res, 'shape', ()))}")
        m = int(res.shape[1])
        if _is_dev(res):
            import torch
            dt = torch.float32 if self.dtype == 32 else torch.float64
            if not _is_dev(H) or res.dtype != dt or H.dtype != dt:
                raise ValueError(f"correct_rows: res and H must both be {dt} device tensors")
        elif _is_dev(H):
            H = H.numpy()
        return self._sensor_update("rows", [("res", res, (m,), False), ("H", H, (m, N), False)], var, m, skip, nis, None, head=(m,))

    def correct_rows(self, res, H, var, skip=None):
        """The general linearised measurement update, m = res.shape[1] rows per filter (1..capi.ROWS_MAX): the caller hands over the
        innovation res = z - h(x), (B, m), and the Jacobian rows H, (B, m, N), columns in the error-state order p v theta ba bg [g]
        under the injection's convention R_true ~ R (I + [dtheta]x), both in the handle's dtype; the library does
        S = H P H' + diag(var), dx = P H' S^-1 res -> its own injection, P <- P - P H' S^-1 H P, the NIS, the gate (thr[m] of
        set_gate) and the likelihood sums.  var: the m variances, float64, (m,) or (B, m); skip: (B,) uint8.  torch device tensors
        take the stream-ordered, capturable device form, numpy arrays are staged.  A filter that is skipped, has a non-finite
        residual or entry of H or a variance that is not a finite number > 0 is left untouched.  fbus_ekf.rows has ready-made
        sensors:  loop { predict_n(...); nominal, rot = get_state_dev()[:2]; res, H = rows.position_fix(nominal, rot, z);
        correct_rows(res, H, var) }."""
        self._rows(res, H, var, skip)

    def correct_rows_nis(self, res, H, var, skip=None):
        """correct_rows() that also returns (nis, dof) per filter: nis = res' S^-1 res, dof = m (0 and 0 for an untouched filter)."""
        return self._rows(res, H, var, skip, nis=True)

    def _nis_outputs(self, dev_like):
        if dev_like is not None:
            import torch
            dt = torch.float32 if self.dtype == 32 else torch.float64
            return (torch.empty(self.B, dtype=dt, device=dev_like.device), torch.empty(self.B, dtype=torch.int32, device=dev_like.device))
        return np.empty(self.B, self.np_dtype), np.empty(self.B, np.int32)

    def correct_nis(self, ids, pos, quat, mode=capi.MODE_NEAREST, skip=None):
        """correct() that also returns (nis, dof) per filter and applies the gate (set_gate): numpy arrays for host inputs,
        device tensors for device inputs."""
        return self._update("correct", ids, self._pose_arrays(pos, quat), (mode,), skip, nis=True)

    def correct_pixels_nis(self, ids, left, right=None, skip=None):
        """correct_pixels() that also returns (nis, dof) per filter and applies the gate (set_gate): numpy arrays for host
        inputs, device tensors for device inputs."""
        return self._update("correct_pixels", ids, self._image_arrays(left, right), (), skip, nis=True)

    def correct_corners_nis(self, ids, left, right=None, geometry=capi.VIS_REFRACTIVE, mode=capi.MODE_NEAREST, skip=None):
        """correct_corners() that also returns (nis, dof) per filter and applies the gate (set_gate)."""
        return self._update("correct_corners", ids, self._image_arrays(left, right, capi.MEAS_CORNERS, geometry), (geometry, mode), skip,
                            nis=True)

    # ---- per-marker chi-square screening (include/fbus_ekf.h: fbus_ekf_screen_markers) ----------------------------------
    def screen_markers(self, kind, ids, a, b=None, geometry=capi.VIS_REFRACTIVE, skip=None, inplace=False):
        """Judges every marker slot of every filter on its own against the prior: nis_m = r_m' (H_m P H_m' + R_m)^-1 r_m of the rows
        the kind's stacked update would fold for slot m alone, kept iff nis_m <= thr[dof_m] of the gate table (set_gate; no table:
        only a NaN is dropped).  kind: capi.SCREEN_POSE (a, b = pos, quat), SCREEN_PIXELS (left, right or None) or SCREEN_CORNERS
        (left, right under `geometry`).  Returns (ids_out, nis, dof, kept): ids with -1 in the dropped slots -- hand it to the update
        in place of ids --, nis and dof (B, M), kept (B,) = the slots of the map left per filter; numpy arrays for host inputs, device
        tensors for device inputs.  inplace: ids_out is ids itself.  Read-only: no record, flag or likelihood sum changes."""
        B = self.B
        if kind == capi.SCREEN_POSE:
            arrays = self._pose_arrays(a, b)
        elif kind in (capi.SCREEN_PIXELS, capi.SCREEN_CORNERS):
            arrays = self._image_arrays(a, b, capi.MEAS_CORNERS if kind == capi.SCREEN_CORNERS else capi.MEAS_PIXELS, geometry)
        else:
            raise ValueError(f"screen_markers: kind {kind} is none of SCREEN_POSE / SCREEN_PIXELS / SCREEN_CORNERS")
        cur = None
        if _is_dev(ids):
            import torch
            transport, M = "_dev", ids.numel() // B
            self._rows_checked(B, M, ids, arrays, skip)
            if ids.dtype != torch.int32:
                raise ValueError(f"screen_markers: ids must be int32, got {ids.dtype}")
            arrs = [x for x, _, _, _ in arrays]
            dt = torch.float32 if self.dtype == 32 else torch.float64
            out = (ids if inplace else torch.empty((B, M), dtype=torch.int32, device=ids.device),
                   torch.empty((B, M), dtype=dt, device=ids.device), torch.empty((B, M), dtype=torch.int32, device=ids.device),
                   torch.empty(B, dtype=torch.int32, device=ids.device))
            self._keep += list(out)
            cur = self._order_in(ids, *arrs, skip)
        else:
            transport = ""
            if inplace and not (isinstance(ids, np.ndarray) and ids.dtype == np.int32 and ids.flags.c_contiguous):
                raise ValueError("screen_markers: inplace needs a contiguous int32 array")
            ids = np.ascontiguousarray(ids, np.int32).reshape(B, -1)
            M = ids.shape[1]
            arrs = [None if (x is None and optional) else self._host(x, (B, M, w)) for x, w, _, optional in arrays]
            skip = None if skip is None else self._host(skip, (B,), np.uint8)
            out = (ids if inplace else np.empty((B, M), np.int32), np.empty((B, M), self.np_dtype), np.empty((B, M), np.int32),
                   np.empty(B, np.int32))
        name = "screen_markers" + transport
        rc = getattr(self._lib, "fbus_ekf_" + name)(self._h, int(kind), M, self._p(ids), *[self._p(x) for x in arrs], int(geometry),
                                                    self._p(skip), *[self._p(o) for o in out])
        self._check(rc, name)
        self._order_out(cur)
        return out

    # ---- predicted corner pixels with their innovation covariance (include/fbus_ekf.h: fbus_ekf_project_markers) -----------------
    def project_markers(self, ids, cameras=2, skip=None, cov=True):
        """Where the four corners of every listed marker appear in the left (cameras=1) or in both images (2) given each filter's
        state -- the h(x) of correct_pixels as an output --, which of them are in view, and the innovation covariance
        S = H P_JJ H' + r_pix I of every projection (r_pix: the filter's own row when a noise table is set).  ids: (B, M) int32, -1
        or an id outside the map = absent.  Returns (left, right, view, cov_left, cov_right): left, right (B, M, 8) in the record
        type, x0 y0 .. x3 y3 -- the arrays correct_pixels takes --, view (B, M) uint8 (bit k: left corner k in view, bit 4 + k: right
        corner k), cov_* (B, M, 4, 3) float64 = (S_uu, S_uv, S_vv) per corner; right and cov_right are None for cameras=1, both
        cov_* for cov=False.  A projection out of view, a slot that is absent and a skipped filter (skip: (B,) uint8) give zeros and
        clear bits.  numpy arrays for host inputs, device tensors (stream-ordered, capturable) for device inputs.  Read-only: no
        record, flag or likelihood sum changes.  gating.search_window turns cov_* into a search box."""
        B = self.B
        if cameras not in (1, 2):
            raise ValueError(f"project_markers: cameras = {cameras} is neither 1 (left) nor 2 (stereo)")
        stereo, cur = cameras == 2, None
        if _is_dev(ids):
            import torch
            transport, M = "_dev", ids.numel() // B
            self._rows_checked(B, M, ids, (), skip)
            if ids.dtype != torch.int32:
                raise ValueError(f"project_markers: ids must be int32, got {ids.dtype}")
            dt = torch.float32 if self.dtype == 32 else torch.float64
            new = lambda shape, t: torch.empty(shape, dtype=t, device=ids.device)
            u8, f64 = torch.uint8, torch.float64
            cur = self._order_in(ids, skip)
        else:
            transport = ""
            ids = np.ascontiguousarray(ids, np.int32).reshape(B, -1)
            M = ids.shape[1]
            skip = None if skip is None else self._host(skip, (B,), np.uint8)
            dt, u8, f64 = self.np_dtype, np.uint8, np.float64
            new = lambda shape, t: np.empty(shape, t)
        left, view = new((B, M, 8), dt), new((B, M), u8)
        right = new((B, M, 8), dt) if stereo else None
        cov_left = new((B, M, 4, 3), f64) if cov else None
        cov_right = new((B, M, 4, 3), f64) if cov and stereo else None
        if transport:
            self._keep += [o for o in (left, right, view, cov_left, cov_right) if o is not None]
        name = "project_markers" + transport
        rc = getattr(self._lib, "fbus_ekf_" + name)(self._h, M, self._p(ids), int(cameras), self._p(skip), self._p(left), self._p(right),
                                                    self._p(cov_left), self._p(cov_right), self._p(view))
        self._check(rc, name)
        self._order_out(cur)
        return left, right, view, cov_left, cov_right

    # ---- consistency against a truth state (include/fbus_ekf.h: fbus_ekf_nees) ----------------------------------------------
    def nees(self, truth, skip=None, err=False, lnp=False):
        """The normalised estimation error squared of every filter against `truth`, (B, 19) float64 in get_state()'s order
        (p v q ba bg g; g ignored for nstate 15): with delta = truth (-) estimate, nees[:, c] = delta_J' P_JJ^-1 delta_J for the
        capi.NEES_COLS blocks NEES_FULL (all N states), NEES_POSE (p and theta) and the 3 x 3 marginals NEES_P .. NEES_G, in double
        for both record types.  err=True also returns delta, (B, N) in the order p v theta ba bg [g]; lnp=True the log-density of
        the truth under N(estimate, P), -1/2 (nees_FULL + ln det P + N ln 2 pi).  A torch device tensor takes the stream-ordered,
        capturable device form and returns device tensors; a numpy array is staged.  skip: (B,) uint8, nonzero = zeros in every
        output.  A column is NaN when one of its delta components is not finite or its block is not positive definite; no other
        column and no other filter is touched.  Read-only: no record, flag or likelihood sum changes.  fbus_ekf.consistency
        has the chi-square bounds for the column means.  Returns nees, or (nees[, err][, lnp])."""
        B, N = self.B, self.N
        if tuple(getattr(truth, "shape", ())) != (B, 19):
            raise ValueError(f"nees: truth must be ({B}, 19), got {tuple(getattr(truth, 'shape', ()))}")
        res = tuple(o for o in self._report_call("nees", (), [("truth", truth, (B, 19), np.float64), ("skip", skip, (B,), np.uint8)],
                                                 [((B, capi.NEES_COLS), np.float64, True), ((B, N), np.float64, err),
                                                  ((B,), np.float64, lnp)]) if o is not None)
        return res[0] if len(res) == 1 else res

    # ---- draws from every filter's own Gaussian (include/fbus_ekf.h: fbus_ekf_sample) --------------------------------------------
    def sample(self, xi, skip=None, drawn=False):
        """S states per filter drawn from N(estimate, P) on the device -- the inverse of nees(): xi, (S, B, N) float64, holds the
        standard-normal (or sigma-point: consistency.sigma_points) coordinates of the draws in the FACTORISATION order p theta v ba bg
        [g]; with L L' = the covariance in that order, delta = L xi in error-state order is injected into the nominal state in double
        (plain sums, q (x) Exp(delta_theta) normalised).  Returns state, (S, B, 19) float64 in get_state()'s order: state[s] is a
        ready truth for nees() -- which then returns FULL = |xi|^2, POSE = |xi[:6]|^2, P = |xi[:3]|^2 and err = delta -- or, cast, a
        nominal for set_state().  drawn=True also returns (B,) uint8: 0 for a filter that is skipped (skip: (B,) uint8) or whose
        covariance is not positive definite; every row of such a filter is its own nominal state.  A torch device tensor takes the
        stream-ordered, capturable device form and returns device tensors; a numpy array is staged.  S is at most capi.SAMPLE_MAX.
        Read-only: no record, flag or likelihood sum changes.  Returns state, or (state, drawn)."""
        B, N = self.B, self.N
        shape = tuple(getattr(xi, "shape", ()))
        if len(shape) != 3 or shape[1:] != (B, N) or not 1 <= shape[0] <= capi.SAMPLE_MAX:
            raise ValueError(f"sample: xi must be (S, {B}, {N}) with S in 1..{capi.SAMPLE_MAX}, got {shape}")
        S = shape[0]
        out = self._report_call("sample", (S,), [("xi", xi, (S, B, N), np.float64), ("skip", skip, (B,), np.uint8)],
                                [((S, B, 19), np.float64, True), ((B,), np.uint8, drawn)])
        return out if drawn else out[0]

    def perturb(self, xi, skip=None):
        """Moves every filter to ONE draw from its own N(estimate, P): xi (B, N) float64 device tensor, as one row of sample().  A
        composition, not a kernel: sample() with S = 1, the row cast to the record type, the rotation matrix of the new unit quaternion
        formed in float64 and rounded once, and set_state(nominal, rot) -- on the device -- for the filters that were drawn; the others
        keep their state, and every covariance, prev_id and flag stays as it is.  The rotation is written on purpose: an in-place
        perturb that left the CARRIED rotation behind would make the pose and pixel rows linearise at the old attitude until the next
        predict.  Returns drawn, (B,) uint8 on the device."""
        import torch
        if not _is_dev(xi) or tuple(xi.shape) != (self.B, self.N):
            raise ValueError(f"perturb: xi must be a ({self.B}, {self.N}) device tensor")
        state, drawn = self.sample(xi.reshape(1, self.B, self.N), skip, drawn=True)
        with torch.cuda.device(xi.device):
            old_nom, old_rot = self.get_state_dev()
            tt = old_nom.dtype
            nom = state[0].to(tt)
            w, x, y, z = nom[:, 6:10].to(torch.float64).unbind(1)      # the quaternion the record will hold
            n2 = w * w + x * x + y * y + z * z
            w, x, y, z = (c / torch.sqrt(n2) for c in (w, x, y, z))
            rot = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                               2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                               2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).to(tt)
            keep = (drawn == 0)[:, None]
            nom = torch.where(keep, old_nom, nom).contiguous()
            rot = torch.where(keep, old_rot, rot).contiguous()
        self._keep += [nom, rot]
        self.set_state(nom, rot, None, None)
        return drawn

    def applied(self):
        out = np.empty(self.B, np.uint8)
        self._check(self._lib.fbus_ekf_get_applied(self._h, self._p(out)), "get_applied")
        return out

    def _frame_call(self, name, head, imu, pre, M, ids, arrays, tail, skip, n, record=None):
        """One frame or window through fbus_ekf_<name>: head (K, or F and kcount), the IMU arrays and per, the int arguments in front of M,
        M, ids and `arrays` (checked as n filter-frames), the int arguments behind them, skip; record: the number of frames whose
        trajectory rows are wanted (and returned), or None"""
        if M > 0:
            self._rows_checked(n, M, ids, arrays, None)
        if skip is not None:
            self._dev_checked(skip, n, "skip")
        accel, gyro, dt, per = imu
        arrs = [a for a, _, _, _ in arrays]
        out = self._traj_outputs(record) if record is not None else ()
        cur = self._order_in(accel, gyro, dt, ids, *arrs, skip, *out)
        rc = getattr(self._lib, "fbus_ekf_" + name)(self._h, *head, self._p(accel), self._p(gyro), self._p(dt), per, *pre, M,
                                                    self._p(ids), *[self._p(a) for a in arrs], *tail, self._p(skip),
                                                    *[self._p(o) for o in out])
        self._check(rc, name)
        self._order_out(cur)
        return out if record is not None else None

    def _window(self, kcount, accel, gyro, dt, ids):
        """(kcount as int32, its pointer, F, M, per) of a window call, the IMU arrays checked"""
        kcount = np.ascontiguousarray(kcount, np.int32)
        F, Kt = int(kcount.size), int(kcount.sum())
        if F > capi.MAX_WINDOW_FRAMES:
            raise ValueError(f"at most {capi.MAX_WINDOW_FRAMES} frames per window")
        M = ids.numel() // (self.B * F) if (ids is not None and F > 0) else 0
        _, per = self._imu(accel, gyro, dt, Kt, "sum(kcount)")
        return kcount, kcount.ctypes.data_as(C.POINTER(C.c_int32)), F, M, per

    def frame(self, accel, gyro, dt, ids, pos, quat, mode=capi.MODE_NEAREST, skip=None, fused=False):
        """K per-sample predict launches followed by one correct launch (device arrays only);
        fused=True: the same frame as ONE launch with the records resident in registers."""
        K, per = self._imu(accel, gyro, dt)
        M = ids.numel() // self.B if ids is not None else 0
        self._frame_call("frame_fused_dev" if fused else "frame_dev", (K,), (accel, gyro, dt, per), (), M, ids,
                         self._pose_arrays(pos, quat), (mode,), skip, self.B)

    def frame_meas(self, accel, gyro, dt, ids, left, right=None, kind=capi.MEAS_PIXELS, geometry=capi.VIS_REFRACTIVE,
                   mode=capi.MODE_STACKED, skip=None):
        """One camera frame with the north star's MeasureUpdate in ONE launch (fbus_ekf_frame_meas_fused_dev; device arrays):
        K predicts, then correct_pixels (kind = MEAS_PIXELS; right=None: left camera) or correct_corners (MEAS_CORNERS, with its
        geometry / mode).  accel, gyro: (K, B, 3); dt: (K,) or (K, B); ids: (B, M); left / right: (B, M, 8) [(B, M, 12) corner
        positions for VIS_CORNERS3D]."""
        K, per = self._imu(accel, gyro, dt)
        M = ids.numel() // self.B if ids is not None else 0
        self._frame_call("frame_meas_fused_dev", (K,), (accel, gyro, dt, per), (kind,), M, ids,
                         self._image_arrays(left, right, kind, geometry), (geometry, mode), skip, self.B)

    def frames_meas(self, kcount, accel, gyro, dt, ids, left, right=None, kind=capi.MEAS_PIXELS, geometry=capi.VIS_REFRACTIVE,
                    mode=capi.MODE_STACKED, skip=None, record=False):
        """A window of camera frames with the north star's MeasureUpdate in ONE launch (fbus_ekf_frames_meas_fused_dev; device arrays):
        len(kcount) times { kcount[f] predicts, correct_pixels / correct_corners }.  accel, gyro: (sum kcount, B, 3); dt: (sum kcount,) or
        (sum kcount, B); ids: (F, B, M); left / right: (F, B, M, 8) [(F, B, M, 12) for VIS_CORNERS3D]; skip: (F, B) or None.
        record=True: the window's trajectory as well (fbus_ekf_frames_meas_fused_traj_dev) -- returns (nominal (F, B, 19), pdiag (F, B, N),
        applied (F, B)), torch tensors on the handle's device: the state after every frame (FBUS_EKF.m:201-204)."""
        kcount, kp, F, M, per = self._window(kcount, accel, gyro, dt, ids)
        return self._frame_call("frames_meas_fused_traj_dev" if record else "frames_meas_fused_dev", (F, kp), (accel, gyro, dt, per), (kind,), M,
                                ids, self._image_arrays(left, right, kind, geometry), (geometry, mode), skip, F * self.B, F if record else None)

    def frames(self, kcount, accel, gyro, dt, ids, pos, quat, mode=capi.MODE_NEAREST, skip=None, record=False):
        """A window of camera frames in ONE launch (device arrays): len(kcount) times { kcount[f] predicts, one correct }
        with the records resident in registers in between -- the frame loop of FBUS_EKF.m:151-210 over a recorded stretch.
        accel, gyro: (sum kcount, B, 3); dt: (sum kcount,) or (sum kcount, B); ids: (F, B, M); pos: (F, B, M, 3);
        quat: (F, B, M, 4); skip: (F, B) or None.  applied() afterwards reports the last frame.
        record=True: the window's trajectory as well (fbus_ekf_frames_fused_traj_dev) -- returns (nominal (F, B, 19), pdiag (F, B, N),
        applied (F, B)), torch tensors on the handle's device: the state after every frame (FBUS_EKF.m:201-204)."""
        kcount, kp, F, M, per = self._window(kcount, accel, gyro, dt, ids)
        return self._frame_call("frames_fused_traj_dev" if record else "frames_fused_dev", (F, kp), (accel, gyro, dt, per), (), M, ids,
                                self._pose_arrays(pos, quat), (mode,), skip, F * self.B, F if record else None)

    def _traj_outputs(self, F):
        """(nominal (F, B, 19), pdiag (F, B, N), applied (F, B)) on the handle's device, kept alive until the next sync()"""
        import torch
        dev = torch.device("cuda", self.device)
        tt = torch.float32 if self.dtype == 32 else torch.float64
        out = (torch.empty((F, self.B, 19), dtype=tt, device=dev), torch.empty((F, self.B, self.N), dtype=tt, device=dev),
               torch.empty((F, self.B), dtype=torch.uint8, device=dev))
        self._keep.extend(out)
        return out

    def snapshot(self):
        """The pose and its sigma of every filter without the full covariance (fbus_ekf_snapshot_dev): (nominal (B, 19), pdiag (B, N),
        applied (B,)), torch tensors on the handle's device -- equal to get_state()'s nominal and diag(P) and to applied(), bit for bit."""
        nominal, pdiag, applied = (o[0] for o in self._traj_outputs(1))
        cur = self._order_in(nominal, pdiag, applied)
        self._check(self._lib.fbus_ekf_snapshot_dev(self._h, self._p(nominal), self._p(pdiag), self._p(applied)), "snapshot_dev")
        self._order_out(cur)
        return nominal, pdiag, applied

    # ---- init / reset / front door (host arrays) --------------------------------------------
    def init_gravity_bias(self, accel, gyro):
        """InitGravityAndGyrobias.m:36-40: accel, gyro (T, B, 3) -> g, bg of every filter."""
        accel = np.ascontiguousarray(accel, self.np_dtype)
        T = accel.size // (3 * self.B)
        gyro = self._host(gyro, (T, self.B, 3))
        self._check(self._lib.fbus_ekf_init_gravity_bias(self._h, T, self._p(accel), self._p(gyro)), "init_gravity_bias")

    def pose_init(self, ids, pos, quat, what=capi.POSE_INIT, mask=None):
        """InitPositionAndQuaternion.m / ResetState.m (what = POSE_INIT / POSE_RESET) from the nearest marker;
        returns the per-filter applied flags."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(self.B, -1)
        M = ids.shape[1]
        pos = self._host(pos, (self.B, M, 3)); quat = self._host(quat, (self.B, M, 4))
        mask = None if mask is None else self._host(mask, (self.B,), np.uint8)
        rc = self._lib.fbus_ekf_pose_init(self._h, M, self._p(ids), self._p(pos), self._p(quat), what, self._p(mask))
        self._check(rc, "pose_init")
        return self.applied()                      # 0 where nothing happened (no marker in range / in the map / masked)

    def vision_only_pose(self, ids, pos, quat):
        """ComputeVisionOnlyResults.m:39-79 -> (B, 7) [p3, q4]; the state is not touched."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(self.B, -1)
        M = ids.shape[1]
        pos = self._host(pos, (self.B, M, 3)); quat = self._host(quat, (self.B, M, 4))
        out = np.zeros((self.B, 7), self.np_dtype)
        rc = self._lib.fbus_ekf_vision_only_pose(self._h, M, self._p(ids), self._p(pos), self._p(quat), self._p(out))
        self._check(rc, "vision_only_pose")
        return out

    def imu_ema(self, accel, gyro, restart=False):
        """IMU pre-filter of FILTER::SetImuData (filter.cpp:36-47); returns filtered copies (T, B, 3)."""
        accel = np.array(accel, self.np_dtype, order="C", copy=True)
        gyro = np.array(gyro, self.np_dtype, order="C", copy=True)
        T = accel.size // (3 * self.B)
        rc = self._lib.fbus_ekf_imu_ema(self._h, T, self._p(accel), self._p(gyro), 1 if restart else 0)
        self._check(rc, "imu_ema")
        return accel.reshape(T, self.B, 3), gyro.reshape(T, self.B, 3)

    # ---- marker pose from stereo corners (vision.cpp:472-759) ---------------------------
    def marker_pose(self, left, right=None, geometry=capi.VIS_REFRACTIVE, want_corners=False):
        """left/right: (n, 8) normalised corner coordinates (or left = (n, 12) 3-D corners with
        geometry VIS_CORNERS3D).  Host arrays in -> (pos (n,3), quat (n,4)[, corners (n,4,3)]) host arrays out;
        device arrays in -> device arrays of the same kind out (torch)."""
        w = 12 if geometry == capi.VIS_CORNERS3D else 8
        if _is_dev(left):
            import torch
            n = left.numel() // w
            pos = torch.empty((n, 3), dtype=left.dtype, device=left.device)
            quat = torch.empty((n, 4), dtype=left.dtype, device=left.device)
            c3 = torch.empty((n, 4, 3), dtype=left.dtype, device=left.device) if want_corners else None
            self._keep += [left, right, pos, quat, c3]
            cur = self._order_in(left, right)       # inputs come from / outputs go to torch's stream: order both ways
            rc = self._lib.fbus_ekf_marker_pose_dev(self._h, n, geometry, self._p(left), self._p(right),
                                                    self._p(pos), self._p(quat), self._p(c3))
            self._check(rc, "marker_pose_dev")
            self._order_out(cur)
            return (pos, quat, c3) if want_corners else (pos, quat)
        left = np.ascontiguousarray(left, self.np_dtype).reshape(-1, w)
        n = left.shape[0]
        right = None if right is None else self._host(right, (n, 8))
        pos = np.empty((n, 3), self.np_dtype)
        quat = np.empty((n, 4), self.np_dtype)
        c3 = np.empty((n, 4, 3), self.np_dtype) if want_corners else None
        rc = self._lib.fbus_ekf_marker_pose(self._h, n, geometry, self._p(left), self._p(right), self._p(pos),
                                            self._p(quat), self._p(c3))
        self._check(rc, "marker_pose")
        return (pos, quat, c3) if want_corners else (pos, quat)

    # ---- L0 helpers one by one (unit-test hook) -------------------------------------------
    def l0_eval(self, op, a, b=None):
        """one of the device inline helpers (capi.L0_*) on n rows of host input; see include/fbus_ekf.h"""
        wa, wb, wo = (4, 4, 4, 4, 3, 3, 1)[op], (4, 0, 0, 0, 1, 0, 0)[op], (4, 9, 9, 4, 9, 4, 4)[op]
        a = np.ascontiguousarray(a, self.np_dtype).reshape(-1, wa)
        n = a.shape[0]
        b = None if not wb else self._host(b, (n, wb))
        out = np.empty((n, wo), self.np_dtype)
        self._check(self._lib.fbus_ekf_l0_eval(self._h, op, n, self._p(a), self._p(b), self._p(out)), "l0_eval")
        return out

    # ---- HIP graphs ------------------------------------------------------------------------
    def graph_capture(self, fn):
        """Runs fn() (device-array calls on this filter only) under stream capture; returns a graph id."""
        self._check(self._lib.fbus_ekf_graph_begin(self._h), "graph_begin")
        self._capturing = True          # no cross-stream markers inside a capture: the caller orders the graph launch
        try:
            fn()
        finally:
            self._capturing = False
            gid = C.c_int(-1)
            rc = self._lib.fbus_ekf_graph_end(self._h, C.byref(gid))
        self._check(rc, "graph_end")
        self._graph_keep = getattr(self, "_graph_keep", []) + list(self._keep)   # captured pointers must stay alive
        return gid.value

    def graph_launch(self, gid):
        self._check(self._lib.fbus_ekf_graph_launch(self._h, gid), "graph_launch")

    # ---- timing -------------------------------------------------------------------------
    def timing_enable(self, on=True, stride=1):
        """stride: frame() brackets only every stride-th frame with HIP events"""
        self._check(self._lib.fbus_ekf_timing_enable(self._h, int(stride) if on else 0), "timing_enable")

    def timing_reset(self):
        self._check(self._lib.fbus_ekf_timing_reset(self._h), "timing_reset")

    def timing_read(self, kernel):
        ms, n = C.c_double(), C.c_int64()
        self._check(self._lib.fbus_ekf_timing_read(self._h, kernel, C.byref(ms), C.byref(n)), "timing_read")
        return ms.value, n.value
