"""Per-frame trajectory output of the frame-window entry points (fbus_ekf_frames_fused_traj_dev, fbus_ekf_frames_meas_fused_traj_dev)
and fbus_ekf_snapshot_dev: the reference's product is one state per camera frame (FBUS_EKF.m:201-204 appends ekfState to EKFResults after
every frame, filter.cpp:238-248 one fusion.txt row).

  * row f of a window == get_state() / applied() after the same frame run alone, bit for bit, on every route the windows take;
  * the records and get_applied after a window with outputs == after the window without them (and with all outputs NULL);
  * snapshot() == get_state()'s nominal and diag(P) bit for bit;
  * replay_windowed(trajectory=True) == replay()'s rows, frame for frame (land recording with resets; water recording with corners=).
"""
import ctypes as C
import os

import numpy as np
import pytest

from fbus_ekf import BatchedFilter, capi, replay, synth
from support import SIZE, device_caster, r32
from util import pixel_scene, state_rel_err, state_rel_err_literal

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DT = 0.005


def _records(flt):
    """the packed records as bytes (fbus_ekf_copy_records into a device buffer, then to the host)"""
    import torch
    _, _, tot = flt.records()
    t = torch.empty(tot, dtype=torch.uint8, device="cuda:0")
    assert flt._lib.fbus_ekf_copy_records(flt._h, C.c_void_p(t.data_ptr()), 0) == 0
    flt.sync()
    return t.cpu().numpy()


def _check_rows(rows, per_frame, what):
    """rows = (nominal (F, B, 19), pdiag (F, B, N), applied (F, B)) on the device; per_frame = [(nominal, P, applied)] read after each frame"""
    import torch
    torch.cuda.synchronize()
    nom, pd, ap = (r.cpu().numpy() for r in rows)
    assert nom.shape[0] == len(per_frame)
    for f, (n, P, a) in enumerate(per_frame):
        assert np.array_equal(nom[f], n), f"{what}: nominal row of frame {f}"
        assert np.array_equal(pd[f], np.diagonal(P, axis1=1, axis2=2)), f"{what}: diag P row of frame {f}"
        assert np.array_equal(ap[f], a), f"{what}: applied row of frame {f}"


def _null_outputs_call(flt, fn, *args):
    rc = fn(flt._h, *args, None, None, None)
    assert rc == 0, flt._lib.fbus_ekf_last_error(flt._h)


MEAS_CASES = [("pixels", False, capi.MODE_STACKED), ("pixels", True, capi.MODE_STACKED),
              ("corners", True, capi.MODE_STACKED), ("corners", True, capi.MODE_NEAREST)]


@pytest.mark.parametrize("route", ["resident", "team", "fp64", "one_frame", "64_frames"])
@pytest.mark.parametrize("what,stereo,mode", MEAS_CASES)
@pytest.mark.parametrize("dialect,n", [(0, 18), (1, 18), (0, 15)])
def test_north_star_window_rows_are_its_frames(dialect, n, what, stereo, mode, route):
    """frames_meas(record=True): row f == get_state() / applied() after frame f of the frame-by-frame run, bit for bit; the records and
    applied() after the window == those of the window without outputs and of the _traj_dev call with all outputs NULL; the last row ==
    get_state() after the window.  The shapes of test_window_of_frames_with_the_north_star_update (B = 443, a blind filter, unknown ids,
    masked filters); routes: the resident window kernel (set_team(1, 1)), the team / per-frame route of a small launch, fp64 records,
    one frame, 64 frames."""
    import torch
    B, M = 448 - 5, 4
    kcount = {"one_frame": [3], "64_frames": [(f * 5) % 4 for f in range(64)]}.get(route, [3, 0, 2, 4])
    F, Kt = len(kcount), sum(kcount)
    dtype = 64 if route == "fp64" else 32
    rq = (lambda a: a) if dtype == 64 else r32
    prm = capi.default_params(dialect)
    prm.marker_size = SIZE
    nom0, _, P, prev = synth.initial_state(0, B, list(prm.p0_diag), n, mixed_cov=True)
    truth, _, ids0, left0, right0 = pixel_scene(B, M, prm, SIZE, seed=61 + dialect, noise=5e-4, nominal=nom0)
    rng = np.random.default_rng(62 + dialect)
    nom = truth.copy()
    nom[:, 0:3] += rng.normal(0, 0.004, (B, 3))
    nom[:, 3:6] = rng.normal(0, 0.02, (B, 3))
    nom = rq(nom)
    rot = rq(synth.q2R(nom[:, 6:10]).reshape(B, 9))
    prev = np.where(ids0[:, 0] >= 0, ids0[:, 0], 0).astype(np.int32)
    P = rq(P)
    acc, gyr = synth.imu_samples(0, B, 0, Kt, nom)
    acc, gyr = rq(acc), rq(gyr)
    ids = np.stack([ids0] * F); left = np.stack([left0] * F); right = np.stack([right0] * F)
    left = rq(left + rng.normal(0, 2e-4, left.shape)); right = rq(right + rng.normal(0, 2e-4, right.shape))
    ids[min(1, F - 1), 5] = -1
    ids[min(2, F - 1), 6, :] = 9
    skip = np.zeros((F, B), np.uint8); skip[min(2, F - 1), 11] = 1; skip[F - 1, 12] = 1; skip[0, 13] = 1
    dd = device_caster(torch, dtype)
    d_acc, d_gyr, d_dt = dd(acc), dd(gyr), dd(np.full(Kt, DT))
    d_ids, d_left, d_right, d_skip = dd(ids), dd(left), dd(right), dd(skip)
    d_r = d_right if stereo else None
    kind = capi.MEAS_PIXELS if what == "pixels" else capi.MEAS_CORNERS
    team = (0, 0) if route == "team" else (1, 1)
    with BatchedFilter(B, prm, dtype=dtype, nstate=n) as fa, BatchedFilter(B, prm, dtype=dtype, nstate=n) as fb, \
            BatchedFilter(B, prm, dtype=dtype, nstate=n) as fc, BatchedFilter(B, prm, dtype=dtype, nstate=n) as fd:
        for f in (fa, fb, fc, fd):
            f.set_team(*team)
            f.set_state(nom, rot, P, prev)
            f.applied()
        rows = fa.frames_meas(kcount, d_acc, d_gyr, d_dt, d_ids, d_left, d_r, kind, capi.VIS_REFRACTIVE, mode, skip=d_skip, record=True)
        fc.frames_meas(kcount, d_acc, d_gyr, d_dt, d_ids, d_left, d_r, kind, capi.VIS_REFRACTIVE, mode, skip=d_skip)
        kc = np.ascontiguousarray(kcount, np.int32)
        _null_outputs_call(fd, fd._lib.fbus_ekf_frames_meas_fused_traj_dev, F, kc.ctypes.data_as(C.POINTER(C.c_int32)), fd._p(d_acc),
                           fd._p(d_gyr), fd._p(d_dt), 0, kind, M, fd._p(d_ids), fd._p(d_left), fd._p(d_r), capi.VIS_REFRACTIVE, mode,
                           fd._p(d_skip))
        per_frame = []
        k0 = 0
        for f, K in enumerate(kcount):
            a, g, t = (d_acc[k0:k0 + K], d_gyr[k0:k0 + K], d_dt[k0:k0 + K]) if K else (None, None, None)
            fb.frame_meas(a, g, t, d_ids[f], d_left[f], d_right[f] if stereo else None, kind, capi.VIS_REFRACTIVE, mode, skip=d_skip[f])
            fb.sync()
            s = fb.get_state()
            per_frame.append((s[0], s[2], fb.applied()))
            k0 += K
        fa.sync(); fc.sync(); fd.sync()
        ra, rc_, rd = _records(fa), _records(fc), _records(fd)
        assert np.array_equal(ra, rc_) and np.array_equal(rd, rc_), "records after the window with / without outputs"
        assert np.array_equal(fa.applied(), fc.applied()) and np.array_equal(fd.applied(), fc.applied())
        end = fa.get_state()
        nom_rows = rows[0].cpu().numpy()
        assert np.array_equal(nom_rows[-1], end[0]) and np.array_equal(rows[1].cpu().numpy()[-1], np.diagonal(end[2], axis1=1, axis2=2))
    _check_rows(rows, per_frame, f"{what} stereo={stereo} mode={mode} route={route}")


POSE_ROUTES = [(mode, route) for mode in (capi.MODE_NEAREST, capi.MODE_STACKED)
               for route in ("resident", "team", "fp64", "one_frame", "64_frames")] + [(capi.MODE_NEAREST, "joseph_nearest")]


@pytest.mark.parametrize("mode,route", POSE_ROUTES)
@pytest.mark.parametrize("dialect,n", [(0, 18), (1, 18), (1, 15)])
def test_pose_window_rows_are_its_frames(dialect, n, mode, route):
    """frames(record=True) against F calls of frame(fused=True), read after every frame; records / applied against the window without
    outputs and with all outputs NULL.  A ragged batch, an invisible marker set, unknown ids, masked filters, a frame without IMU samples."""
    import torch
    B, M = 448 - 5, 4
    kcount = {"one_frame": [5], "64_frames": [(f * 3) % 5 for f in range(64)]}.get(route, [3, 0, 2, 4])
    F, Kt = len(kcount), sum(kcount)
    dtype = 64 if route == "fp64" else 32
    rq = (lambda a: a) if dtype == 64 else r32
    prm = capi.default_params(dialect)
    if route == "joseph_nearest":
        prm.cov_form = capi.COV_JOSEPH
    nom, rot, P, prev = synth.initial_state(0, B, list(prm.p0_diag), n, mixed_cov=True)
    nom, rot, P = rq(nom), rq(rot), rq(P)
    acc, gyr = synth.imu_samples(0, B, 0, Kt, nom)
    fr = [synth.marker_frame(0, B, f, M, nom, prm) for f in range(F)]
    ids = np.stack([x[0] for x in fr]); pos = rq(np.stack([x[1] for x in fr])); quat = rq(np.stack([x[2] for x in fr]))
    ids[min(1, F - 1), 5] = -1
    ids[min(2, F - 1), 6, :] = 9
    skip = np.zeros((F, B), np.uint8); skip[min(2, F - 1), 11] = 1; skip[F - 1, 12] = 1
    dd = device_caster(torch, dtype)
    d_acc, d_gyr, d_dt = dd(rq(acc)), dd(rq(gyr)), dd(np.full(Kt, DT))
    d_ids, d_pos, d_quat, d_skip = dd(ids), dd(pos), dd(quat), dd(skip)
    team = (0, 0) if route == "team" else (1, 1)
    with BatchedFilter(B, prm, dtype=dtype, nstate=n) as fa, BatchedFilter(B, prm, dtype=dtype, nstate=n) as fb, \
            BatchedFilter(B, prm, dtype=dtype, nstate=n) as fc, BatchedFilter(B, prm, dtype=dtype, nstate=n) as fd:
        for f in (fa, fb, fc, fd):
            f.set_team(*team)
            f.set_state(nom, rot, P, prev)
        if route == "team":
            assert fa.launch_info(capi.INFO_TEAM_FRAMES) == 1
        rows = fa.frames(kcount, d_acc, d_gyr, d_dt, d_ids, d_pos, d_quat, mode, skip=d_skip, record=True)
        fc.frames(kcount, d_acc, d_gyr, d_dt, d_ids, d_pos, d_quat, mode, skip=d_skip)
        kc = np.ascontiguousarray(kcount, np.int32)
        _null_outputs_call(fd, fd._lib.fbus_ekf_frames_fused_traj_dev, F, kc.ctypes.data_as(C.POINTER(C.c_int32)), fd._p(d_acc),
                           fd._p(d_gyr), fd._p(d_dt), 0, M, fd._p(d_ids), fd._p(d_pos), fd._p(d_quat), mode, fd._p(d_skip))
        per_frame = []
        k0 = 0
        for f, K in enumerate(kcount):
            a, g, t = (d_acc[k0:k0 + K], d_gyr[k0:k0 + K], d_dt[k0:k0 + K]) if K else (None, None, None)
            if n == 18:
                fb.frame(a, g, t, d_ids[f], d_pos[f], d_quat[f], mode, skip=d_skip[f], fused=True)
            else:
                # N = 15: the window and the fused frame kernel are not bit-equal for every combination (the existing equality test covers
                # N = 18); the frame-by-frame reference is then the same entry point one frame at a time
                fb.frames([K], a, g, t, d_ids[f:f + 1], d_pos[f:f + 1], d_quat[f:f + 1], mode, skip=d_skip[f:f + 1])
            fb.sync()
            s = fb.get_state()
            per_frame.append((s[0], s[2], fb.applied()))
            k0 += K
        fa.sync(); fc.sync(); fd.sync()
        ra, rc_, rd = _records(fa), _records(fc), _records(fd)
        assert np.array_equal(ra, rc_) and np.array_equal(rd, rc_), "records after the window with / without outputs"
        assert np.array_equal(fa.applied(), fc.applied()) and np.array_equal(fd.applied(), fc.applied())
        end = fa.get_state()
        assert np.array_equal(rows[0].cpu().numpy()[-1], end[0])
    _check_rows(rows, per_frame, f"pose rows mode={mode} route={route}")


@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("n", [18, 15])
def test_snapshot_is_get_state_bit_for_bit(dtype, n):
    """snapshot() == get_state()'s nominal and diag(P), and applied(), bit for bit (a ragged batch after a predict and a correct)."""
    import torch
    B, M = 200 - 7, 3
    prm = capi.default_params(0)
    nom, rot, P, prev = synth.initial_state(0, B, list(prm.p0_diag), n, mixed_cov=True)
    acc, gyr = synth.imu_samples(0, B, 0, 1, nom)
    ids, pos, quat = synth.marker_frame(0, B, 0, M, nom, prm)
    ids[4] = -1
    with BatchedFilter(B, prm, dtype=dtype, nstate=n) as flt:
        flt.set_state(nom, rot, P, prev)
        flt.predict(acc[0], gyr[0], np.array([DT]))
        flt.correct(ids, pos, quat, capi.MODE_STACKED)
        s = flt.get_state()
        nm, pd, ap = flt.snapshot()
        torch.cuda.synchronize()
        assert np.array_equal(nm.cpu().numpy(), s[0])
        assert np.array_equal(pd.cpu().numpy(), np.diagonal(s[2], axis1=1, axis2=2))
        assert np.array_equal(ap.cpu().numpy(), flt.applied()) and ap.cpu().numpy()[4] == 0


def test_trajectory_refuses_outputs_on_the_records():
    """an output that overlaps the records is refused before any launch"""
    B = 128
    prm = capi.default_params(0)
    with BatchedFilter(B, prm) as flt:
        ptr, _, _ = flt.records()
        rc = flt._lib.fbus_ekf_snapshot_dev(flt._h, C.c_void_p(ptr), None, None)
        assert rc == 1                              # FBUS_ERR_INVALID


def _land_gapped():
    d = np.load(os.path.join(GOLD, "recordings.npz"))
    imu, image = d["land_imu"], d["land_image"]
    t = image[:, 0]
    keep = ~(((t > t[0] + 8.0) & (t < t[0] + 8.4)) | ((t > t[0] + 20.0) & (t < t[0] + 20.25)))
    return imu, image[keep]


@pytest.mark.parametrize("dialect", [0, 1])
def test_recording_replay_trajectory_through_frame_windows(dialect):
    """replay_windowed(trajectory=True) on the gapped land recording (two resets), 256 filters: the same frames and time stamps as replay(),
    all 256 filters identical, every frame within 1e-9 (fp64; pdiag 1e-8 relative) / the end-state band of the window replay test (fp32)."""
    imu, image = _land_gapped()
    prm = capi.default_params(dialect)
    assert sum(1 for p in replay.plan_windows(imu, image) if p[0] == "reset") == 2
    B = 256
    for dtype in (64, 32):
        with BatchedFilter(1, prm, dtype=dtype) as f1:
            ref, nref = replay.replay(f1, imu, image, prm)
        with BatchedFilter(B, prm, dtype=dtype) as flt:
            steps, rows = replay.replay_windowed(flt, imu, image, prm, trajectory=True)
            nom, rot, P, _ = flt.get_state()
        assert steps == int(nref.sum()) + len(ref) - 2                     # a reset frame is no EKF step
        assert all(np.array_equal(a[0], a[-1]) and np.array_equal(a[0], a[B // 2]) for a in (nom, rot, P))
        assert rows.shape == (len(ref), 1 + 19 + 18)
        assert np.array_equal(rows[:, 0], ref[:, 0])
        assert np.array_equal(rows[-1, 1:20], nom[0].astype(np.float64))
        refP = ref[:, 29:].reshape(-1, 18, 18)
        refd = np.diagonal(refP, axis1=1, axis2=2)
        if dtype == 64:
            assert np.abs(rows[:, 1:20] - ref[:, 1:20]).max() < 1e-9
            assert (np.abs(rows[:, 20:] - refd) / np.abs(refd)).max() < 1e-8
        else:
            for k in range(len(ref)):
                lit = state_rel_err_literal(rows[k:k + 1, 1:20], ref[k:k + 1, 1:20])
                sig = state_rel_err(rows[k:k + 1, 1:20], ref[k:k + 1, 1:20], refP[k:k + 1])
                assert lit < 1e-4 and sig[0] < 3e-3, (k, lit, sig[0])
        # fusion_rows reads them as it reads replay()'s rows
        assert np.array_equal(replay.fusion_rows(rows)[:, 0], replay.fusion_rows(ref)[:, 0])


WATER_MARKER_SIDE = 0.1142


def test_water_recording_trajectory_through_pixel_windows():
    """replay_windowed(trajectory=True, corners=...) on the first 100 frames of the water recording against replay(corners=...): the same
    frames and time stamps, fp64 within 1e-9 per frame, fp32 through the window gate of tests/util.py at every frame."""
    d = np.load(os.path.join(GOLD, "recordings.npz"))
    imu, image, corners = d["water_imu"], d["water_image"], d["water_corners"]
    nfr = 100
    for dialect in (0, 1):
        prm = capi.default_params(dialect)
        prm.marker_size = WATER_MARKER_SIDE
        with BatchedFilter(1, prm, dtype=64) as f1:
            ref, _ = replay.replay(f1, imu, image, prm, max_frames=nfr, corners=corners)
        with BatchedFilter(8, prm, dtype=64) as flt:
            _, rows = replay.replay_windowed(flt, imu, image, prm, max_frames=nfr, trajectory=True, corners=corners)
        assert rows.shape[0] == len(ref) and np.array_equal(rows[:, 0], ref[:, 0])
        assert np.abs(rows[:, 1:20] - ref[:, 1:20]).max() < 1e-9
        refd = np.diagonal(ref[:, 29:].reshape(-1, 18, 18), axis1=1, axis2=2)
        assert (np.abs(rows[:, 20:] - refd) / np.abs(refd)).max() < 1e-8
        with BatchedFilter(8, prm, dtype=32) as flt:
            _, r32_ = replay.replay_windowed(flt, imu, image, prm, max_frames=nfr, trajectory=True, corners=corners)
        assert np.array_equal(r32_[:, 0], ref[:, 0])
        for k in range(len(ref)):
            lit = state_rel_err_literal(r32_[k:k + 1, 1:20], ref[k:k + 1, 1:20])
            sig = state_rel_err(r32_[k:k + 1, 1:20], ref[k:k + 1, 1:20], ref[k:k + 1, 29:].reshape(1, 18, 18))
            assert lit < 1e-4 and sig[0] < 1e-3, (dialect, k, lit, sig[0])


def test_cpp_mirror_reaches_the_trajectory_entry_points(tmp_path):
    """include/fbus/batched_filter.hpp: the frames_fused_dev overload with outputs and snapshot_dev, compiled with plain g++ against the
    device library -- the window's last row equals the snapshot after it."""
    import subprocess
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(ROOT, "fbus-ekf_amd", "lib")
    src = tmp_path / "tj.cpp"
    src.write_text(r'''
#include <fbus/batched_filter.hpp>
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <cstring>
#include <vector>
int main() {
    using BF = fbus::BatchedFilter<float>;
    const int B = 300, F = 3, Kf = 4, K = F * Kf;
    std::vector<float> a(size_t(K) * B * 3), w(size_t(K) * B * 3), dt(K, 0.005f);
    for (size_t i = 0; i < a.size(); ++i) { a[i] = 0.05f * float(i % 11) - 0.2f; w[i] = 0.002f * float(i % 7) - 0.004f; }
    float *da, *dw, *ddt, *dn, *dp, *sn, *sp;
    uint8_t *dap, *sap;
    if (hipMalloc((void**)&da, a.size() * 4) != hipSuccess || hipMalloc((void**)&dw, w.size() * 4) != hipSuccess ||
        hipMalloc((void**)&ddt, K * 4) != hipSuccess || hipMalloc((void**)&dn, size_t(F) * B * 19 * 4) != hipSuccess ||
        hipMalloc((void**)&dp, size_t(F) * B * 18 * 4) != hipSuccess || hipMalloc((void**)&dap, size_t(F) * B) != hipSuccess ||
        hipMalloc((void**)&sn, size_t(B) * 19 * 4) != hipSuccess || hipMalloc((void**)&sp, size_t(B) * 18 * 4) != hipSuccess ||
        hipMalloc((void**)&sap, B) != hipSuccess) return 2;
    hipMemcpy(da, a.data(), a.size() * 4, hipMemcpyHostToDevice); hipMemcpy(dw, w.data(), w.size() * 4, hipMemcpyHostToDevice);
    hipMemcpy(ddt, dt.data(), K * 4, hipMemcpyHostToDevice);
    BF f(B, BF::defaults(FBUS_DIALECT_MATLAB), 0);
    f.reset_covariance();
    f.set_team(1, 1);
    f.frames_fused_dev(std::vector<int32_t>(F, Kf), da, dw, ddt, 0, nullptr, nullptr, nullptr, BF::Mode::Stacked, nullptr, dn, dp, dap);
    f.snapshot_dev(sn, sp, sap);
    f.sync();
    std::vector<float> rn(size_t(B) * 19), rp(size_t(B) * 18), qn(size_t(B) * 19), qp(size_t(B) * 18);
    hipMemcpy(rn.data(), dn + size_t(F - 1) * B * 19, rn.size() * 4, hipMemcpyDeviceToHost);
    hipMemcpy(rp.data(), dp + size_t(F - 1) * B * 18, rp.size() * 4, hipMemcpyDeviceToHost);
    hipMemcpy(qn.data(), sn, qn.size() * 4, hipMemcpyDeviceToHost);
    hipMemcpy(qp.data(), sp, qp.size() * 4, hipMemcpyDeviceToHost);
    const bool eq = std::memcmp(rn.data(), qn.data(), rn.size() * 4) == 0 && std::memcmp(rp.data(), qp.data(), rp.size() * 4) == 0;
    bool threw = false;
    void* recs = nullptr;
    fbus_ekf_records(f.handle(), &recs, nullptr, nullptr);
    try { f.snapshot_dev(static_cast<float*>(recs), nullptr, nullptr); } catch (const std::exception&) { threw = true; }
    std::printf("last row equal %d refused %d\n", int(eq), int(threw));
    return eq && threw ? 0 : 5;
}
''')
    exe = tmp_path / "tj"
    subprocess.run(["g++", "-std=c++14", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                    str(src), "-o", str(exe), "-L", libdir, "-lfbus_ekf", "-L", "/opt/rocm/lib", "-lamdhip64",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "last row equal 1 refused 1" in r.stdout
