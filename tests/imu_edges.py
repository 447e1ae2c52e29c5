"""IMU samples at the edges of predict_nominal's domain (fbus-ekf_amd/csrc/ekf_device.hpp): the scene, its fp64 reference and a plain numpy
restatement of one ImuUpdate with switches for wrong variants.  A plain library: no tests, no pytest marks, no GPU.  Used by
tests/test_imu_edges_cpu.py (the scene's own conditions; the gate catches every mutant) and tests/test_imu_edges_gpu.py (every route that
predicts, on this scene).

The scene: B = 193 filters (support.B_IND), K = 7 samples.  Sample k of filter b belongs to class (b + k) % C of CLASSES, so the classes
interleave inside every wave and every filter changes branch from sample to sample.  The gyro sample is bias + rate x a random unit vector,
every input rounded with support.r32.  The filters b % 5 == 0 carry a zero gyro bias: only they can realise a rate whose square is an fp32
denormal (elsewhere bias + 3e-20 rounds to the bias, an exact zero rate).  Two streams share the accelerometer and gyro samples:
  "per"     every filter its own period, the class's (dt_per_filter = 1)
  "shared"  one period per sample, cycling through SHARED_DT (dt_per_filter = 0); the rate still follows the class

The reference is replay_ref.OracleEngine (the C oracle's fbo_predict).  The reference's Matlab dialect divides 0 / 0 at w == 0
(ImuUpdate.m:41-43, axisangle_to_quaternion.m:22-29) and the oracle returns NaN there as the reference does, so for the samples whose
(gyro - bg)^2 sums below 1.2e-38 the Matlab-dialect oracle is given bg + 1e-12 x direction in place of the gyro sample: that moves its
result by 1e-13 at most.  The C++ dialect's oracle needs no substitute (filter.cpp:553-560 is finite at w == 0)."""
import types

import numpy as np

from replay_ref import OracleEngine
from support import B_IND, fp32_record_floor, frozen, imu_of, r32, round_records, state_batch

B, K = B_IND, 7
# (rate |gyro - bg| [rad/s], period [s], what it exercises)
CLASSES = (
    (0.0, 5e-3, "exact zero rate"),
    (3e-20, 5e-3, "square is an fp32 denormal"),
    (3e-5, 5e-3, "below the guard"),
    (0.9e-4, 5e-3, "just below the guard"),
    (1.1e-4, 5e-3, "just above the guard"),
    (0.02, 5e-3, "the common path"),
    (9.9, 0.1, "half-angle 0.495 rad"),
    (10.1, 0.1, "half-angle 0.505 rad"),
    (25.0, 0.1, "half-angle 1.25 rad"),
    (9e-5, 1.0, "small-rate branch over 1 s"),
    (3e-5, 1.0, "small-rate branch over 1 s, slower"),
    (0.0, 1.0, "zero rate over 1 s"),
    (0.02, 0.0, "zero period"),
    (0.0, 0.0, "zero rate and zero period"),
    (0.02, -5e-3, "negative period"),
    (3e-5, -5e-3, "negative period below the guard"),
)
C = len(CLASSES)
# the shared periods.  They were (5e-3, 0.1, 1.0, 0, -5e-3) to begin with.  A shared period is taken by EVERY filter, and over a period h the
# fp32 rounding of the carried rotation (1.2e-7) times 9.8 m/s^2 times h lands in the velocity; the N = 15 filters of the C++ dialect hold
# that against a velocity sigma of 0.1 m/s (no gravity block feeds it), so their fp32-record floor is about 1.2e-5 x h [s] per step:
# measured sigma-aware 2.6e-6 with (0.1, 1.0) and 1.2e-6 .. 1.8e-6 with 0.1 and any third period from 0.02 to 0.25 -- past a tenth of the
# 1e-5 gate.  The classes were shrunk, not the gate: 0.02 s (taken twice) and 0.05 s (once) read 7e-7.  25 rad/s over 0.05 s is a
# half-angle of 0.625 rad, so the shared stream still takes the library sin/cos beside the polynomials.
SHARED_DT = (5e-3, 0.02, 0.05, 0.0, -5e-3)
# One more class that only fp64 records run, on its own (guard_probe): mutant (c) moves the guard of the C++ dialect's small-rate branch, and
# the two branches differ in the third order of the angle -- theta^3 / 12 = 6e-14 rad at 9e-5 rad/s over 1 s, under every gate.  The fp64
# gate (1e-9) needs theta >= 2.3e-3 rad, i.e. more than 25 s below the guard; over such a step fp32 records are far outside a tenth of
# their gates, so the class cannot join the scene above.
GUARD_PROBE = (9e-5, 64.0)
STREAMS = ("per", "shared")
DENORMAL = 1.2e-38                            # (gyro - bg)^2 below this: the Matlab-dialect oracle gets the substitute
MUTANTS = {"a": "identity increment below the guard", "b": "the half increment's 0.25 written as 0.5", "c": "the guard compared against 1e-5",
           "d": "the polynomial sin/cos above 0.5 rad", "e": "the sign of dt dropped from F(theta, theta)",
           "f": "dt == 0 treated as no step for the covariance"}
CPP_ONLY = "abc"                              # the mutants of the C++ dialect's small-rate branch (filter.cpp:553-560)

_SCENES, _REFS = {}, {}


def scene(nstate, dialect):
    """the scene for one (state size, dialect), cached and read-only: prm, state = (nominal, rot, P, prev), acc / gyr (K, B, 3),
    gyr_oracle (gyr, or the substitute where the Matlab dialect needs it), dt = {"per": (K, B), "shared": (K,)}, cls (K, B): the class of
    every sample, w2 (K, B): the squared rate every sample realises"""
    key = (nstate, dialect)
    if key not in _SCENES:
        prm, nom, rot, P, prev = state_batch(B, dialect, nstate)
        nom[np.arange(B) % 5 == 0, 13:16] = 0.0
        acc, _ = imu_of(0, B, 0, K, nom)
        cls = (np.arange(B)[None, :] + np.arange(K)[:, None]) % C
        rate, period = (np.array([c[i] for c in CLASSES])[cls] for i in (0, 1))
        axis = np.random.default_rng(4711).normal(size=(K, B, 3))
        axis /= np.linalg.norm(axis, axis=2, keepdims=True)
        bg = nom[None, :, 13:16]
        gyr = r32(bg + rate[..., None] * axis)
        w2 = ((gyr - bg) ** 2).sum(axis=2)
        gyr_oracle = np.where((w2 < DENORMAL)[..., None], bg + 1e-12 * axis, gyr) if dialect == 0 else gyr
        dt = {"per": r32(period), "shared": r32(np.array([SHARED_DT[k % len(SHARED_DT)] for k in range(K)]))}
        _SCENES[key] = frozen(types.SimpleNamespace(prm=prm, state=(nom, rot, P, prev), acc=acc, gyr=gyr, gyr_oracle=gyr_oracle, dt=dt,
                                                    cls=cls, w2=w2, nstate=nstate, dialect=dialect))
    return _SCENES[key]


def guard_probe(nstate, dialect):
    """ONE sample of GUARD_PROBE for every filter of the scene's initial state, shaped like scene(): for fp64 records only"""
    key = (nstate, dialect, "guard")
    if key not in _SCENES:
        s = scene(nstate, dialect)
        nom = s.state[0]
        axis = np.random.default_rng(4712).normal(size=(1, B, 3))
        axis /= np.linalg.norm(axis, axis=2, keepdims=True)
        gyr = r32(nom[None, :, 13:16] + GUARD_PROBE[0] * axis)
        w2 = ((gyr - nom[None, :, 13:16]) ** 2).sum(axis=2)
        assert (w2 > 1e-5 ** 2).all() and (w2 < 10e-5 ** 2).all()         # (between the mutant's guard and the reference's)
        dt = {"per": np.full((1, B), GUARD_PROBE[1]), "shared": np.full(1, GUARD_PROBE[1])}
        _SCENES[key] = frozen(types.SimpleNamespace(prm=s.prm, state=s.state, acc=s.acc[:1], gyr=gyr, gyr_oracle=gyr, dt=dt,
                                                    cls=np.full((1, B), C), w2=w2, nstate=nstate, dialect=dialect))
    return _SCENES[key]


def period_of(s, stream, k):
    """the period(s) of sample k as predict takes them: (B,) or (1,)"""
    return s.dt[stream][k] if stream == "per" else s.dt[stream][k:k + 1]


def oracle_run(s, stream, fp32_records=False, step=None):
    """the states after 0 .. K samples (as many as s holds) through the C oracle, a list of (nominal, rot, P, prev); fp32_records: the
    record rounded to fp32 after every step (support.fp32_record_floor); step: a function in place of the oracle's predict (the
    restatement below)"""
    eng = OracleEngine(B, s.dialect, s.nstate)
    eng.set_state(*s.state)
    out = [eng.get_state()]
    for k in range(len(s.acc)):
        h = period_of(s, stream, k)
        if step is None:
            eng.predict(s.acc[k], s.gyr_oracle[k], h)
        else:
            eng.nominal[...], eng.rot[...], eng.P[...] = step(eng.nominal, eng.rot, eng.P, s.acc[k], s.gyr_oracle[k], np.broadcast_to(h, (B,)))
        if fp32_records:
            round_records(eng.nominal, eng.rot, eng.P)
        out.append(eng.get_state())
    return out


def reference(nstate, dialect, stream, guard=False):
    """oracle_run of the scene (guard: of guard_probe), cached and read-only"""
    key = (nstate, dialect, stream, guard)
    if key not in _REFS:
        _REFS[key] = frozen(oracle_run((guard_probe if guard else scene)(nstate, dialect), stream))
    return _REFS[key]


def record_floor(nstate, dialect, stream):
    """util.parity_errors of the K-sample oracle run with fp32 records against the fp64 run"""
    s = scene(nstate, dialect)
    return fp32_record_floor(lambda rounded: oracle_run(s, stream, rounded)[K])[1]


# ---- one ImuUpdate in plain numpy, batched over the filters -------------------------------------------------------------------------------
def _qmul(p, q):                              # quaternion_add.m:22-28
    pw, px, py, pz = p.T
    qw, qx, qy, qz = q.T
    return np.stack([pw * qw - px * qx - py * qy - pz * qz, pw * qx + px * qw + py * qz - pz * qy,
                     pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw], axis=1)


def _q2R(q, eigen):                           # quaternion_to_rotmat.m:22-33 ; Eigen toRotationMatrix (filter.cpp:542,562,564)
    w, x, y, z = q.T
    d = ((1 - 2 * (y * y + z * z), 1 - 2 * (x * x + z * z), 1 - 2 * (x * x + y * y)) if eigen else
         (w * w + x * x - y * y - z * z, w * w - x * x + y * y - z * z, w * w - x * x - y * y + z * z))
    return np.stack([d[0], 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), d[1], 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), d[2]], axis=1).reshape(-1, 3, 3)


def _skew(v):                                 # vector_to_crossmat.m:22-30
    z = np.zeros(len(v))
    return np.stack([z, -v[:, 2], v[:, 1], v[:, 2], z, -v[:, 0], -v[:, 1], v[:, 0], z], axis=1).reshape(-1, 3, 3)


def _sincos(x, mutant):
    if mutant != "d":
        return np.sin(x), np.cos(x)
    x2 = x * x                                # (d) the header's Taylor polynomials through x^7 / x^8 at every angle
    return (x * (1 - x2 / 6 * (1 - x2 / 20 * (1 - x2 / 42))), 1 - x2 / 2 * (1 - x2 / 12 * (1 - x2 / 30 * (1 - x2 / 56))))


def _axisangle(axis, angle, mutant):          # axisangle_to_quaternion.m:22-29 ; matrix_math.hpp:90-99 (0 / 0 at a zero axis, kept)
    s, c = _sincos(angle / 2, mutant)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.concatenate([c[:, None], axis / np.linalg.norm(axis, axis=1, keepdims=True) * s[:, None]], axis=1)


def imu_update(nominal, rot, P, accel, gyro, dt, dialect, q_diag, mutant=None):
    """one ImuUpdate (ImuUpdate.m:36-82 ; filter.cpp:533-616) of B filters, dt (B,) -> new (nominal, rot, P).  mutant: a key of MUTANTS"""
    n, nb = P.shape[1], len(nominal)
    p, v, q, ba, bg, g = (nominal[:, i:j] for i, j in ((0, 3), (3, 6), (6, 10), (10, 13), (13, 16), (16, 19)))
    R, h = rot.reshape(-1, 3, 3), dt[:, None]
    a, w = accel - ba, gyro - bg                                         # ImuUpdate.m:37-38 ; filter.cpp:539,568
    # covariance, from the pre-step state: ImuUpdate.m:63-73 ; filter.cpp:588-616
    hF = np.abs(dt) if mutant == "e" else dt
    Fx = np.tile(np.eye(n), (nb, 1, 1))
    i3 = np.eye(3)[None]
    Fx[:, 0:3, 3:6] = i3 * dt[:, None, None]
    Fx[:, 3:6, 6:9] = -(R @ _skew(a)) * dt[:, None, None]
    Fx[:, 3:6, 9:12] = -R * dt[:, None, None]
    if n == 18:
        Fx[:, 3:6, 15:18] = i3 * dt[:, None, None]
    Fx[:, 6:9, 12:15] = -i3 * dt[:, None, None]
    Kx = _skew(-w * hF[:, None])
    if dialect == 1:                                                     # filter.cpp:603: I - [w]x dt
        Fx[:, 6:9, 6:9] = i3 + Kx
    else:                                                                # ImuUpdate.m:68: expm(-[w]x dt), Rodrigues
        phi = np.linalg.norm(w * hF[:, None], axis=1)
        small = phi < 1e-6
        ps = np.where(small, 1.0, phi)
        ca = np.where(small, 1 - phi * phi / 6, np.sin(ps) / ps)
        cb = np.where(small, 0.5 - phi * phi / 24, (1 - np.cos(ps)) / (ps * ps))
        Fx[:, 6:9, 6:9] = i3 + ca[:, None, None] * Kx + cb[:, None, None] * (Kx @ Kx)
    Pn = Fx @ P @ np.swapaxes(Fx, 1, 2)
    i = np.arange(3, 15)
    Pn[:, i, i] += np.asarray(q_diag)[(i - 3) // 3]                      # Fi Q Fi'
    Pn = (Pn + np.swapaxes(Pn, 1, 2)) / 2
    if mutant == "f":
        Pn[dt == 0] = P[dt == 0]
    # nominal state: ImuUpdate.m:41-60,76-79 ; filter.cpp:533-582
    if dialect == 0:
        dth = np.linalg.norm(w * h, axis=1)                              # norm(w dt): the sign of dt is lost (ImuUpdate.m:41)
        qT, qH = _qmul(q, _axisangle(w, dth, mutant)), _qmul(q, _axisangle(w, dth / 2, mutant))
        R0, RH, RT = R, _q2R(qH, False), _q2R(qT, False)                 # R0: the carried rotation (ImuUpdate.m:46)
    else:
        wn = np.linalg.norm(w, axis=1)
        big = (wn > (1e-5 if mutant == "c" else 10e-5))[:, None]          # filter.cpp:544
        one = np.ones((nb, 1))
        first_T = np.concatenate([one, 0.5 * h * w], axis=1)             # filter.cpp:553-560
        first_H = np.concatenate([one, (0.5 if mutant == "b" else 0.25) * h * w], axis=1)
        if mutant == "a":
            first_T = first_H = np.concatenate([one, 0 * w], axis=1)
        qT = _qmul(q, np.where(big, np.nan_to_num(_axisangle(w, wn * dt, mutant)), first_T))
        qH = _qmul(q, np.where(big, np.nan_to_num(_axisangle(w, wn * dt / 2, mutant)), first_H))
        qT, qH = (x / np.linalg.norm(x, axis=1, keepdims=True) for x in (qT, qH))
        R0, RH, RT = _q2R(q, True), _q2R(qH, True), _q2R(qT, True)       # R0: fresh from q (filter.cpp:542)
    kv1, kv2, kv4 = (np.einsum("bij,bj->bi", X, a) + g for X in (R0, RH, RT))
    kv3 = kv2
    vn = v + h / 6 * (kv1 + 2 * kv2 + 2 * kv3 + kv4)                     # ImuUpdate.m:49-60 ; filter.cpp:567-581
    kp2, kp3, kp4 = v + kv1 * h / 2, v + kv2 * h / 2, v + kv3 * h / 2     # dt / 2 in kp4, sic (ImuUpdate.m:59, filter.cpp:580)
    pn = p + h / 6 * (v + 2 * kp2 + 2 * kp3 + kp4)
    if dialect == 0:
        qT = qT / np.linalg.norm(qT, axis=1, keepdims=True)              # ImuUpdate.m:76
    return np.concatenate([pn, vn, qT, ba, bg, g], axis=1), RT.reshape(-1, 9), Pn


def restated_run(s, stream, mutant=None):
    """oracle_run with imu_update in place of the oracle's predict"""
    q = list(s.prm.q_diag)
    return oracle_run(s, stream, step=lambda nom, rot, P, a, w, h: imu_update(nom, rot, P, a, w, h, s.dialect, q, mutant))


# ---- diagnostics: which class carries an error (kept out of the passing path) -----------------------------------------------------------------
# the gates of util.assert_parity for fp32 records (the rotation figure at its sharper 2e-6) and what an fp64 record is held to
GATES = {"literal": 1e-5, "sigma": 1e-5, "plain": 2e-4, "rot": 2e-6, "cov": 1e-4, "cov_block": 1e-5}
GATES_F64 = {"literal": 1e-9, "sigma": 1e-9, "plain": 1e-9, "rot": 1e-9, "cov": 1e-9, "cov_block": 1e-11}


def worst_figure(e, gates=GATES):
    """(figure, value, value / gate) of the figure of util.parity_errors' dict nearest to (or furthest past) its gate"""
    name = max(gates, key=lambda k: e[k] / gates[k])
    return name, e[name], e[name] / gates[name]


def class_figures(got, ref, s, samples=K):
    """{class: util.parity_errors of the filters that met the class among their first `samples` samples}"""
    from util import parity_errors
    out = {}
    for c in range(C):
        sel = (s.cls[:samples] == c).any(axis=0)
        if sel.any():
            out[c] = parity_errors(tuple(np.asarray(x)[sel] for x in got[:3]), tuple(np.asarray(x)[sel] for x in ref[:3]))
    return out


def print_classes(what, got, ref, s, samples=K, gates=GATES):
    for c, e in class_figures(got, ref, s, samples).items():
        name, value, ratio = worst_figure(e, gates)
        print(f"    {what}: filters that met class {c:2d} ({CLASSES[c][0]:g} rad/s, {CLASSES[c][2]}): worst {name} {value:.2e} = {ratio:.2f} x gate")


def step_class_figures(s, stream, step, gates=GATES):
    """every sample on its own, re-seeded from the reference: step(state k, k) -> the state after sample k, held against the reference's
    state k + 1 on the filters of each class.  -> {class: (figure, value, value / gate)}, the worst over the samples: the class that
    carries an error, without what the filter's other samples add"""
    from util import parity_errors
    ref = reference(s.nstate, s.dialect, stream)
    cls = s.cls if stream == "per" else s.cls + C * (np.arange(K)[:, None] % len(SHARED_DT))
    out = {}
    for k in range(K):
        got = step(ref[k], k)
        for c in np.unique(cls[k]):
            sel = cls[k] == c
            w = worst_figure(parity_errors(tuple(np.asarray(x)[sel] for x in got[:3]), tuple(x[sel] for x in ref[k + 1][:3])), gates)
            if c not in out or w[2] > out[c][2]:
                out[c] = w
    return out


def class_name(c, stream):
    """a class key of step_class_figures in words (shared stream: the rate's class and the sample's period)"""
    if stream == "per":
        return f"class {c} ({CLASSES[c][0]:g} rad/s, dt {CLASSES[c][1]:g} s)"
    return f"rate class {c % C} ({CLASSES[c % C][0]:g} rad/s) at the shared dt {SHARED_DT[c // C]:g} s"
