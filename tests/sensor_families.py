"""The three families of streamed sensor updates -- fbus_ekf_correct_depth, fbus_ekf_correct_velocity, fbus_ekf_correct_rows (csrc/ekf_depth.hpp,
ekf_velocity.hpp, ekf_rows.hpp over csrc/ekf_sensor.hpp) -- as the tests see them, and the only place in tests/ that knows them: one adapter
per family with the sensor's constants, the inputs of its suites, the call in every form and the fp64 restatement (depth_ref, velocity_ref,
rows_ref).  tests/test_sensor_suite_{cpu,gpu}.py run every family through the same tests, tests/exits_plan.py sends them through every
exit, tests/test_{depth,velocity,rows}_gpu.py keep what is a family's own.  A plain library: no tests and no pytest marks, importable
without a GPU.

A family carries
  name, rows, variants, labels     the row count; the sensor variants of the one-update test, the first one the full sensor
  set_sensor(f, variant)           the handle's sensor
  readings(st, dtype, aux, variant, seed)    the plain inputs, a dict in call order: z = h(the state) + noise of the sensor's size
  mixed(st, dtype, aux)            readings with a tail of outliers, three variance rows and the lanes that must stay untouched, one kind
                                   per lane group: the inputs with "skip" and "kinds" (0 usable, 1 .. KINDS the unusable kinds)
  ref(st, n, inputs, thr, joseph, variant)   -> (state arrays, applied, nis, dof, ln det S)
  call(f, inputs, form), FORMS     one update through the form; the forms the family has
  SHARE, THR, CAP, MIN_APPLIED     the gate share of gate_between, the fixed threshold, the cap on the share of lanes not applied under
                                   the former and the least number applied under the latter
  UNUSABLE, KINDS                  the unusable lanes of mixed() at B = 193 and the number of their kinds
and, for tests/exits_plan.py alone, inputs / values / spoil / finish: that plan's own builders.  one_update() at the end is the body of the
one-update parity test that each family's module runs under its own ids."""
import ctypes as C

import numpy as np
import torch

import depth_ref
import rows_ref as W
import velocity_ref as V
from fbus_ekf import BatchedFilter
from support import B_IND, DT, imu_of, r32, same_state, state_batch
from util import assert_parity

NAMES = ("nominal", "rot", "P", "prev")
NIS_TOL = {32: 1e-4, 64: 1e-9}                       # fp32: S inherits the covariance gate
FACTOR = np.array([1.0, 4.0, 0.25])                  # the three variance rows, by b % 3

# the kinds of a lane of tests/exits_plan.py (its lane_plan decides which lane is of which kind; spoil() below writes them)
CLEAN, SKIP, NAN_IN, INF_IN, VAR_ZERO, VAR_NEG, VAR_INF, VAR_NAN, EXTRA, NAN_REC, NEG_COV = range(11)


def rnd(a, dtype):
    return r32(a) if dtype == 32 else np.asarray(a, np.float64)


def ft(dtype):
    return np.float32 if dtype == 32 else np.float64


def rel(a, b):
    return np.abs(a - b) / np.abs(b)


def gate_between(nis, share):
    """a threshold strictly between two neighbouring values of the sorted finite nis"""
    v = np.sort(nis[np.isfinite(nis) & (nis > 0)].astype(np.float64))
    i = int(share * len(v))
    assert v[i - 1] < v[i]
    return 0.5 * (v[i - 1] + v[i])


def chi2_gate(m):
    return {1: 3.84, 2: 5.99, 3: 7.81}[m]              # chi-square, 95 %: the outlier tail lies above it


def outs(f, nis=None, dof=None):
    d = dict(zip(NAMES, f.get_state()), applied=f.applied())
    if nis is not None:
        d.update(nis=nis, dof=dof)
    return d


def carried(nB, dtype, n, dialect, seed_off=0):
    """a handle whose records hold a state of support.state_batch behind three predicts (the carried rotation is the stale one);
    returns (handle, the rate sample that goes with a reading: the fourth IMU sample, the first three are the predicts')"""
    prm, nom, rot, P, prev = state_batch(nB, dialect, n, seed_off=seed_off)
    f = BatchedFilter(nB, prm, device=0, dtype=dtype, nstate=n)
    f.set_state(nom, rot, P, prev)
    a, w = imu_of(seed_off, seed_off + nB, 0, 4, nom)
    for k in range(3):
        f.predict(a[k], w[k], DT)
    return f, w[3]


def _spoil_common(kinds, comp, vals, var):
    """the input kinds every family has, on component comp[b] of lane b: vals (nB, rows) the residuals / readings, var (nB, rows)"""
    b = np.arange(len(kinds))
    for k, x in ((NAN_IN, np.nan),):
        vals[kinds == k, comp[kinds == k]] = x
    inf = kinds == INF_IN
    vals[inf, comp[inf]] = np.where((b[inf] // 16) % 2 == 0, np.inf, -np.inf)
    for k, x in ((VAR_ZERO, 0.0), (VAR_NEG, -1e-4), (VAR_INF, np.inf), (VAR_NAN, np.nan)):
        var[kinds == k, comp[kinds == k]] = x


def _four_kinds(vals, var, comp):
    """the lanes of mixed() that depth and velocity share, on component comp[b] of lane b of vals and var (nB, rows): 1 skipped, 2 a NaN
    reading, 3 a variance <= 0, 4 a NaN variance; -> kinds"""
    b = np.arange(len(vals))
    kinds = np.zeros(len(vals), int)
    kinds[b % 16 == 3], kinds[b % 16 == 7], kinds[b % 32 == 11], kinds[b % 32 == 27] = 1, 2, 3, 4
    vals[kinds == 2, comp[kinds == 2]] = np.nan
    var[kinds == 3, comp[kinds == 3]] = np.where(b[kinds == 3] % 64 == 11, 0.0, -1e-4)
    var[kinds == 4, comp[kinds == 4]] = np.nan
    return kinds


class _Family:
    """what the three have in common.  keys: the inputs in the order of the Python call (the C call has var behind the others);
    typed: those in the record type; head: the integers in front of the C call's arrays"""
    head = ()
    CAP, MIN_APPLIED = 1 / 3, B_IND // 2 + 1
    SECOND = None                                      # a second call of the likelihood test
    NEG_COV_VAR = None                                 # the variance under which every negated covariance gives S < 0, where VARS does not
    FORMS = ("host", "dev", "async", "nis null", "nis dev", "graph")
    DEVICE_FORMS = ("dev", "nis null", "nis dev", "graph")

    def __str__(self):
        return "correct_" + self.name

    def handle(self, nB, dtype, n, dialect, variant=None, seed_off=0):
        """carried() with the sensor set -> (handle, its state as get_state() gives it, the rate sample)"""
        f, w = carried(nB, dtype, n, dialect, seed_off)
        self.set_sensor(f, variant)
        return f, f.get_state(), w

    def aux_cpu(self, nB, n, nom):
        """the rate sample of carried(), without a handle"""
        return imu_of(0, nB, 0, 4, nom)[1][3]

    def gate(self, thr):
        """a gate table whose thr[rows] is thr"""
        return [np.inf] * self.rows + [thr]

    def cast(self, inp, dtype):
        """the inputs with the typed ones in the record type, as a device form takes them"""
        return {k: v.astype(ft(dtype)) if k in self.typed else v for k, v in inp.items()}

    def usable(self, inp):
        """the header's rule on the inputs, lane by lane: not skipped, every input finite, every variance > 0"""
        ok = inp["skip"] == 0
        for k in self.keys:
            x = np.asarray(inp[k], np.float64).reshape(len(ok), -1)
            ok = ok & np.isfinite(x).all(axis=1) & ((x > 0).all(axis=1) if k == "var" else True)
        return ok

    def per_filter(self, inp):
        """-> (the inputs with a variance per filter, [(a variance for every filter, the filters whose own it is), ...])"""
        k = np.arange(len(inp[self.keys[0]])) % 3
        return dict(inp, var=self.VARS[k]), [(v if v.ndim else float(v), np.nonzero(k == i)[0]) for i, v in enumerate(self.VARS)]

    def call(self, f, inp, form):
        """one update.  "host" / "dev": the plain call on the arrays as they are, numpy or device tensors; "nis" / "nis dev": the _nis form
        likewise, -> (nis, dof); "async": pinned copies through the _async form, waited for; "nis null": fbus_ekf_correct_*_nis_dev on
        device tensors with neither output"""
        a = [inp[k] for k in self.keys] + [inp.get("skip")]
        stem = "correct_" + self.name
        if form in ("host", "dev"):
            return getattr(f, stem)(*a)
        if form in ("nis", "nis dev"):
            return getattr(f, stem + "_nis")(*a)
        if form == "async":
            getattr(f, stem + "_async")(*(None if x is None else torch.from_numpy(np.ascontiguousarray(x)).pin_memory() for x in a))
            return f.async_inputs_consumed()
        assert form == "nis null", form
        vp = lambda t: C.c_void_p(t.data_ptr())
        ptrs = [vp(inp[k]) for k in self.keys if k != "var"] + [vp(inp["var"])]
        assert getattr(f._lib, f"fbus_ekf_{stem}_nis_dev")(f._h, *self.head, *ptrs, 1, vp(inp["skip"]), None, None) == 0


class Depth(_Family):
    """fbus_ekf_correct_depth, a tilted axis.  The three variances of the exits plan lie BELOW the smallest H P H' of these states
    (8.4e-5: a position prior of 1e-4 along the tilted axis), so that a negated covariance gives S = -H P H' + var < 0 on every lane
    (exits_plan.prepare() asserts that the restatement sees it so)."""
    name, rows, keys, typed = "depth", 1, ("z", "var"), ("z",)
    AXIS, LEVER, OFFSET = np.array([0.12, -0.2, 1.0]), np.array([0.11, -0.07, 0.05]), 0.4
    SENSOR_VAR = 1e-4                                  # a 1 cm sensor beside a prior of ~1 cm in position
    VARS = np.array([1e-4, 4e-4, 2.5e-5])
    VAR = 1e-5 * FACTOR                                # the exits plan's: 1e-5, 4e-5, 2.5e-6
    variants, labels = ((LEVER,), (None,)), ("lever", "no lever")
    SHARE, THR, UNUSABLE, KINDS = 0.85, 4.0, 36, 4
    NEG_COV_VAR = 2.5e-5

    def set_sensor(self, f, variant=None):
        f.set_depth_sensor(self.AXIS, self.OFFSET, (variant or self.variants[0])[0])

    def readings(self, st, dtype, aux=None, variant=None, seed=5, sigma=0.01):
        """z = h(the handle's own state) + N(0, sigma^2), representable in the record type"""
        nom, rot = np.asarray(st[0], np.float64), np.asarray(st[1], np.float64)
        lv = depth_ref.lever_of((variant or self.variants[0])[0])
        hx = (nom[:, 0:3] + rot.reshape(-1, 3, 3) @ lv) @ depth_ref.unit(self.AXIS) + self.OFFSET
        return dict(z=rnd(hx + np.random.default_rng(seed).normal(0, sigma, len(nom)), dtype), var=self.SENSOR_VAR)

    def mixed(self, st, dtype, aux=None):
        b = np.arange(len(st[0]))
        z = np.array(self.readings(st, dtype)["z"])
        z[b % 5 == 2] += 0.08                                  # outliers for the gate
        z = rnd(z, dtype)
        var = self.VARS[b % 3].copy()
        kinds = _four_kinds(z.reshape(-1, 1), var.reshape(-1, 1), np.zeros(len(b), int))
        return dict(z=z, var=var, skip=(kinds == 1).astype(np.uint8), kinds=kinds)

    def ref(self, st, n, inp, thr=np.inf, joseph=False, variant=None):
        ss = V.states_of(st, n)
        z, skip = inp["z"], inp.get("skip")
        var = np.broadcast_to(np.asarray(inp["var"], np.float64), (len(ss),))
        out = [depth_ref.correct_depth(s, n, float(z[b]), float(var[b]), self.AXIS, self.OFFSET, (variant or self.variants[0])[0], thr,
                                       bool(skip[b]) if skip is not None else False, joseph) for b, s in enumerate(ss)]
        app, nis, dof, S = (np.array(c) for c in zip(*out))
        with np.errstate(all="ignore"):
            return V.arrays_of(ss), app, nis, dof.astype(np.int32), np.log(S)

    # ---- the exits plan's builders
    def inputs(self, st, dtype, n, aux, seed=6):
        """z = h(the state) + N(0, (1 cm)^2) as readings() has it; -> (inputs, the diagonal of S (nB, 1)).  (Seed 6: readings()'s 5
        draws lane 320's reading two sigma out, above every threshold of the band, and the tail tile is to have an applied lane.)"""
        nom, rot, P = (np.asarray(x, np.float64) for x in st[:3])
        nB = len(nom)
        a = depth_ref.unit(self.AXIS)
        Rm = rot.reshape(-1, 3, 3)
        hx = (nom[:, 0:3] + Rm @ self.LEVER) @ a + self.OFFSET
        z = rnd(hx + np.random.default_rng(seed).normal(0, 0.01, nB), dtype)
        H = np.zeros((nB, n))
        H[:, 0:3] = a
        H[:, 6:9] = np.cross(self.LEVER, np.einsum("bji,j->bi", Rm, a))
        var = self.VAR[np.arange(nB) % 3].copy()
        S = np.einsum("bi,bij,bj->b", H, P, H) + var
        return dict(z=z.reshape(nB, 1), var=var.reshape(nB, 1)), S.reshape(nB, 1)

    def values(self, inp):
        return inp["z"]

    def spoil(self, inp, kinds, n):
        _spoil_common(kinds, np.zeros(len(kinds), int), inp["z"], inp["var"])

    def finish(self, inp, dtype):
        inp["z"] = np.ascontiguousarray(inp["z"].ravel(), ft(dtype))
        inp["var"] = np.ascontiguousarray(inp["var"].ravel())


class Velocity(_Family):
    """fbus_ekf_correct_velocity, a mount with no zero entry, with the rate sample.  A variant is (mount, lever, rate sample given)."""
    name, rows, keys, typed = "velocity", 3, ("z", "var", "gyro"), ("z", "gyro")
    MOUNT, LEVER = V.tilted_mount(), np.array([0.21, -0.08, 0.12])
    VAR = np.array([1e-4, 4e-4, 2.5e-5])
    VARS = VAR[None, :] * FACTOR[:, None]
    FULL, BARE, LEVER_UNUSED, MOUNT_ONLY = (MOUNT, LEVER, True), (None, None, False), (None, LEVER, False), (MOUNT, None, False)
    variants, labels = (FULL, BARE), ("full", "bare")
    SHARE, THR, UNUSABLE, KINDS = 0.9, 7.81, 42, 5         # THR: chi-square, 3 degrees of freedom, 95 %: the outlier tail lies above it

    def set_sensor(self, f, variant=None):
        f.set_velocity_sensor(*(variant or self.FULL)[:2])

    def predicted(self, st, gyro, mount, lever):
        """h of the handle's own state, (B, 3) in double"""
        nom, rot = np.asarray(st[0], np.float64), np.asarray(st[1], np.float64).reshape(-1, 3, 3)
        y = np.einsum("bji,bj->bi", rot, nom[:, 3:6])
        if gyro is not None:
            y = y + np.cross(gyro - nom[:, 13:16], V.lever_of(lever))
        return y @ V.mount_of(mount).T

    def readings(self, st, dtype, aux=None, variant=None, seed=5):
        """z = h(the handle's own state) + N(0, diag(VAR)), representable in the record type"""
        mount, lever, rate = variant or self.FULL
        gyro = aux if rate else None
        e = np.random.default_rng(seed).normal(0, 1, (len(st[0]), 3)) * np.sqrt(self.VAR)
        return dict(z=rnd(self.predicted(st, gyro, mount, lever) + e, dtype), var=self.VAR, gyro=gyro)

    def mixed(self, st, dtype, aux):
        """The lanes b % 32 == 19 are among the skipped ones (19 % 16 == 3) and carry a NaN rate as well; the rate rule has lanes of its
        own (kind 5) at b % 32 == 21: 12 + 12 + 6 + 6 + 6 = 42 of the 193 lanes are unusable."""
        b = np.arange(len(st[0]))
        z = np.array(self.readings(st, dtype, aux)["z"])
        z[b % 5 == 2, 1] += 2.0                                # outliers for the gate: S is of the order of the prior's 0.13 (m/s)^2
        z = rnd(z, dtype)
        var = self.VARS[b % 3].copy()
        gyro = np.array(aux)
        kinds = _four_kinds(z, var, b % 3)
        kinds[b % 32 == 21] = 5
        gyro[(kinds == 5) | (b % 32 == 19), 2] = np.nan
        return dict(z=z, var=var, gyro=gyro, skip=(kinds == 1).astype(np.uint8), kinds=kinds)

    def ref(self, st, n, inp, thr=np.inf, joseph=False, variant=None):
        mount, lever, _ = variant or self.FULL
        ss = V.states_of(st, n)
        z, gyro, skip = inp["z"], inp["gyro"], inp.get("skip")
        var = np.broadcast_to(np.asarray(inp["var"], np.float64), (len(ss), 3))
        out = [V.correct_velocity(s, n, z[b], var[b], None if gyro is None else gyro[b], mount, lever, thr,
                                  bool(skip[b]) if skip is not None else False, joseph) for b, s in enumerate(ss)]
        app, nis, dof, lnd = (np.array(c) for c in zip(*out))
        return V.arrays_of(ss), app, nis, dof.astype(np.int32), lnd

    # ---- the exits plan's builders
    def inputs(self, st, dtype, n, aux, seed=5):
        """z = h(the state) + N(0, diag(VAR)) as readings() has it; -> (inputs, the diagonal of S (nB, 3))"""
        nB = len(st[0])
        ss = V.states_of(st, n)
        hx = np.array([V.h(s, self.MOUNT, self.LEVER, aux[b]) for b, s in enumerate(ss)])
        z = rnd(hx + np.random.default_rng(seed).normal(0, 1, (nB, 3)) * np.sqrt(self.VAR), dtype)
        var = (self.VAR[None, :] * FACTOR[np.arange(nB) % 3][:, None]).copy()
        H = np.array([V.H_rows(s, n, self.MOUNT, self.LEVER, aux[b]) for b, s in enumerate(ss)])
        S = np.einsum("bki,bij,bkj->bk", H, np.asarray(st[2], np.float64), H) + var
        return dict(z=np.array(z), var=var, gyro=np.array(aux)), S

    def values(self, inp):
        return inp["z"]

    def spoil(self, inp, kinds, n):
        b = np.arange(len(kinds))
        _spoil_common(kinds, b % 3, inp["z"], inp["var"])
        inp["gyro"][kinds == EXTRA, b[kinds == EXTRA] % 3] = np.nan

    def finish(self, inp, dtype):
        inp["z"], inp["gyro"] = np.ascontiguousarray(inp["z"], ft(dtype)), np.ascontiguousarray(inp["gyro"], ft(dtype))


class Rows(_Family):
    """fbus_ekf_correct_rows with m dense rows"""
    name, keys, typed = "rows", ("res", "H", "var"), ("res", "H")
    RATIO = np.array([300.0, 1000.0, 3000.0])          # H P H' / var of the dense rows, row by row (the exits plan: x 1 / FACTOR)
    variants, labels = (None,), ("dense",)
    SHARE, UNUSABLE, KINDS = 0.9, 72, 8
    CAP, MIN_APPLIED = 1 / 2, 80                       # 121 lanes are usable, a fifth of them outliers
    SECOND = dict(m=1, seed=23, thr=1e9)               # the likelihood test: then m = 1 on the new state, on every lane
    PICKS = (0, 63, 64, 100, 192)                      # per_filter(): every one of these has a variance set of its own
    FORMS = ("host", "dev", "nis", "nis null", "nis dev", "graph")

    def __init__(self, m):
        self.rows, self.head, self.THR = m, (m,), chi2_gate(m)

    def __str__(self):
        return f"correct_rows m={self.rows}"

    def set_sensor(self, f, variant=None):
        pass

    def dense(self, st, dtype, seed=5):
        """dense rows, every column non-zero, scaled by the prior's sigmas so that every block of the state is in play; a variance per
        filter and row that puts H P H' / var at RATIO; a residual of the size of S.  All representable in the record type (var is
        double).  -> res (B, m), H (B, m, n), var (B, m), hph (B, m)"""
        m, P = self.rows, np.asarray(st[2], np.float64)
        nB, n = P.shape[:2]
        rng = np.random.default_rng(seed + 10 * m)
        d = 1.0 / np.sqrt(np.median(np.einsum("bii->bi", P), axis=0))
        H = rng.uniform(0.3, 1.0, (nB, m, n)) * rng.choice([-1.0, 1.0], (nB, m, n)) * d
        H = rnd(H, dtype)
        hph = np.einsum("bki,bij,bkj->bk", H, P, H)
        var = hph / self.RATIO[:m]
        res = rnd(rng.normal(0, 1, (nB, m)) * np.sqrt(hph + var), dtype)
        return res.astype(ft(dtype)), H.astype(ft(dtype)), var, hph

    def readings(self, st, dtype, aux=None, variant=None, seed=5):
        res, H, var, _ = self.dense(st, dtype, seed)
        return dict(res=res, H=H, var=var)

    def mixed(self, st, dtype, aux=None):
        """dense rows with a tail of outliers on one residual, and the lanes that must stay untouched, one kind per lane group
        (b % 16 == 3, 7, 11, 15 and b % 32 == 5, 13, 21, 29): 12 x 4 + 6 x 4 = 72 of the 193 lanes.  kinds: 1 skip, 2 NaN res, 3 inf res,
        4 NaN in H, 5 var 0, 6 var < 0, 7 var inf, 8 var NaN"""
        m, n = self.rows, np.shape(st[2])[1]
        b = np.arange(len(st[0]))
        res, H, var, hph = self.dense(st, dtype)
        res, H, var = res.copy(), H.copy(), var.copy()
        out = b % 5 == 2
        res[out, 1 % m] += (6.0 * np.sqrt(hph[out, 1 % m])).astype(res.dtype)          # outliers for the gate
        kinds = np.zeros(len(b), int)
        for k, sel in ((1, b % 16 == 3), (2, b % 16 == 7), (3, b % 16 == 11), (4, b % 16 == 15), (5, b % 32 == 5), (6, b % 32 == 13),
                       (7, b % 32 == 21), (8, b % 32 == 29)):
            kinds[sel] = k
        res[kinds == 2, b[kinds == 2] % m] = np.nan
        res[kinds == 3, b[kinds == 3] % m] = np.inf
        w = b[kinds == 4]
        H[w, w % m, (5 * w) % n] = np.nan                                             # a single entry
        for k, x in ((5, 0.0), (6, -1e-4), (7, np.inf), (8, np.nan)):
            var[kinds == k, b[kinds == k] % m] = x
        return dict(res=res, H=H, var=var, skip=(kinds == 1).astype(np.uint8), kinds=kinds)

    def per_filter(self, inp):
        return inp, [(inp["var"][b], [b]) for b in self.PICKS]            # the m scalars of filter b for every filter

    def ref(self, st, n, inp, thr=np.inf, joseph=False, variant=None):
        return W.update_batch(st, n, inp["res"], inp["H"], inp["var"], thr, inp.get("skip"), joseph)

    # ---- the exits plan's builders
    def inputs(self, st, dtype, n, aux, seed=5):
        """dense rows, every column non-zero, scaled by the prior's sigmas; a variance per filter and row that puts H P H' / var at
        RATIO / FACTOR; a residual of the size of S; -> (inputs, the diagonal of S (nB, m))"""
        m = self.rows
        P = np.asarray(st[2], np.float64)
        nB = len(P)
        rng = np.random.default_rng(seed + 10 * m)
        d = 1.0 / np.sqrt(np.median(np.einsum("bii->bi", P), axis=0))
        H = rnd(rng.uniform(0.3, 1.0, (nB, m, n)) * rng.choice([-1.0, 1.0], (nB, m, n)) * d, dtype)
        hph = np.einsum("bki,bij,bkj->bk", H, P, H)
        var = hph / self.RATIO[:m]
        res = rnd(rng.normal(0, 1, (nB, m)) * np.sqrt(hph + var), dtype)
        var = var * FACTOR[np.arange(nB) % 3][:, None]
        return dict(res=np.array(res), H=np.array(H), var=var), hph + var

    def values(self, inp):
        return inp["res"]

    def spoil(self, inp, kinds, n):
        b = np.arange(len(kinds))
        _spoil_common(kinds, b % self.rows, inp["res"], inp["var"])
        w = b[kinds == EXTRA]
        inp["H"][w, w % self.rows, (5 * w) % n] = np.nan          # a single entry, in row b % m

    def finish(self, inp, dtype):
        inp["res"], inp["H"] = np.ascontiguousarray(inp["res"], ft(dtype)), np.ascontiguousarray(inp["H"], ft(dtype))


def family(name, m=None):
    return {"depth": Depth, "velocity": Velocity}[name]() if name != "rows" else Rows(m)


# ---- the one-update parity check, which every family's own module runs under its own ids -------------------------------------------------------
def velocity_tail(fam, variant, dtype, n, dialect, st0, inp, got):
    # H_theta = C [R' v]x is in play on every filter
    Rtv = np.einsum("bji,bj->bi", np.asarray(st0[1], np.float64).reshape(-1, 3, 3), np.asarray(st0[0], np.float64)[:, 3:6])
    assert np.linalg.norm(Rtv, axis=1).min() > 1e-3
    if variant is fam.BARE:
        # the gyro bias is not a column of H: it moves through its cross-covariance with v and theta alone (and it does move)
        assert not np.array_equal(got[0][:, 13:16], st0[0][:, 13:16])
        # ... and a lever without a rate sample is not used: the same bits as the sensor without one
        f, st1, _ = fam.handle(B_IND, dtype, n, dialect, fam.LEVER_UNUSED)
        with f:
            assert same_state(st0, st1)
            fam.call(f, inp, "host")
            assert same_state(got, f.get_state())


def rows_tail(fam, variant, dtype, n, dialect, st0, inp, got):
    H = inp["H"].astype(np.float64)
    assert (H != 0).all()
    ratio = np.einsum("bki,bij,bkj->bk", H, np.asarray(st0[2], np.float64), H) / inp["var"]
    assert ratio.min() >= 100 and ratio.max() <= 1e4, (ratio.min(), ratio.max())          # in the hundreds to thousands, every row
    assert not np.array_equal(got[0], st0[0])


TAIL = {"depth": lambda *a: None, "velocity": velocity_tail, "rows": rows_tail}


def one_update(fam, dtype, n, dialect):
    """the body of test_one_update_against_the_restatement of tests/test_{depth,velocity,rows}_gpu.py: one update of B = 193 filters
    with every sensor variant of the family against the restatement in its literal and its Joseph form, then the family's tail"""
    for variant, label in zip(fam.variants, fam.labels):
        f, st0, aux = fam.handle(B_IND, dtype, n, dialect, variant)
        with f:
            inp = fam.readings(st0, dtype, aux, variant)
            nis, dof = fam.call(f, inp, "nis")
            got, app = f.get_state(), f.applied()
        assert app.all() and (dof == fam.rows).all()
        for joseph in (False, True):
            ref, rapp, rnis, rdof, _ = fam.ref(st0, n, inp, joseph=joseph, variant=variant)
            assert rapp.all()
            print(f"nis rel err {rel(nis.astype(np.float64), rnis).max():.3e}")
            assert_parity(got, ref, dtype, f"{fam} f{dtype} N={n} dialect {dialect} {label} joseph {joseph}")
            assert rel(nis.astype(np.float64), rnis).max() <= NIS_TOL[dtype]
        assert np.array_equal(got[1], st0[1]) and np.array_equal(got[3], st0[3])          # R and prev_id are not written
        if n == 15:
            assert np.array_equal(got[0][:, 16:19], st0[0][:, 16:19])                      # no gravity state: g stays
        TAIL[fam.name](fam, variant, dtype, n, dialect, st0, inp, got)
