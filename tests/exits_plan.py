"""What tests/test_sensor_exits_gpu.py and tests/test_sensor_exits_cpu.py share: the lane plan that sends the filters of one call through
every exit of a streamed sensor kernel (csrc/ekf_depth.hpp, ekf_velocity.hpp, ekf_rows.hpp), the threshold chooser, and one adapter per
family -- build the inputs as the family's own suite does, call the update, call the fp64 restatement (depth_ref, velocity_ref,
rows_ref).  A plain library: no tests and no pytest marks, importable without a GPU.

The exits of a lane, in the order the kernels meet them:
  untouched     skipped, or an input that is not usable: no store, applied = nis = dof = 0, no likelihood term
  not applied   usable, but a pivot is not > 0 or nis <= thr[rows] is false (a NaN among them): no store, applied = 0, nis and dof = rows
                written, rejected += 1
  applied       the stores, applied = 1, ll / rows / applied of the likelihood sums

B = 321, five full 64-filter tiles and a tile of one.  The kind of a lane is decided by its number alone:
  tile 1 (64..127)    every lane skipped: the whole wave leaves at the untouched branch
  tile 3 (192..255)   every lane clean with a planted outlier: the whole wave leaves at the gate
  tiles 0, 2, 4       the unusable kinds on b % 16 in {3, 7, 11, 15} and b % 32 in {5, 13, 21, 29} (tests/test_rows_gpu.py's pattern), the
                      two broken-record kinds on b % 32 == 9 and == 25, an outlier planted on the clean lanes with b % 5 == 2
  lane 320            clean: the tail tile has an applied lane"""
import types

import numpy as np

import depth_ref
import rows_ref as W
import velocity_ref as V
from fbus_ekf import BatchedFilter
from support import DT, imu_of, r32, state_batch

B = 321
TILE = 64
NIS_TOL = {32: 1e-4, 64: 1e-9}                       # the three suites' own
HALF_WIDTH = 5e-3                                    # 50 x NIS_TOL[32]: the smallest relative half-width of the gap the threshold sits in
DIALECT = {18: 1, 15: 0}
FACTOR = np.array([1.0, 4.0, 0.25])                  # the three variance rows, by b % 3

CLEAN, SKIP, NAN_IN, INF_IN, VAR_ZERO, VAR_NEG, VAR_INF, VAR_NAN, EXTRA, NAN_REC, NEG_COV = range(11)
KIND_NAMES = {SKIP: "skip", NAN_IN: "NaN residual / reading", INF_IN: "+-inf residual / reading", VAR_ZERO: "var 0", VAR_NEG: "var < 0",
              VAR_INF: "var inf", VAR_NAN: "var NaN", EXTRA: "NaN in gyro (velocity) / in H (rows)", NAN_REC: "record of NaN",
              NEG_COV: "negated covariance"}
UNUSABLE = (SKIP, NAN_IN, INF_IN, VAR_ZERO, VAR_NEG, VAR_INF, VAR_NAN, EXTRA)
BROKEN = (NAN_REC, NEG_COV)


def rnd(a, dtype):
    return r32(a) if dtype == 32 else np.asarray(a, np.float64)


def ft(dtype):
    return np.float32 if dtype == 32 else np.float64


# ---- the lane plan ----------------------------------------------------------------------------------------------------------------------------
def lane_plan(family, nB=B):
    """(kinds (nB,), planted (nB,) bool).  family: "depth" | "velocity" | "rows".  Depth has no input of its own kind (EXTRA): its slot,
    b % 16 == 15, carries the infinite reading a second time.  (+inf and -inf alternate from one group of 16 lanes to the next.)"""
    b = np.arange(nB)
    tile = b // TILE
    mixed = (tile != 1) & (tile != 3)
    kinds = np.zeros(nB, int)
    for k, sel in ((SKIP, b % 16 == 3), (NAN_IN, b % 16 == 7), (INF_IN, b % 16 == 11), (EXTRA if family != "depth" else INF_IN, b % 16 == 15),
                   (VAR_ZERO, b % 32 == 5), (VAR_NEG, b % 32 == 13), (VAR_INF, b % 32 == 21), (VAR_NAN, b % 32 == 29),
                   (NAN_REC, b % 32 == 9), (NEG_COV, b % 32 == 25)):
        kinds[sel & mixed] = k
    kinds[tile == 1] = SKIP
    planted = ((kinds == CLEAN) & mixed & (b % 5 == 2)) | (tile == 3)
    return kinds, planted


def kinds_of(family):
    return tuple(k for k in UNUSABLE + BROKEN if not (family == "depth" and k == EXTRA))


def usable_kind(kinds):
    """the lanes whose INPUTS are usable: clean ones and the two broken-record kinds"""
    return (kinds == CLEAN) | (kinds == NAN_REC) | (kinds == NEG_COV)


def plan_conditions(family, kinds, planted, nB=B):
    """the conditions of the plan on itself; raises AssertionError"""
    b = np.arange(nB)
    for k in kinds_of(family):
        assert (kinds == k).sum() >= 6, (family, KIND_NAMES[k], int((kinds == k).sum()))
    assert (kinds[b // TILE == 1] == SKIP).all()
    assert (kinds[b // TILE == 3] == CLEAN).all() and planted[b // TILE == 3].all()
    assert kinds[nB - 1] == CLEAN and not planted[nB - 1] and (nB - 1) % TILE == 0
    mixed = (b // TILE != 1) & (b // TILE != 3)
    assert all((~usable_kind(kinds) & (b // TILE == t)).any() and (usable_kind(kinds) & (b // TILE == t)).any() for t in (0, 2, 4))
    assert (planted & mixed & (kinds == CLEAN)).sum() >= 10                       # the gate's own lanes in the mixed tiles
    assert ((kinds == CLEAN) & ~planted).sum() >= 80                              # 0.8 of them are applied: >= 64


# ---- the threshold ----------------------------------------------------------------------------------------------------------------------------
def choose_threshold(nis, lo=0.80, hi=0.95):
    """(thr, relative half-width): the midpoint of the widest relative gap between neighbours of the sorted nis in the lo..hi quantile
    band.  Every value differs from thr by at least half-width x thr: an nis within HALF_WIDTH (relative) of its reference falls on the
    reference's side."""
    v = np.sort(np.asarray(nis, np.float64))
    assert np.isfinite(v).all() and (v > 0).all() and len(v) >= 20
    i = np.arange(int(np.ceil(lo * len(v))), int(np.floor(hi * len(v))) + 1)
    half = (v[i] - v[i - 1]) / (v[i] + v[i - 1])
    j = int(np.argmax(half))
    return 0.5 * (v[i[j]] + v[i[j] - 1]), float(half[j])


def gate_only(rows, thr):
    """a gate table whose only finite entry is thr[rows]"""
    t = np.full(4, np.inf)
    t[rows] = thr
    return t


def gate_wrong_entries(rows):
    """a full gate table, thr[rows] = +inf and EVERY other entry 0: a kernel that reads another entry rejects everything"""
    t = np.zeros(257)
    t[rows] = np.inf
    return t


# ---- the families -----------------------------------------------------------------------------------------------------------------------------
def _carried(nB, dtype, n, K):
    """a handle whose records hold a state of support.state_batch behind three predicts (the carried rotation is the stale one): the
    carried() of the three suites.  K: the IMU samples drawn (the suites draw 3 for depth, 4 for velocity and rows: sample 3 is the rate
    that goes with a reading)"""
    prm, nom, rot, P, prev = state_batch(nB, DIALECT[n], n)
    f = BatchedFilter(nB, prm, device=0, dtype=dtype, nstate=n)
    f.set_state(nom, rot, P, prev)
    a, w = imu_of(0, nB, 0, K, nom)
    for k in range(3):
        f.predict(a[k], w[k], DT)
    return f, w[K - 1]


def _spoil_common(kinds, comp, vals, var):
    """the input kinds every family has, on component comp[b] of lane b: vals (nB, rows) the residuals / readings, var (nB, rows)"""
    b = np.arange(len(kinds))
    for k, x in ((NAN_IN, np.nan),):
        vals[kinds == k, comp[kinds == k]] = x
    inf = kinds == INF_IN
    vals[inf, comp[inf]] = np.where((b[inf] // 16) % 2 == 0, np.inf, -np.inf)
    for k, x in ((VAR_ZERO, 0.0), (VAR_NEG, -1e-4), (VAR_INF, np.inf), (VAR_NAN, np.nan)):
        var[kinds == k, comp[kinds == k]] = x


class Depth:
    """fbus_ekf_correct_depth: the sensor of tests/test_depth_gpu.py.  The three variances lie BELOW the smallest H P H' of these states
    (8.4e-5: a position prior of 1e-4 along the tilted axis), so that a negated covariance gives S = -H P H' + var < 0 on every lane
    (prepare() asserts that the restatement sees it so)."""
    name, rows = "depth", 1
    AXIS, LEVER, OFFSET = np.array([0.12, -0.2, 1.0]), np.array([0.11, -0.07, 0.05]), 0.4
    VAR = 1e-5 * FACTOR                                # 1e-5, 4e-5, 2.5e-6

    def __str__(self):
        return "correct_depth"

    def carried(self, nB, dtype, n):
        f, _ = _carried(nB, dtype, n, 3)
        f.set_depth_sensor(self.AXIS, self.OFFSET, self.LEVER)
        return f, None

    def aux_cpu(self, nB, n, nom):
        return None

    def inputs(self, st, dtype, n, aux, seed=6):
        """z = h(the state) + N(0, (1 cm)^2) as the suite's readings() has it; -> (inputs, the diagonal of S (nB, 1)).  (Seed 6: the
        suite's 5 draws lane 320's reading two sigma out, above every threshold of the band, and the tail tile is to have an applied
        lane.)"""
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

    def call(self, f, inp):
        return f.correct_depth_nis(inp["z"], inp["var"], inp["skip"])

    def ref(self, st, n, inp, thr=np.inf):
        """-> ((nominal, rot, P, prev), applied, nis, dof, ln det S)"""
        ss = V.states_of(st, n)
        out = [depth_ref.correct_depth(s, n, float(inp["z"][b]), float(inp["var"][b]), self.AXIS, self.OFFSET, self.LEVER, thr,
                                       bool(inp["skip"][b])) for b, s in enumerate(ss)]
        app, nis, dof, S = (np.array(c) for c in zip(*out))
        with np.errstate(all="ignore"):
            return V.arrays_of(ss), app, nis, dof.astype(np.int32), np.log(S)


class Velocity:
    """fbus_ekf_correct_velocity: the sensor of tests/test_velocity_gpu.py, with the rate sample"""
    name, rows = "velocity", 3
    MOUNT, LEVER = V.tilted_mount(), np.array([0.21, -0.08, 0.12])
    VAR = np.array([1e-4, 4e-4, 2.5e-5])

    def __str__(self):
        return "correct_velocity"

    def carried(self, nB, dtype, n):
        f, w = _carried(nB, dtype, n, 4)
        f.set_velocity_sensor(self.MOUNT, self.LEVER)
        return f, w

    def aux_cpu(self, nB, n, nom):
        return imu_of(0, nB, 0, 4, nom)[1][3]

    def inputs(self, st, dtype, n, aux, seed=5):
        """z = h(the state) + N(0, diag(VAR)) as the suite's readings() has it; -> (inputs, the diagonal of S (nB, 3))"""
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

    def call(self, f, inp):
        return f.correct_velocity_nis(inp["z"], inp["var"], inp["gyro"], inp["skip"])

    def ref(self, st, n, inp, thr=np.inf):
        ss = V.states_of(st, n)
        out = [V.correct_velocity(s, n, inp["z"][b], inp["var"][b], inp["gyro"][b], self.MOUNT, self.LEVER, thr, bool(inp["skip"][b]))
               for b, s in enumerate(ss)]
        app, nis, dof, lnd = (np.array(c) for c in zip(*out))
        return V.arrays_of(ss), app, nis, dof.astype(np.int32), lnd


class Rows:
    """fbus_ekf_correct_rows with m dense rows: the dense() of tests/test_rows_gpu.py"""
    name = "rows"
    RATIO = np.array([300.0, 1000.0, 3000.0])          # H P H' / var of the dense rows, row by row (x 1 / FACTOR)

    def __init__(self, m):
        self.rows = m

    def __str__(self):
        return f"correct_rows m={self.rows}"

    def carried(self, nB, dtype, n):
        f, _ = _carried(nB, dtype, n, 4)
        return f, None

    def aux_cpu(self, nB, n, nom):
        return None

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

    def call(self, f, inp):
        return f.correct_rows_nis(inp["res"], inp["H"], inp["var"], inp["skip"])

    def ref(self, st, n, inp, thr=np.inf):
        return W.update_batch(st, n, inp["res"], inp["H"], inp["var"], thr, inp["skip"])


def family(name, m=None):
    return {"depth": Depth, "velocity": Velocity}[name]() if name != "rows" else Rows(m)


CASES = [("depth", d, n, 1) for d in (32, 64) for n in (18, 15)] + [("velocity", d, n, 3) for d in (32, 64) for n in (18, 15)] + \
        [("rows", d, n, m) for d in (32, 64) for n in (18, 15) for m in (1, 2, 3)]          # the 20 code objects


# ---- one case ---------------------------------------------------------------------------------------------------------------------------------
def broken_records(st, kinds, dtype):
    """a copy of the get_state() arrays st in the record type with the NAN_REC lanes NaN in nominal, rot and P and the covariance of the
    NEG_COV lanes negated (support.poisoned_state's forms (a) and (c))"""
    nom, rot, P = (np.array(x, ft(dtype)) for x in st[:3])
    a, c = kinds == NAN_REC, kinds == NEG_COV
    nom[a], rot[a], P[a] = np.nan, np.nan, np.nan
    P[c] = -P[c]
    return nom, rot, P, np.array(st[3])


def prepare(fam, st0, dtype, n, aux):
    """Everything one case needs, from the healthy carried state st0 (get_state() arrays; aux: the family's rate sample or None).
    The inputs are built from st0, the outlier is planted with the S of st0, and the reference runs on `state`: st0 with its records
    broken.  -> a namespace:
      kinds, planted, inp, state      the plan, the inputs as the call takes them (with skip), the state to set
      thr, half                        the threshold from the reference's nis on the clean, unplanted lanes, and its gap's half-width
      free, gated                      the restatement without a gate and at thr: (state arrays, applied, nis, dof, ln det S)"""
    nB = len(st0[0])
    b = np.arange(nB)
    kinds, planted = lane_plan(fam.name, nB)
    inp, S = fam.inputs(st0, dtype, n, aux)
    vals = fam.values(inp)
    comp = b % fam.rows
    vals[planted, comp[planted]] += 6.0 * np.sqrt(S[planted, comp[planted]])
    vals[...] = rnd(vals, dtype)                                                   # representable in the record type
    fam.spoil(inp, kinds, n)
    inp["skip"] = (kinds == SKIP).astype(np.uint8)
    fam.finish(inp, dtype)
    state = broken_records(st0, kinds, dtype)
    with np.errstate(all="ignore"):
        free = fam.ref(state, n, inp)
        pool = (kinds == CLEAN) & ~planted
        thr, half = choose_threshold(free[2][pool])
        gated = fam.ref(state, n, inp, thr)
    return types.SimpleNamespace(kinds=kinds, planted=planted, inp=inp, state=state, thr=thr, half=half, free=free, gated=gated)


def reference_conditions(fam, case):
    """what the reference itself must show for the case to be the case it claims to be; raises AssertionError"""
    kinds, planted, nB = case.kinds, case.planted, len(case.kinds)
    b = np.arange(nB)
    mixed = (b // TILE != 1) & (b // TILE != 3)
    plan_conditions(fam.name, kinds, planted, nB)
    assert case.half >= HALF_WIDTH, (str(fam), case.half)                         # (a failure here: another seed, not another margin)
    app, nis, dof = case.gated[1].astype(bool), case.gated[2], case.gated[3]
    usable = usable_kind(kinds)
    assert np.array_equal(dof, fam.rows * usable.astype(np.int32))
    assert np.array_equal(case.free[1].astype(bool), kinds == CLEAN)              # without a gate: every clean lane, no broken record
    assert np.isnan(nis[kinds == NAN_REC]).all() and np.isfinite(nis[kinds == NEG_COV]).all()
    assert (nis[~usable] == 0).all()
    assert not app[b // TILE == 3].any() and not app[b // TILE == 1].any()        # two waves that leave whole
    assert ((kinds == CLEAN) & mixed & ~app).sum() >= 10 and app.sum() >= 64 and app[nB - 1]
    assert np.array_equal(app, (kinds == CLEAN) & (nis <= case.thr))
