"""What tests/test_sensor_exits_gpu.py and tests/test_sensor_exits_cpu.py share: the lane plan that sends the filters of one call through
every exit of a streamed sensor kernel (csrc/ekf_depth.hpp, ekf_velocity.hpp, ekf_rows.hpp), the threshold chooser, and the one case
built from them.  The families themselves -- their inputs, the call, the fp64 restatement -- are tests/sensor_families.py's.  A plain
library: no tests and no pytest marks, importable without a GPU.

The exits of a lane, in the order the kernels meet them:
  untouched     skipped, or an input that is not usable: no store, applied = nis = dof = 0, no likelihood term
  not applied   usable, but a pivot is not > 0 or nis <= thr[rows] is false (a NaN among them): no store, applied = 0, nis and dof = rows
                written, rejected += 1
  applied       the stores, applied = 1, ll / rows / applied of the likelihood sums

B = 321, five full 64-filter tiles and a tile of one.  The kind of a lane is decided by its number alone:
  tile 1 (64..127)    every lane skipped: the whole wave leaves at the untouched branch
  tile 3 (192..255)   every lane clean with a planted outlier: the whole wave leaves at the gate
  tiles 0, 2, 4       the unusable kinds on b % 16 in {3, 7, 11, 15} and b % 32 in {5, 13, 21, 29} (the pattern of sensor_families'
                      Rows.mixed), the two broken-record kinds on b % 32 == 9 and == 25, an outlier planted on the clean lanes with
                      b % 5 == 2
  lane 320            clean: the tail tile has an applied lane"""
import types

import numpy as np

from sensor_families import (CLEAN, EXTRA, INF_IN, NAN_IN, NAN_REC, NEG_COV, NIS_TOL, SKIP, VAR_INF, VAR_NAN, VAR_NEG,
                             VAR_ZERO, Depth, Rows, Velocity, family, ft, rnd)

B = 321
TILE = 64
HALF_WIDTH = 5e-3                                    # 50 x NIS_TOL[32]: the smallest relative half-width of the gap the threshold sits in
DIALECT = {18: 1, 15: 0}

KIND_NAMES = {SKIP: "skip", NAN_IN: "NaN residual / reading", INF_IN: "+-inf residual / reading", VAR_ZERO: "var 0", VAR_NEG: "var < 0",
              VAR_INF: "var inf", VAR_NAN: "var NaN", EXTRA: "NaN in gyro (velocity) / in H (rows)", NAN_REC: "record of NaN",
              NEG_COV: "negated covariance"}
UNUSABLE = (SKIP, NAN_IN, INF_IN, VAR_ZERO, VAR_NEG, VAR_INF, VAR_NAN, EXTRA)
BROKEN = (NAN_REC, NEG_COV)


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


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------------------
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
