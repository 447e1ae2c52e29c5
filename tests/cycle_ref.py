"""The IMM cycle of include/fbus_ekf.h ("hypothesis groups": loglik_reset, a window of frames, the sensor updates, logw = logc + ll,
group_fuse, group_mix) as a MISSION of C stretches, and its fp64 reference COMPOSED of the restatements the suite already has: the C oracle
(oracle_capi: predict, pose rows, pixel rows) with one parameter set per hypothesis (support.with_row), sensor_families' depth_ref /
velocity_ref / rows_ref, loglik_ref.dense_pose / dense_pixels for the ll terms, group_ref.fuse and group_mix_ref.mix.  No arithmetic of
its own.  tests/test_cycle_cpu.py holds the conditions that make the comparison meaningful, tests/test_cycle_gpu.py runs the device
against it.  A plain library: no tests and no pytest marks, importable without a GPU.

A bank is NG vehicles x G members, filter b = vehicle b // G, member b % G, running hypothesis (row of the noise table) (g + j) % G; all
members of a vehicle start from the same state and get the same IMU samples and readings.  One stretch:
    loglik_reset
    a window of 3 frames, kcount = KCOUNT, of the cell's pose / pixel rows          (ungated: the window entry points ignore the gate)
    predict_n K = 2, correct_depth, one variance
    one predict,     correct_velocity: rate sample, tilted mount, lever, a variance set per filter
    one predict,     correct_rows m = 2: the first two rows of rows_ref.fix_inputs at the state of that moment
    the sums; logw = logc + ll; group_fuse; group_mix -> weight, logc
(9 IMU samples and 6 updates.)  The gate table chi-square 0.999 reaches the cell's largest dof.  In EVERY stretch the vehicles
j % 8 == 1 get an outlier depth reading (+0.5 m), j % 8 == 3 an outlier velocity reading (+4 m/s on axis 1), j % 8 == 5 an outlier fix
(+0.5 m on row 0): every sensor kind rejects somewhere, in every stretch."""
import functools
import types

import numpy as np

import group_mix_ref
import group_ref
import rows_ref
import sensor_families as F
from fbus_ekf import capi, gating, noise, synth
from loglik_ref import LN2PI, dense_pixels, dense_pose, tol_m2ll
from replay_ref import OracleEngine
from support import DT, SIZE, frozen, r32, round_records, with_row
from util import (COV_BLOCK_TOL, COV_BLOCK_TOL_F64, COV_TOL, F64_TOL, FLOOR_FACTOR, PLAIN_WINDOW_TOL, STATE_TOL, WINDOW_COV_BLOCK_TOL,
                  WINDOW_TOL, cov_rel_err, cov_rel_err_blockwise, parity_errors, pixel_scene, state_rel_err, state_rel_err_literal, window_literal_tol)

C = 3
KCOUNT = (2, 0, 3)
K_SENSOR = (2, 1, 1)                         # IMU samples in front of the depth, the velocity and the rows update
K_STRETCH = sum(KCOUNT) + sum(K_SENSOR)
F_WIN = len(KCOUNT)
STAY = 0.9
GATE_PROB = 0.999
M_ROWS = 2
OUTLIER = {"depth": (1, 0.5), "velocity": (3, 4.0), "rows": (5, 0.5)}      # kind -> (vehicles j % 8 == this, size)
KINDS = ("depth", "velocity", "rows")
DEPTH, VELOCITY, ROWS = F.Depth(), F.Velocity(), F.Rows(M_ROWS)

# window: "stacked" | "nearest" (pose rows) | "left" (pixel rows of the left camera).  grid: the two table columns, G factors each;
# hypothesis k is row (k, k) of noise.grid's G x G product -- every hypothesis differs from every other in both columns.  The first column
# is a process noise, the second the window's measurement noise, both ascending ladders.  Member g of vehicle j runs hypothesis
# (g + j) % G (hypothesis_of): the same G rows in every group, in an order that turns from vehicle to vehicle, so that `best` names
# different members in different groups.  wrong: the column the wrong-member mutation reads from member (g + 1) % G.
# noise_frac: the window's measurement noise as a fraction of sqrt(R).  It is SMALL on purpose: the evidence then comes from log det S,
# which the draw does not move, and every group ranks its hypotheses with about the same margins (tests/test_cycle_cpu.py holds them).
def _cell(name, B, G, N, dialect, window, M, q_col, q_fac, r_col, r_step, noise_frac=0.1):
    return types.SimpleNamespace(name=name, B=B, G=G, N=N, dialect=dialect, window=window, M=M, wrong=r_col, noise_frac=noise_frac,
                                 grid={q_col: list(q_fac), r_col: [r_step ** k for k in range(G)]},
                                 pick=tuple(k * G + k for k in range(G)))


CELLS = {
    "A": _cell("A", 192, 3, 18, 0, "stacked", 4, "q_v", (0.5, 1.0, 2.0), "r_pos", 1.08),
    "B": _cell("B", 128, 4, 15, 1, "nearest", 3, "q_theta", (0.5, 1.0, 2.0, 4.0), "r_quat", 1.28),
    "C": _cell("C", 192, 8, 18, 0, "left", 3, "q_v", (0.5, 0.7, 1.0, 1.4, 2.0, 2.8, 4.0, 5.6), "r_pix", 1.10),
}
MUTATIONS = {"no_logc": "any", "no_reset": "any", "rot_own": "A", "prev_chart": "B", "no_spread": "any", "depth_var": "any",
             "apply_rejected": "any", "wrong_member": "any"}


def rows_per_frame(cell, ids):
    """rows of S of one window frame, per filter, by the header's rules: all 7 rows of each used marker (both dialects), 8 per marker in
    view of the left camera.  ids (B, M): the frame's marker slots"""
    n = (np.asarray(ids) >= 0).sum(axis=1)
    return {"stacked": 7 * n, "nearest": 7 * (n > 0), "left": 8 * n}[cell.window]


def max_dof(cell):
    per = 7 if cell.dialect == 1 else 3
    return max({"stacked": per * cell.M, "nearest": per, "left": 8 * cell.M}[cell.window], 3)


def member_of(cell):
    return np.arange(cell.B) % cell.G


def hypothesis_of(cell):
    """the table row of every filter: member g of vehicle j runs hypothesis (g + j) % G"""
    b = np.arange(cell.B)
    return (b % cell.G + b // cell.G) % cell.G


def outlier_lanes(cell, kind):
    return (np.arange(cell.B) // cell.G) % 8 == OUTLIER[kind][0]


# ---- the mission -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mission(name):
    """every input array of the C stretches of cell `name`, drawn once and fp32-representable (both record types hold exactly these
    values), read-only: prm, state (nominal, rot, P, prev), table (B, 7), rows (G, 7), trans, gate, acc / gyr (C, K_STRETCH, B, 3), the
    window frames ids (C, F, B, M) with pos, quat or left, z_depth (C, B), z_vel (C, B, 3), var_vel (B, 3), var_depth, var_rows"""
    cell = CELLS[name]
    B, G, N, M = cell.B, cell.G, cell.N, cell.M
    NG = B // G
    rep = lambda a, axis=0: np.repeat(a, G, axis=axis)
    rng = np.random.default_rng(2024 + ord(name))
    m = types.SimpleNamespace(cell=cell)
    if cell.window == "left":
        # tests/test_frame_meas_gpu.py's scene with a cleaner image: every vehicle looks at map markers from 0.6 - 1.2 m, a marker in view
        # has all four corners well inside the port's view (util.pixel_scene), the state stands 4 mm beside the truth
        m.prm = capi.default_params(cell.dialect)
        m.prm.marker_size = SIZE
        # r_pix = (1e-2)^2: the first update then shrinks the 1 cm prior by about ten, not by a thousand.  At the default 1e-6 the oracle's
        # literal (I - K H) P and its Joseph form part by 1.6e-10 of the posterior in double after the first window, the states by 3e-9,
        # and a depth residual that happens to be small turns that into 1e-8 of its nis: no free-running fp64 comparison holds there.
        m.prm.r_pix = 1e-4
        sd = cell.noise_frac * np.sqrt(m.prm.r_pix)
        nom0, _, P, prev = synth.initial_state(0, NG, list(m.prm.p0_diag), N, mixed_cov=True)
        truth, _, ids, left, _ = pixel_scene(NG, M, m.prm, SIZE, seed=61, noise=0.0, nominal=nom0)
        assert (ids[:, 0] >= 0).all()
        nom = truth.copy()
        nom[:, 0:3] += rng.normal(0, 0.004, (NG, 3))
        nom[:, 3:6] = rng.normal(0, 0.02, (NG, 3))                    # slow: the predicts must not carry the markers out of view
        nom = r32(nom)
        rot, P = r32(synth.q2R(nom[:, 6:10]).reshape(NG, 9)), r32(P)
        m.ids = rep(np.stack([np.stack([ids] * F_WIN)] * C), 2)
        m.left = rep(r32(left[None, None] + rng.normal(0, sd, (C, F_WIN) + left.shape)), 2)
    else:
        m.prm = capi.default_params(cell.dialect)
        nom, rot, P, prev = synth.initial_state(0, NG, list(m.prm.p0_diag), N, mixed_cov=True)
        nom, rot, P = r32(nom), r32(rot), r32(P)
        # one set of markers per vehicle for the whole mission (the C++ dialect's hysteresis keeps a marker only while it stays in view),
        # fresh noise in every frame
        ids, pos, quat = synth.marker_frame(0, NG, 0, M, nom, m.prm, noise=0.0)
        pos = pos[None, None] + rng.normal(0, cell.noise_frac * np.sqrt(m.prm.r_pos), (C, F_WIN) + pos.shape)
        quat = quat[None, None] + rng.normal(0, cell.noise_frac * np.sqrt(m.prm.r_quat), (C, F_WIN) + quat.shape)
        quat /= np.linalg.norm(quat, axis=-1, keepdims=True)
        m.ids = rep(np.stack([np.stack([ids] * F_WIN)] * C), 2)
        m.pos, m.quat = rep(r32(pos), 2), rep(r32(quat), 2)
    nom, rot, P, prev = rep(nom), rep(rot), rep(P), rep(prev)
    if cell.window == "nearest":
        prev = m.ids[0, 0, np.arange(B), member_of(cell) % M].astype(np.int32)       # every member holds on to a marker of its own
    m.state = (nom, rot, P, prev)
    _, _, grid_rows = noise.grid(m.prm, B, **cell.grid)
    m.rows = grid_rows[list(cell.pick)]
    assert len(m.rows) == G and all(len(set(m.rows[:, noise.COLUMNS.index(c)])) > 1 for c in cell.grid)
    m.table = m.rows[hypothesis_of(cell)]
    m.trans = noise.imm_transition(G, STAY)
    m.gate = gating.chi2_gate(GATE_PROB, max_dof(cell))
    acc, gyr = synth.imu_samples(0, NG, 0, C * K_STRETCH, nom[::G])
    m.acc = rep(r32(acc), 1).reshape(C, K_STRETCH, B, 3)
    m.gyr = rep(r32(gyr), 1).reshape(C, K_STRETCH, B, 3)
    # the readings of the built-in sensors: h(the initial state) + noise of the sensor's size, per vehicle and stretch
    st0 = tuple(x[::G] for x in m.state)
    m.var_depth, m.var_vel, m.var_rows = DEPTH.SENSOR_VAR, VELOCITY.VARS[np.arange(B) % 3].copy(), rows_ref.FIX["var"][:M_ROWS].copy()
    zd = np.stack([DEPTH.readings(st0, 64, seed=31 + c)["z"] for c in range(C)])
    rate = m.gyr[:, K_STRETCH - 2, ::G]                                # the rate sample in front of the velocity update
    zv = np.stack([VELOCITY.readings(st0, 64, rate[c], seed=43 + c)["z"] for c in range(C)])
    zd, zv = rep(zd, 1), rep(zv, 1)
    zd[:, outlier_lanes(cell, "depth")] += OUTLIER["depth"][1]
    zv[:, outlier_lanes(cell, "velocity"), 1] += OUTLIER["velocity"][1]
    m.z_depth, m.z_vel = r32(zd), r32(zv)
    return frozen(m)


def imu_slices(c_stage):
    """stage -> (first sample, count) inside a stretch: "frame0" .. "frame2", "depth", "velocity", "rows\""""
    out, k = {}, 0
    for f, K in enumerate(KCOUNT):
        out[f"frame{f}"] = (k, K); k += K
    for kind, K in zip(KINDS, K_SENSOR):
        out[kind] = (k, K); k += K
    return out[c_stage]


def rows_inputs(cell, st, dtype, c):
    """(res (B, 2), H (B, 2, N)) in the record type: the first two rows of rows_ref.fix_inputs at the state st, member by member (every
    member of a vehicle gets the same draw of the fix's noise), the outlier added"""
    G, t = cell.G, F.ft(dtype)
    res, H = np.empty((cell.B, M_ROWS), t), np.empty((cell.B, M_ROWS, cell.N), t)
    for g in range(G):
        r, h = rows_ref.fix_inputs(tuple(x[g::G] for x in st), dtype, cell.N, seed=51 + c)
        res[g::G], H[g::G] = r[:, :M_ROWS], h[:, :M_ROWS]
    res[outlier_lanes(cell, "rows"), 0] += t(OUTLIER["rows"][1])
    return res, H


def log_prior(cell):
    return np.full(cell.B, -np.log(cell.G))


# ---- the reference -------------------------------------------------------------------------------------------------------------------------------
def _engines(cell, m, joseph, mutation):
    """one oracle and one parameter set per hypothesis: row k of the table (the wrong-member mutation: one column from the row of the next
    member, (k + 1) % G)"""
    engs, prms = [], []
    for g in range(cell.G):
        row = m.rows[g].copy()
        if mutation == "wrong_member":
            col = noise.COLUMNS.index(cell.wrong)
            row[col] = m.rows[(g + 1) % cell.G][col]
        prm = with_row(m.prm, row)
        eng = OracleEngine(cell.B // cell.G, cell.dialect, cell.N, 1 if joseph else 0)
        for i in range(4):
            eng.orc.prm.q_diag[i] = prm.q_diag[i]
        eng.orc.prm.r_pos, eng.orc.prm.r_quat = prm.r_pos, prm.r_quat
        engs.append(eng); prms.append(prm)
    return engs, prms


def run_ref(name, dtype=64, state=None, logc=None, joseph=False, mutation=None, seeds=None, rows_in=None, quantise=False, stretches=C):
    """The mission of cell `name` through the composed fp64 reference -> a list of one dict per stretch:
        window, depth, velocity, rows   dict(state, applied[, nis, dof]) behind that stage
        sums (ll, rows, applied, rejected), ll_bound {32:, 64:}, logw, fuse dict(weight, best, nominal, P, pdiag),
        mix dict(weight, logc, state), count {kind: (applied, rejected)}
    dtype: the record type the rows update's inputs are formed in when rows_in is None.  state, logc: the start (default: the mission's
    state, the uniform prior).  seeds: per stretch a dict that re-seeds the reference -- "state", "logc" at the start of the stretch,
    "premix" (state) and "logw" in front of fuse and mix; each may be missing.  rows_in: per stretch (res, H) as the device got them.
    quantise: the records rounded to fp32 after every step (support.round_records: the floor of util.assert_window_parity).
    mutation: one of MUTATIONS, the slips the comparison must see."""
    cell, m = CELLS[name], mission(name)
    B, G, N = cell.B, cell.G, cell.N
    assert mutation is None or mutation in MUTATIONS
    engs, prms = _engines(cell, m, joseph, mutation)
    st = [np.array(x, np.float64 if i < 3 else np.int32) for i, x in enumerate(state if state is not None else m.state)]
    logc = np.array(log_prior(cell) if logc is None else logc, np.float64)
    thr = m.gate
    sums = [np.zeros(B), np.zeros(B, np.int64), np.zeros(B, np.int32), np.zeros(B, np.int32)]
    cpp = cell.dialect == 1
    mode = capi.MODE_NEAREST if cell.window == "nearest" else capi.MODE_STACKED
    q = (lambda: round_records(*st[:3])) if quantise else (lambda: None)

    hyp = hypothesis_of(cell)

    def each_member(fn):
        for g in range(G):
            who = np.nonzero(hyp == g)[0]
            engs[g].set_state(*(x[who] for x in st))
            fn(g, engs[g], who)
            for x, y in zip(st, engs[g].get_state()):
                x[who] = y

    def predict(c, first, K):
        for k in range(first, first + K):
            each_member(lambda g, eng, who: eng.predict(m.acc[c, k, who], m.gyr[c, k, who], DT))
            q()

    def frame(c, f, bound):
        applied = np.zeros(B, np.uint8)

        def one(g, eng, who):
            pre = eng.get_state()
            ids = m.ids[c, f, who]
            if cell.window == "left":
                app = eng.orc.correct_pixels(eng.nominal, eng.rot, eng.P, eng.prev, ids, m.left[c, f, who], None, SIZE, prms[g].r_pix,
                                                 analytic=True)          # (the central-difference oracle is good to 1e-7 only)
            else:
                app = eng.correct(ids, m.pos[c, f, who], m.quat[c, f, who], mode)
            applied[who] = app
            for k, b in enumerate(who):
                if not app[k]:
                    continue
                if cell.window == "left":
                    # dense_pixels takes its rotation from the quaternion; the update linearises with the CARRIED rotation, which an
                    # earlier update's injection and the mix leave behind the quaternion: hand it the carried rotation's quaternion
                    at = pre[0][k].copy()
                    at[6:10] = synth.R2q(pre[1][k].reshape(3, 3))
                    nr, ld, nrow, _ = dense_pixels(at, pre[2][k], ids[k], m.left[c, f, b], None, prms[g], "left", r=prms[g].r_pix)
                    tol = {d: tol_m2ll(d, False, nr, ld) for d in (32, 64)}
                else:
                    used = [int(eng.prev[k])] if (cell.window == "nearest" and cpp) else [int(i) for i in ids[k] if i >= 0]
                    nr, ld, nrow, rr = dense_pose(eng.orc, pre[0][k], pre[1][k], pre[2][k], ids[k], m.pos[c, f, b], m.quat[c, f, b], used, prms[g])
                    tol = {d: tol_m2ll(d, True, nr, ld, rr) for d in (32, 64)}
                sums[0][b] += -0.5 * (nr + ld + nrow * LN2PI)
                sums[1][b] += nrow
                sums[2][b] += 1
                for d in (32, 64):
                    bound[d][b] += 0.5 * tol[d]
        each_member(one)
        q()
        return applied

    def sensor(fam, inp, bound, gated=True):
        new, app, nis, dof, lnd = fam.ref(tuple(st), N, inp, thr[fam.rows] if gated else np.inf, joseph)
        for x, y in zip(st, new):
            x[...] = y
        q()
        app = np.asarray(app, bool)
        sums[0][app] += -0.5 * (nis[app] + lnd[app] + fam.rows * LN2PI)
        sums[1][app] += fam.rows
        sums[2][app] += 1
        sums[3][(dof > 0) & ~app] += 1
        for d in (32, 64):           # one call of tests/test_sensor_suite_gpu.py: nis to NIS_TOL (relative), the rest of ll to 1e-9 + NIS_TOL
            bound[d][app] += 0.5 * F.NIS_TOL[d] * np.maximum(nis[app], 1.0) + 1e-9 + F.NIS_TOL[d]
        return dict(state=tuple(x.copy() for x in st), applied=app.astype(np.uint8), nis=nis, dof=dof), (int(app.sum()), int(((dof > 0) & ~app).sum()))

    out = []
    for c in range(stretches):
        seed = (seeds[c] if seeds is not None else {})
        if "state" in seed:
            st = [np.array(x, np.float64 if i < 3 else np.int32) for i, x in enumerate(seed["state"])]
        if "logc" in seed:
            logc = np.array(seed["logc"], np.float64)
        o = {}
        if not (mutation == "no_reset" and c > 0):
            for s in sums:
                s[...] = 0
        bound = {32: np.zeros(B), 64: np.zeros(B)}
        for f in range(F_WIN):
            predict(c, *imu_slices(f"frame{f}"))
            app = frame(c, f, bound)
        o["window"] = dict(state=tuple(x.copy() for x in st), applied=app)
        o["count"] = {}
        predict(c, *imu_slices("depth"))
        var = m.var_depth * (1.01 if mutation == "depth_var" else 1.0)
        o["depth"], o["count"]["depth"] = sensor(DEPTH, dict(z=m.z_depth[c], var=var), bound, gated=mutation != "apply_rejected")
        predict(c, *imu_slices("velocity"))
        k_rate = imu_slices("velocity")[0]
        o["velocity"], o["count"]["velocity"] = sensor(VELOCITY, dict(z=m.z_vel[c], var=m.var_vel, gyro=m.gyr[c, k_rate]), bound)
        predict(c, *imu_slices("rows"))
        res, H = rows_in[c] if rows_in is not None else rows_inputs(cell, tuple(st), dtype, c)
        o["rows_in"] = (res, H)
        o["rows"], o["count"]["rows"] = sensor(ROWS, dict(res=np.asarray(res, np.float64), H=np.asarray(H, np.float64), var=m.var_rows), bound)
        o["sums"] = tuple(s.copy() for s in sums)
        o["ll_bound"] = bound
        o["logw"] = sums[0].copy() if mutation == "no_logc" else logc + sums[0]
        if "premix" in seed:
            st = [np.array(x, np.float64 if i < 3 else np.int32) for i, x in enumerate(seed["premix"])]
        logw = np.array(seed["logw"], np.float64) if "logw" in seed else o["logw"]
        w, best, fnom, fP = group_ref.fuse(st[0], st[2], logw, G)
        o["fuse"] = dict(weight=w, best=best, nominal=fnom, P=fP, pdiag=np.einsum("bii->bi", fP).copy())
        w, logc, nom, rot, P = group_mix_ref.mix(tuple(st), logw, m.trans, G)
        chart = np.repeat(np.arange(B // G) * G + np.maximum(best, 0), G)
        prev = st[3].copy()
        if mutation == "rot_own":                 # every target keeps the carried rotation of its own record
            rot = st[1].copy()
        if mutation == "prev_chart":              # every target takes the chart member's prev_id
            prev = st[3][chart]
        if mutation == "no_spread":               # the mix of members that all sit at the chart: sum_i W_ij P_i alone
            P = group_mix_ref.mix((st[0][chart], st[1], st[2], st[3]), logw, m.trans, G)[4]
        st = [nom, rot, P, prev]
        q()
        o["mix"] = dict(weight=w, logc=logc.copy(), state=tuple(x.copy() for x in st))
        out.append(o)
    return out


# ---- the comparison ------------------------------------------------------------------------------------------------------------------------------
RECORD_STAGES = ("window", "depth", "velocity", "rows")


def record_gates(cell, dtype, floor=None):
    """fp64: the single-step gates of util.assert_parity; fp32: the gates of util.assert_window_parity, floor-relative where a floor is
    given"""
    if dtype == 64:
        return dict(literal=F64_TOL, sigma=F64_TOL, plain=F64_TOL, rot=F64_TOL, cov=F64_TOL, cov_block=COV_BLOCK_TOL_F64)
    std = dict(literal=window_literal_tol(cell.dialect, cell.N), sigma=WINDOW_TOL, plain=PLAIN_WINDOW_TOL, cov=COV_TOL, cov_block=WINDOW_COV_BLOCK_TOL)
    return {k: max(v, FLOOR_FACTOR * (floor or {}).get(k, 0.0)) for k, v in std.items()}


def group_gates(dtype):
    """tests/test_group_mix_gpu.py::_gates / _hold"""
    st, cv, cb = (F64_TOL, F64_TOL, COV_BLOCK_TOL_F64) if dtype == 64 else (STATE_TOL, COV_TOL, COV_BLOCK_TOL)
    return dict(literal=min(st, STATE_TOL), sigma=st, cov=cv, cov_block=cb)


def _hold_rows(what, got_nom, got_P, ref_nom, ref_P, dtype):
    g = group_gates(dtype)
    e = dict(literal=state_rel_err_literal(got_nom, ref_nom), sigma=state_rel_err(got_nom, ref_nom, ref_P)[0],
             cov=cov_rel_err(got_P, ref_P), cov_block=cov_rel_err_blockwise(got_P, ref_P))
    return [(what, k, e[k], g[k]) for k in g]


def _exact(what, name, a, b):
    a, b = np.asarray(a), np.asarray(b)
    return (what, name, float((a != b).sum()) if a.shape == b.shape else float("inf"), 0.0)


def compare(name, got, ref, dtype, seeded=False, floors=None):
    """every compared output of the mission as rows (stage, figure, error, gate): got / ref = lists of stretch dicts as run_ref returns
    them (a device run holds the same keys).  seeded=False: the free-running comparison, the records behind every stage under the
    single-step gates.  seeded=True: the reference was re-seeded per stretch and in front of the mix -- the records at the end of the
    stretch under the window gates (floors: per stretch the fp32-record floor, or None), nothing in between.  Integers are exact
    (error = the number of entries that differ, gate 0)."""
    cell = CELLS[name]
    rows = []
    for c, (g, r) in enumerate(zip(got, ref)):
        for stage in (("rows",) if seeded else RECORD_STAGES):
            what = f"{c} {stage}"
            e = parity_errors(g[stage]["state"], r[stage]["state"])
            gates = record_gates(cell, dtype, (floors or {}).get(c) if seeded else None)
            rows += [(what, k, e[k], gates[k]) for k in gates]
            rows += [(what, "asym", e["asym"], 0.0), _exact(what, "prev", g[stage]["state"][3], r[stage]["state"][3])]
        for stage in RECORD_STAGES:
            what = f"{c} {stage}"
            rows.append(_exact(what, "applied", g[stage]["applied"], r[stage]["applied"]))
            if "nis" in r[stage]:
                rows.append(_exact(what, "dof", g[stage]["dof"], r[stage]["dof"]))
            if "nis" in r[stage] and not seeded:             # (one call's tolerance: behind a free-running fp32 window it has no meaning)
                on = np.asarray(r[stage]["dof"]) > 0
                rows.append((what, "nis", float(F.rel(np.asarray(g[stage]["nis"], np.float64)[on], r[stage]["nis"][on]).max()), F.NIS_TOL[dtype]))
        what = f"{c} sums"
        for k, nm in ((1, "rows"), (2, "applied"), (3, "rejected")):
            rows.append(_exact(what, nm, g["sums"][k], r["sums"][k]))
        bound = r["ll_bound"][dtype]
        rows.append((what, "ll / bound", float((np.abs(g["sums"][0] - r["sums"][0]) / bound).max()), 1.0))
        rows.append((what, "logw / bound", float((np.abs(g["logw"] - r["logw"]) / bound).max()), 1.0))
        what = f"{c} fuse"
        rows.append(_exact(what, "best", g["fuse"]["best"], r["fuse"]["best"]))
        rows.append((what, "weight", float(np.abs(g["fuse"]["weight"] - r["fuse"]["weight"]).max()), 1e-12))
        rows += _hold_rows(what, g["fuse"]["nominal"], g["fuse"]["P"], r["fuse"]["nominal"], r["fuse"]["P"], dtype)
        rows.append((what, "pdiag", float(np.abs(np.asarray(g["fuse"]["pdiag"], np.float64) - np.einsum("bii->bi", np.asarray(g["fuse"]["P"], np.float64))).max()), 0.0))
        what = f"{c} mix"
        rows.append((what, "weight", float(np.abs(g["mix"]["weight"] - r["mix"]["weight"]).max()), 1e-12))
        assert np.isfinite(r["mix"]["logc"]).all()
        rows.append((what, "logc", float(np.abs(g["mix"]["logc"] - r["mix"]["logc"]).max()), 1e-12))
        gs, rs = g["mix"]["state"], r["mix"]["state"]
        rows += _hold_rows(what, gs[0], gs[2], rs[0], rs[2], dtype)
        rows.append((what, "rot", float(np.abs(np.asarray(gs[1], np.float64) - rs[1]).max()), 0.0 if seeded else F64_TOL))
        P = np.asarray(gs[2])
        rows += [(what, "asym", float(np.abs(P - np.swapaxes(P, 1, 2)).max()), 0.0), _exact(what, "prev", gs[3], rs[3])]
    return rows


def worst(rows):
    """the row with the largest error / gate (an exact figure that differs counts as infinite)"""
    ratio = lambda r: (np.inf if r[2] > 0 else 0.0) if r[3] == 0 else r[2] / r[3]
    w = max(rows, key=ratio)
    return ratio(w), w


def failing(rows):
    return [r for r in rows if not r[2] <= r[3]]


def seeds_of(run):
    """the seeds that restart a reference from `run` (a device run, or a reference run standing in for one): its state and logc at the start of
    every stretch but the first, its state and logw in front of every mix"""
    seeds = []
    for c, o in enumerate(run):
        s = dict(premix=o["rows"]["state"], logw=o["logw"])
        if c > 0:
            s.update(state=run[c - 1]["mix"]["state"], logc=run[c - 1]["mix"]["logc"])
        seeds.append(s)
    return seeds
