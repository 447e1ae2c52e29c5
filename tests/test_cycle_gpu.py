"""GPU suite: the IMM cycle end to end -- the loop include/fbus_ekf.h closes its hypothesis-group section with -- as the mission of
tests/cycle_ref.py: small banks through three full cycles (loglik_reset, a frame window, depth, velocity and rows updates between
predicts, the sums, group_fuse, group_mix, logc fed back) on a tabled, gated, sums-on handle, against the fp64 reference composed of
the suite's own restatements.  What one entry point leaves behind for the next is what is under test: the chart's carried rotation in
the Matlab dialect's predict, every member's own prev_id in the C++ dialect's hysteresis, the sums across a reset, the counters over
four kinds of update, logc through a second and third mix.  tests/test_cycle_cpu.py holds the conditions that make this meaningful.

  1  fp64 records, free-running: device and reference run the whole mission from the same state.  Two arrays go to the reference as
     the device formed them, because they are INPUTS of a call that both sides must receive identically: res and H of the rows update,
     and logw of group_fuse / group_mix (the weights are held to the 1e-12 of one call; logw itself is held to the ll bound).
  2  fp32 records: the reference restarts from the device's state and logc at every stretch and from its state in front of the mix.
  3  equal bits: window = its frames, host = _dev, a second run, the groups in reverse order, the sensor updates on a plain handle.
  4  what a call must not touch."""
import functools
import time

import numpy as np
import pytest
import torch

import cycle_ref as R
from fbus_ekf import BatchedFilter, capi
from support import DT, fp32_record_floor, same_rows, same_state, to_device
from util import assert_window_parity

pytestmark = pytest.mark.gpu

CASES = [pytest.param(n, d, id=f"{n}-{d}") for n in ("A", "B", "C") for d in (32, 64)]


def _np(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def reversed_groups(cell):
    """position -> filter: the vehicles in reverse order, every group's members in their own order"""
    j, g = np.arange(cell.B) // cell.G, np.arange(cell.B) % cell.G
    return (cell.B // cell.G - 1 - j) * cell.G + g


def run_dev(name, dtype, form="dev", window=True, order=None, probe=False):
    """the mission on a device handle -> the stretch dicts of cycle_ref.run_ref (+ "before": the state in front of each sensor update,
    "probe": with probe=True what must not be touched, around every reset, fuse and mix).  form "dev": device arrays and the window entry point (window=False: the
    same frames one by one, predict_n + the per-call update); "host": the host-pointer form of every call.  order: position -> filter of
    the mission (None: as drawn); every output comes back in the mission's own order."""
    cell, m = R.CELLS[name], R.mission(name)
    B, G, N = cell.B, cell.G, cell.N
    NG = B // G
    sel = np.arange(B) if order is None else np.asarray(order)
    inv = np.argsort(sel)
    vsel = sel[::G] // G                                            # position -> vehicle
    vinv = np.argsort(vsel)
    npd = np.float32 if dtype == 32 else np.float64
    host = form == "host"
    put = (lambda a, dt=npd: np.ascontiguousarray(a, dt)) if host else (lambda a, dt=npd: to_device(np.ascontiguousarray(a), dt))
    mode = capi.MODE_NEAREST if cell.window == "nearest" else capi.MODE_STACKED
    out = []
    with BatchedFilter(B, m.prm, device=0, dtype=dtype, nstate=N) as f:
        f.set_state(*(x[sel] for x in m.state))
        f.set_noise(m.table[sel])
        f.set_gate(m.gate)
        f.loglik_enable(True)
        R.DEPTH.set_sensor(f)
        R.VELOCITY.set_sensor(f)
        logc = R.log_prior(cell)[sel]

        def state():
            f.sync()
            return tuple(x[inv] for x in f.get_state())

        def snap():
            return dict(zip(("nominal", "rot", "P", "prev"), f.get_state()), applied=f.applied(), noise=f.get_noise(),
                        **dict(zip(("ll", "rows", "napp", "nrej"), f.loglik())))

        def predict(c, first, K):
            if K:
                f.predict_n(put(m.acc[c, first:first + K][:, sel]), put(m.gyr[c, first:first + K][:, sel]), put(np.full(K, DT[0])), K=K)

        def update(c, fr):
            ids = put(m.ids[c, fr][sel], np.int32)
            if cell.window == "left":
                f.correct_pixels(ids, put(m.left[c, fr][sel]), None)
            else:
                f.correct(ids, put(m.pos[c, fr][sel]), put(m.quat[c, fr][sel]), mode)

        def sensor(o, kind, call):
            o_k = dict(before=state())
            nis, dof = call()
            f.sync()
            o_k.update(state=state(), applied=f.applied()[inv], nis=_np(nis).astype(np.float64)[inv], dof=_np(dof)[inv])
            o[kind] = o_k

        for c in range(R.C):
            o, pr = {}, {}
            if probe:
                pr["pre_reset"] = snap()
            f.loglik_reset()
            if probe:
                pr["post_reset"] = snap()
            if window and not host:
                Kw = sum(R.KCOUNT)
                imu = (put(m.acc[c, :Kw][:, sel]), put(m.gyr[c, :Kw][:, sel]), put(np.full(Kw, DT[0])))
                ids = put(m.ids[c][:, sel], np.int32)
                if cell.window == "left":
                    f.frames_meas(list(R.KCOUNT), *imu, ids, put(m.left[c][:, sel]), None)
                else:
                    f.frames(list(R.KCOUNT), *imu, ids, put(m.pos[c][:, sel]), put(m.quat[c][:, sel]), mode)
            else:
                for fr in range(R.F_WIN):
                    predict(c, *R.imu_slices(f"frame{fr}"))
                    update(c, fr)
            o["window"] = dict(state=state(), applied=f.applied()[inv])
            predict(c, *R.imu_slices("depth"))
            sensor(o, "depth", lambda: f.correct_depth_nis(put(m.z_depth[c][sel]), m.var_depth))
            predict(c, *R.imu_slices("velocity"))
            k_rate = R.imu_slices("velocity")[0]
            sensor(o, "velocity", lambda: f.correct_velocity_nis(put(m.z_vel[c][sel]), put(m.var_vel[sel], np.float64),
                                                                 put(m.gyr[c, k_rate][sel])))
            predict(c, *R.imu_slices("rows"))
            res, H = R.rows_inputs(cell, state(), dtype, c)              # (formed in the mission's order, handed over in the handle's)
            o["rows_in"] = (res, H)
            sensor(o, "rows", lambda: f.correct_rows_nis(put(res[sel]), put(H[sel]), np.array(m.var_rows)))
            sums = f.loglik()
            o["sums"] = tuple(x[inv] for x in sums)
            logw = logc + sums[0]
            o["logw"] = logw[inv]
            if probe:
                pr["pre_fuse"] = snap()
            if host:
                tt = npd
                fu = (np.zeros(B), np.zeros(NG, np.int32), np.zeros((NG, 19), tt), np.zeros((NG, N, N), tt), np.zeros((NG, N), tt))
                f._check(f._lib.fbus_ekf_group_fuse(f._h, G, f._p(logw), *(f._p(x) for x in fu)), "group_fuse")
            else:
                fu = f.group_fuse(G, logw)
                f.sync()
                fu = tuple(_np(x) for x in fu)
            o["fuse"] = dict(weight=fu[0][inv], best=fu[1][vinv], nominal=fu[2][vinv], P=fu[3][vinv], pdiag=fu[4][vinv])
            if probe:
                pr["post_fuse"] = snap()
            if host:
                w, lc = np.zeros(B), np.zeros(B)
                f._check(f._lib.fbus_ekf_group_mix(f._h, G, f._p(logw), f._p(np.ascontiguousarray(m.trans)), f._p(w), f._p(lc)), "group_mix")
            else:
                w, lc = f.group_mix(G, np.array(m.trans), logw)
                f.sync()
                w, lc = _np(w), _np(lc)
            logc = lc
            o["mix"] = dict(weight=w[inv], logc=lc[inv], state=state())
            if probe:
                pr["post_mix"] = snap()
                o["probe"] = pr
            out.append(o)
        if probe:                                                       # after the last cycle: collapse onto `best`
            before = f.get_state()
            f.group_collapse(G, fu[1])
            out.append(dict(collapsed=f.get_state(), best=fu[1], before=before))
    return out


@functools.lru_cache(maxsize=None)
def dev_run(name, dtype):
    t = time.time()
    out = run_dev(name, dtype)
    print(f"[cycle] cell {name} fp{dtype}: the mission on the device in {time.time() - t:.2f} s")
    return out


def flat(run):
    """every per-filter and per-group output of a run as name -> array, for bit comparisons"""
    d = {}
    for c, o in enumerate(run[:R.C]):
        for stage in R.RECORD_STAGES:
            for k, v in zip(("nominal", "rot", "P", "prev"), o[stage]["state"]):
                d[f"{c} {stage} {k}"] = v
            for k in ("applied", "nis", "dof"):
                if k in o[stage]:
                    d[f"{c} {stage} {k}"] = o[stage][k]
        for k, v in zip(("ll", "rows", "napp", "nrej"), o["sums"]):
            d[f"{c} sums {k}"] = v
        d[f"{c} logw"] = o["logw"]
        for k, v in o["fuse"].items():
            d[f"{c} fuse {k}"] = v
        d[f"{c} mix weight"], d[f"{c} mix logc"] = o["mix"]["weight"], o["mix"]["logc"]
        for k, v in zip(("nominal", "rot", "P", "prev"), o["mix"]["state"]):
            d[f"{c} mix {k}"] = v
    return d


def show(name, dtype, rows, what):
    """the stage maxima against their gates, one line per figure: the largest error / gate over the stretches"""
    worst = {}
    for stage, fig, err, gate in rows:
        key = (stage.split()[1], fig)
        r = (np.inf if err > 0 else 0.0) if gate == 0 else err / gate
        if key not in worst or r > worst[key][0]:
            worst[key] = (r, err, gate, stage)
    for (stage, fig), (r, err, gate, where) in worst.items():
        print(f"[cycle] cell {name} fp{dtype} {what}: {stage:9s} {fig:13s} {err:.3e} against {gate:.1e} (stretch {where.split()[0]})")


def mutation_factors(name, dtype, dev, seeded):
    """how far the device stands from every mutated reference, in units of the gate (gated figures; exact ones that differ count as inf):
    cells A and B (a reference run of cell C takes 8 s, tests/test_cycle_cpu.py has its factors)"""
    if name == "C":
        print(f"[cycle] cell C fp{dtype}: no mutated references here (8 s each); tests/test_cycle_cpu.py has the factors of the cells A and B")
        return
    rows_in = [o["rows_in"] for o in dev]
    for mut, where in R.MUTATIONS.items():
        if where not in ("any", name):
            continue
        seeds = R.seeds_of(dev) if seeded else [dict(logw=o["logw"]) for o in dev]
        ref = R.run_ref(name, dtype, mutation=mut, seeds=seeds, rows_in=rows_in)
        f, w = R.worst(R.compare(name, dev, ref, dtype, seeded=seeded))
        print(f"[cycle] cell {name} fp{dtype}: device against the reference with {mut}: {f:.3g} x the gate ({w[0]}: {w[1]})")
        assert f >= (10 if dtype == 32 else 100)


# ---- 1. fp64 records, free-running -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_fp64_mission_free_running(name):
    dev = dev_run(name, 64)
    t = time.time()
    ref = R.run_ref(name, 64, rows_in=[o["rows_in"] for o in dev], seeds=[dict(logw=o["logw"]) for o in dev])
    print(f"[cycle] cell {name} fp64: the reference in {time.time() - t:.2f} s")
    rows = R.compare(name, dev, ref, 64)
    show(name, 64, rows, "free-running")
    assert not R.failing(rows), R.failing(rows)
    mutation_factors(name, 64, dev, seeded=False)


# ---- 2. fp32 records, re-seeded per stretch ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_fp32_mission_reseeded_per_stretch(name):
    cell = R.CELLS[name]
    dev = dev_run(name, 32)
    kw = dict(rows_in=[o["rows_in"] for o in dev], seeds=R.seeds_of(dev))
    t = time.time()
    both = {False: R.run_ref(name, 32, **kw)}
    floors = {}
    if name == "C":                                                  # the fp32-record floor, as tests/test_frame_meas_gpu.py computes it
        both[True] = R.run_ref(name, 32, quantise=True, **kw)
        for c in range(R.C):
            _, floors[c] = fp32_record_floor(lambda q, c=c: both[q][c]["rows"]["state"])
    ref = both[False]
    print(f"[cycle] cell {name} fp32: the reference{' and its fp32-record twin' if floors else ''} in {time.time() - t:.2f} s")
    rows = R.compare(name, dev, ref, 32, seeded=True, floors=floors)
    show(name, 32, rows, "re-seeded")
    for c in range(R.C):
        assert_window_parity(dev[c]["rows"]["state"], ref[c]["rows"]["state"], f"cell {name} stretch {c}: 9 predicts and 6 updates", cell.dialect, cell.N,
                             floor=floors.get(c))
    assert not R.failing(rows), R.failing(rows)
    mutation_factors(name, 32, dev, seeded=True)


# ---- 3. equal bits -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,dtype", CASES)
def test_equal_bits(name, dtype):
    cell = R.CELLS[name]
    first = flat(dev_run(name, dtype))
    # the window entry point = its frames one by one (the header's promise while the sums are on); the host-pointer form of every call
    # = the _dev form; a second run = the first; the groups in reverse order: every group the bits it had
    for what, kw in (("frames one by one", dict(window=False)), ("host forms", dict(form="host")), ("second run", {}),
                     ("groups reversed", dict(order=reversed_groups(cell)))):
        assert same_rows(first, flat(run_dev(name, dtype, **kw))), what
    # the three sensor updates of stretch 0 on the tabled, sums-on handle = the same calls on a plain handle (no table, no sums) given
    # the state the tabled handle holds in front of each: the header's "do not enter"
    m, o = R.mission(name), dev_run(name, dtype)[0]
    npd = np.float32 if dtype == 32 else np.float64
    k_rate = R.imu_slices("velocity")[0]
    res, H = o["rows_in"]
    calls = {"depth": lambda f: f.correct_depth_nis(m.z_depth[0].astype(npd), m.var_depth),
             "velocity": lambda f: f.correct_velocity_nis(m.z_vel[0].astype(npd), m.var_vel, m.gyr[0, k_rate].astype(npd)),
             "rows": lambda f: f.correct_rows_nis(res, H, m.var_rows)}
    with BatchedFilter(cell.B, m.prm, device=0, dtype=dtype, nstate=cell.N) as f:
        f.set_gate(m.gate)
        R.DEPTH.set_sensor(f)
        R.VELOCITY.set_sensor(f)
        for kind in R.KINDS:
            f.set_state(*o[kind]["before"])
            nis, dof = calls[kind](f)
            assert same_state(f.get_state(), o[kind]["state"]), kind
            assert np.array_equal(f.applied(), o[kind]["applied"]) and np.array_equal(dof, o[kind]["dof"]), kind
            assert np.array_equal(nis.astype(np.float64), o[kind]["nis"]), kind
            assert 0 < o[kind]["applied"].sum() < cell.B


# ---- 4. what a call must not touch ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,dtype", CASES)
def test_what_a_call_must_not_touch(name, dtype):
    cell, m = R.CELLS[name], R.mission(name)
    run = run_dev(name, dtype, probe=True)
    records = ("nominal", "rot", "P", "prev")
    for c, o in enumerate(run[:R.C]):
        p = o["probe"]
        # loglik_reset: the records and the flags as they were, the sums zero
        assert same_rows({k: p["pre_reset"][k] for k in records + ("applied", "noise")}, p["post_reset"]), c
        assert all((p["post_reset"][k] == 0).all() for k in ("ll", "rows", "napp", "nrej")), c
        assert c == 0 or (p["pre_reset"]["napp"] >= R.F_WIN).all()        # (there was something to reset)
        # group_fuse: nothing but its outputs
        assert same_rows(p["pre_fuse"], p["post_fuse"]), c
        # group_mix: the flags, the four sums and the table (the records are what it rewrites)
        keep = ("applied", "noise", "ll", "rows", "napp", "nrej", "prev")
        assert same_rows({k: p["post_fuse"][k] for k in keep}, p["post_mix"]), c
        assert not np.array_equal(p["post_fuse"]["nominal"], p["post_mix"]["nominal"])
        assert np.array_equal(p["post_mix"]["noise"], m.table)
    # after the last cycle group_collapse(G, best) makes every member's record the best member's, bit for bit
    end = run[-1]
    src = np.repeat(np.arange(cell.B // cell.G) * cell.G + end["best"], cell.G)
    assert (end["best"] >= 0).all()
    assert same_state(end["collapsed"], tuple(x[src] for x in end["before"]))
    assert not np.array_equal(end["collapsed"][0], end["before"][0])
