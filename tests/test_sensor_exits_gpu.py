"""Every streamed sensor kernel through every exit: the 20 separately compiled code objects of csrc/ekf_depth.hpp, csrc/ekf_velocity.hpp
and csrc/ekf_rows.hpp -- depth and velocity (fp32, fp64) x (N = 18, 15), rows (fp32, fp64) x (N = 18, 15) x (m = 1, 2, 3) -- each with ONE
gated call (the _nis form, the likelihood sums on) whose 321 lanes follow tests/exits_plan.py: a wave that leaves whole at the untouched
branch, one that leaves whole at the gate, three tiles in which skipped, unusable, rejected, broken-record and applied lanes sit side by
side, and a tail tile of one applied lane.  The threshold comes from the fp64 restatement's nis, in a gap wide enough that the device's
partition must be the restatement's, lane for lane.  A second call on a fresh, identical handle under a gate table whose every other
entry is 0 holds each kernel to thr[its own row count].

Measured on an MI355X, maxima over each case's lanes: in the docstrings of the three tests."""
import numpy as np
import pytest
import torch

import exits_plan as X
from sensor_families import NAMES
from support import same_rows
from util import assert_parity

pytestmark = pytest.mark.gpu

LN2PI = float(np.log(2 * np.pi))


def named(st):
    return dict(zip(NAMES, st))


def raw_records(f):
    """(bytes of the packed records on the host, bytes per filter): fbus_ekf_copy_records into a device buffer, as
    tests/test_trajectory_gpu.py reads them"""
    _, bpf, tot = f.records()
    t = torch.empty(tot, dtype=torch.uint8, device="cuda:0")
    f.copy_records(t)
    f.sync()
    return t.cpu().numpy(), bpf


def lanes_of(raw, bpf):
    """the record bytes, one row per lane: a tile is bpf / 16 chunks of 64 lanes x 16 bytes (csrc/ekf_kernels.hpp, tile_rsrc and
    load_chunks: the tile's bytes start at tile x NCH x 1024, chunk c of lane l at c x 1024 + l x 16; bpf = NCH x 16)"""
    nch = bpf // 16
    return raw.reshape(-1, nch, X.TILE, 16).transpose(0, 2, 1, 3).reshape(-1, bpf)


def fresh(fam, dtype, n, state):
    """a handle of the family's construction holding exactly `state`; -> (handle, the state as it reads back, its raw bytes)"""
    f = fam.handle(X.B, dtype, n, X.DIALECT[n])[0]
    f.set_state(*state)
    before = f.get_state()
    assert same_rows(named(state), named(before))                    # the restatement runs on what the records hold
    raw, bpf = raw_records(f)
    return f, before, raw, bpf


def run_case(name, dtype, n, m):
    fam = X.family(name, m)
    rows, what = fam.rows, f"{X.family(name, m)} f{dtype} N={n}"
    f, st0, aux = fam.handle(X.B, dtype, n, X.DIALECT[n])
    f.close()
    case = X.prepare(fam, st0, dtype, n, aux)
    X.reference_conditions(fam, case)                                # 1. the plan, the threshold's gap, the reference's own partition
    kinds, inp, thr = case.kinds, case.inp, case.thr
    b = np.arange(X.B)
    usable = X.usable_kind(kinds)
    r_state, r_app, r_nis, r_dof, r_lnd = case.gated
    r_app = r_app.astype(bool)

    # ---- the one gated call --------------------------------------------------------------------------------------------------------------
    f, before, raw0, bpf = fresh(fam, dtype, n, case.state)
    with f:
        assert bpf % 16 == 0 and len(raw0) == 6 * X.TILE * bpf      # six tiles of 64 records, the last one padded
        f.set_gate(X.gate_only(rows, thr))
        f.loglik_enable()
        assert all((x == 0).all() for x in f.loglik())
        nis, dof = fam.call(f, inp, "nis")
        got, app = f.get_state(), f.applied().astype(bool)
        raw1, _ = raw_records(f)
        ll, lrows, lapp, lrej = f.loglik()
    nis64 = nis.astype(np.float64)
    assert np.array_equal(app, r_app), (what, np.nonzero(app != r_app)[0])                      # 2. the partition, lane for lane
    assert np.array_equal(dof, rows * usable.astype(np.int32)), what                            # 3. dof
    assert (nis[~usable] == 0).all() and np.isnan(nis[kinds == X.NAN_REC]).all(), what          # 4. nis where there is none
    fin = usable & np.isfinite(r_nis)
    assert np.array_equal(fin, usable & (kinds != X.NAN_REC))
    e_nis = np.abs(nis64[fin] - r_nis[fin]) / np.abs(r_nis[fin])
    print(f"[exits] {what}: thr[{rows}] = {thr:.6g} (gap half-width {case.half:.2e}), applied {int(app.sum())}, rejected by the gate "
          f"{int(((kinds == X.CLEAN) & ~app).sum())}, nis rel err {e_nis.max():.3e}")
    assert e_nis.max() <= X.NIS_TOL[dtype], (what, e_nis.max())                                  # 5. nis of every usable lane
    sel = np.nonzero(app)[0]
    assert_parity([x[sel] for x in got], [x[sel] for x in r_state], dtype, f"[exits] {what}: the applied lanes")          # 6.
    rest = np.nonzero(~app)[0]
    assert same_rows(named(before), named(got), rest, rest), what                                # 7. not applied: the state before, bit for bit
    assert same_rows({k: named(before)[k] for k in ("rot", "prev")}, {k: named(got)[k] for k in ("rot", "prev")}), what          # 8.
    if n == 15:
        assert np.array_equal(got[0][sel, 16:19], before[0][sel, 16:19]), what
    assert not np.array_equal(got[0][sel], before[0][sel]) and not np.array_equal(got[2][sel], before[2][sel])          # (they did move)
    Pg = got[2][kinds != X.NAN_REC]
    assert np.array_equal(Pg, np.swapaxes(Pg, 1, 2)), what                                       # 9. exactly symmetric
    # 10. the raw bytes, padding and the chunks that hold only the rotation included: the two whole-wave tiles as ranges of the buffer,
    # every lane that is not applied through the tile's layout, and the padding records behind lane 320
    t0, t1 = X.TILE * bpf, 2 * X.TILE * bpf
    assert np.array_equal(raw0[t0:t1], raw1[t0:t1]) and np.array_equal(raw0[3 * t0:4 * t0], raw1[3 * t0:4 * t0]), what
    l0, l1 = lanes_of(raw0, bpf), lanes_of(raw1, bpf)
    assert np.array_equal(l0[rest], l1[rest]) and np.array_equal(l0[X.B:], l1[X.B:]), what
    assert (l0[sel] != l1[sel]).any(axis=1).all()
    # 11. the likelihood counters
    assert np.array_equal(lrows, rows * app.astype(np.int64)) and np.array_equal(lapp, app.astype(np.int32)), what
    assert np.array_equal(lrej, (usable & ~app).astype(np.int32)), what
    assert lrej[kinds == X.NAN_REC].all() and lrej[kinds == X.NEG_COV].all() and not lrej[~usable].any()
    # 12. ll: the device's nis, the reference's ln det S
    want = -0.5 * (nis64[app] + r_lnd[app] + rows * LN2PI)
    e_ll = np.abs(ll[app] - want).max()
    print(f"[exits] {what}: max |ll - (-1/2)(nis + ln det S + {rows} ln 2 pi)| = {e_ll:.3e}")
    assert e_ll <= 1e-9 + X.NIS_TOL[dtype], (what, e_ll)
    assert (ll[~app] == 0).all(), what

    # ---- the wrong-entry check: thr[rows] = +inf, every other entry 0, against a handle without a table ---------------------------------
    outs = {}
    for table in ("wrong entries", "none"):
        f, again, raw, _ = fresh(fam, dtype, n, case.state)
        with f:
            assert np.array_equal(raw, raw0)                          # a fresh, identical handle
            if table == "wrong entries":
                f.set_gate(X.gate_wrong_entries(rows))
            nis_w, dof_w = fam.call(f, inp, "nis")
            outs[table] = dict(raw=raw_records(f)[0], applied=f.applied(), nis=nis_w, dof=dof_w)
    healthy = kinds == X.CLEAN
    assert np.array_equal(outs["wrong entries"]["applied"].astype(bool), healthy), what          # nothing is rejected by the gate
    assert np.array_equal(case.free[1].astype(bool), healthy)
    assert same_rows(outs["none"], outs["wrong entries"]), what
    assert same_rows({"nis": nis, "dof": dof}, {k: outs["none"][k] for k in ("nis", "dof")}), what          # the gate changes no output


@pytest.mark.parametrize("dtype,n", [(d, n) for d in (32, 64) for n in (18, 15)])
def test_depth_through_every_exit(dtype, n):
    """Measured on an MI355X (columns: nis rel err | applied lanes: literal, sigma-aware, plain per-block, cov, cov block-wise | ll abs err):
      f32 N=18  8.9e-08 | 5.4e-08 7.3e-08 1.0e-07 3.6e-08 8.5e-08 | 5.9e-08        f32 N=15  8.0e-08 | 7.7e-09 7.5e-08 9.5e-08 5.1e-08 9.5e-08 | 4.4e-08
      f64 N=18  4.6e-13 | 2.0e-15 4.6e-15 7.3e-14 2.2e-16 3.2e-15 | 8.9e-16        f64 N=15  4.6e-13 | 2.8e-16 7.9e-15 1.5e-14 2.5e-16 4.2e-15 | 8.9e-16
    82 lanes applied, 91 rejected at the gate.  With the condition of the first version (nis > thr[1] alone) the NaN-record and the
    negated-covariance lanes are applied and all four cases fail at the partition."""
    run_case("depth", dtype, n, 1)


@pytest.mark.parametrize("dtype,n", [(d, n) for d in (32, 64) for n in (18, 15)])
def test_velocity_through_every_exit(dtype, n):
    """Measured on an MI355X (columns: nis rel err | applied lanes: literal, sigma-aware, plain per-block, cov, cov block-wise | ll abs err):
      f32 N=18  1.0e-07 | 5.3e-08 8.8e-08 1.6e-07 5.0e-08 1.5e-07 | 9.0e-08        f32 N=15  1.3e-07 | 7.2e-09 7.0e-08 7.0e-08 5.7e-08 1.8e-07 | 6.5e-08
      f64 N=18  8.0e-15 | 1.9e-16 3.4e-16 1.8e-15 2.0e-15 2.7e-13 | 1.3e-15        f64 N=15  3.1e-15 | 1.1e-17 3.2e-16 3.9e-16 1.6e-14 8.5e-13 | 1.3e-15
    78 / 79 lanes applied, 95 / 94 rejected at the gate.  The fp32 objects of the first version reported nis = NaN on the negated-covariance
    lanes (the root of a negative pivot) and failed at the nis of the usable lanes; the fp64 objects passed."""
    run_case("velocity", dtype, n, 3)


@pytest.mark.parametrize("dtype,n,m", [(d, n, m) for d in (32, 64) for n in (18, 15) for m in (1, 2, 3)])
def test_rows_through_every_exit(dtype, n, m):
    """Measured on an MI355X (columns: nis rel err | applied lanes: literal, sigma-aware, plain per-block, cov, cov block-wise | ll abs err):
      f32 N=18 m=1  5.6e-08 | 5.2e-08 9.6e-08 9.6e-08 3.8e-08 5.7e-08 | 2.3e-08    f32 N=15 m=1  5.9e-08 | 8.3e-09 8.1e-08 1.1e-07 5.9e-08 5.9e-08 | 5.9e-08
      f32 N=18 m=2  5.3e-08 | 8.8e-08 8.8e-08 1.9e-07 4.4e-08 5.8e-08 | 1.1e-07    f32 N=15 m=2  5.2e-08 | 7.2e-09 1.1e-07 1.8e-07 4.3e-08 5.8e-08 | 8.9e-08
      f32 N=18 m=3  5.4e-08 | 3.4e-07 1.1e-07 3.4e-07 4.6e-08 5.9e-08 | 1.2e-07    f32 N=15 m=3  5.5e-08 | 8.9e-09 1.6e-07 2.8e-07 4.5e-08 5.7e-08 | 1.1e-07
      f64 N=18 m=1  5.9e-16 | 2.7e-16 2.8e-16 7.0e-16 2.9e-16 6.5e-16 | 4.4e-16    f64 N=15 m=1  3.7e-16 | 2.3e-17 3.3e-16 9.7e-16 3.6e-16 8.3e-16 | 4.4e-16
      f64 N=18 m=2  8.3e-16 | 9.4e-16 4.9e-16 2.1e-15 4.1e-16 8.5e-16 | 8.9e-16    f64 N=15 m=2  7.5e-16 | 2.3e-17 3.8e-16 1.4e-15 4.6e-16 1.1e-15 | 8.9e-16
      f64 N=18 m=3  6.5e-16 | 4.2e-15 7.7e-16 4.2e-15 5.4e-16 8.6e-16 | 1.8e-15    f64 N=15 m=3  5.9e-16 | 2.3e-17 7.0e-16 2.5e-15 1.1e-15 3.6e-15 | 1.8e-15
    73 .. 82 lanes applied, 91 .. 100 rejected at the gate.  The six fp32 objects of the first version failed as the velocity update's did."""
    run_case("rows", dtype, n, m)
