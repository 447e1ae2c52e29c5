"""GPU suite of the per-marker screen (include/fbus_ekf.h, fbus_ekf_screen_markers*; csrc/ekf_screen.hpp) against tests/screen_ref.py, the
fp64 restatement from the header: the statistic of every slot against the reference and against the _nis entry points on a frame that
holds the slot alone, the decision, its statistics on a scene with planted outliers, the screen in front of the gated update, that it
writes nothing but its outputs, the edges, independence of the neighbours, the noise table, the refusals and a captured graph.
B = 200 (three full tiles and 8 lanes) unless stated.  The pixel scenes of support.perturbed_setup hold ONE to FOUR markers per filter
in view (1.27 on average), padded with -1: most of a frame's slots are padding."""
import math

import numpy as np
import pytest
import torch

import screen_ref
from fbus_ekf import capi, gating
from support import (B_IND, G, J, make_filter, permutation, perturbed_setup, pose_setup, rows_of, to_device, update_call, vp_tilted,
                     with_row)

pytestmark = pytest.mark.gpu

B = 200
KIND = {"pose": capi.SCREEN_POSE, "left": capi.SCREEN_PIXELS, "stereo": capi.SCREEN_PIXELS, "corners": capi.SCREEN_CORNERS}
VARIANTS = [("pose", 0), ("pose", 1), ("left", 0), ("stereo", 1), ("corners", 0)]          # (kind, dialect)
_SCENES = {}


def scene(kind, Bn, dtype, nstate, dialect=0, M=4, tilted=False):
    """(prm, state, ids, a, b): pose rows of support.pose_setup, or the first M slots of support.perturbed_setup's frame (corners:
    a = the 12 coordinates of VIS_CORNERS3D, b = None; tilted: the port normal support.TILT).  Cached; the arrays are not written by any
    test (copies are)"""
    key = (kind, Bn, dtype, nstate, dialect, M, tilted)
    if key not in _SCENES:
        if kind == "pose":
            prm, nom, rot, P, prev, ids, a, b = pose_setup(Bn, dtype, nstate, dialect, False, M)
        else:
            # (at least the 256 filters of the underlying scene: the corner rows are built for all of them)
            prm, nom, rot, P, prev, ids, a, b = (x[:Bn] if isinstance(x, np.ndarray) else x
                                                 for x in perturbed_setup(max(Bn, 256), dtype, nstate, dialect, kind, tilted=tilted))
            nom, rot, P, prev = (np.ascontiguousarray(x) for x in (nom, rot, P, prev))
            ids, a, b = (np.ascontiguousarray(x[:, :M]) for x in (ids, a, b))
            b = b if kind == "stereo" else None
        _SCENES[key] = (prm, (nom, rot, P, prev), ids, a, b)
    return _SCENES[key]


def screen_call(f, kind, ids, a, b, skip=None, host=False, inplace=False):
    """one screen through BatchedFilter.screen_markers (device arrays; host=True: numpy in and out) -> numpy (ids_out, nis as float64,
    dof, kept)"""
    conv = (lambda x, dt=None: None if x is None else np.ascontiguousarray(x, dt)) if host else to_device
    geometry = capi.VIS_CORNERS3D if kind == "corners" else capi.VIS_REFRACTIVE
    out = f.screen_markers(KIND[kind], conv(ids, np.int32), conv(a, f.np_dtype), conv(b, f.np_dtype), geometry=geometry,
                           skip=None if skip is None else conv(skip, np.uint8), inplace=inplace)
    f.sync()
    io, nis, dof, kept = (x if host else x.cpu().numpy() for x in out)
    return io, nis.astype(np.float64), dof, kept


def plant(kind, prm, a, bad, slot=0):
    """a copy of `a` with one corner (pose: the position) of `slot` of the filters `bad` moved 30 sigma in every coordinate"""
    a = a.copy()
    if kind in ("left", "stereo"):
        a[bad, slot, 0:2] += 30 * math.sqrt(prm.r_pix)
    else:
        a[bad, slot, 0:3] += 30 * math.sqrt(prm.r_pos)
    return a


def nis_tol(kind, dtype, ref, rr):
    if kind == "pose":
        return (1e-3 * max(ref, 1.0) + 1e-6 * rr) if dtype == 32 else (1e-8 * max(ref, 1.0) + 1e-12 * rr)
    return (1e-3 if dtype == 32 else 1e-6) * max(ref, 1.0)


def check_statistic(kind, dialect, dtype, nstate, prm, st, ids, a, b, slots, filters, vp=None):
    M = ids.shape[1]
    with make_filter(B, prm, dtype, nstate, st) as f, make_filter(B, prm, dtype, nstate, st) as t:
        st0 = f.get_state()
        ids_out, nis, dof, kept = screen_call(f, kind, ids, a, b)
        twin = {}
        for m in slots:                                     # the parent's kernels on a frame that holds slot m alone
            t.set_state(*st)
            one = np.full_like(ids, -1)
            one[:, m] = ids[:, m]
            twin[m] = update_call(t, kind, one, np.nan_to_num(a), None if b is None else np.nan_to_num(b), nis=True)
    assert np.array_equal(ids_out, ids)                     # no table: nothing finite is dropped
    rn, rd, rj, rr = screen_ref.screen(st0, ids, a, b, prm, kind, filters, dialect, nstate, vp=vp)
    worst, worst_twin, n = 0.0, 0.0, 0
    for k in filters:
        for m in range(M):
            assert dof[k, m] == rd[k, m], (k, m, dof[k, m], rd[k, m])
            if not rj[k, m]:
                assert nis[k, m] == 0.0
                continue
            assert abs(nis[k, m] - rn[k, m]) <= nis_tol(kind, dtype, rn[k, m], rr[k, m]), (k, m, nis[k, m], rn[k, m], rr[k, m])
            worst = max(worst, abs(nis[k, m] - rn[k, m]) / max(rn[k, m], 1.0))
            n += 1
    assert n >= 20
    for m in slots:
        assert np.array_equal(twin[m][1], dof[:, m]), m     # the _nis call's dof, exactly
        worst_twin = max(worst_twin, float(np.max(np.abs(twin[m][0] - nis[:, m]) / np.maximum(nis[:, m], 1.0))))
    assert np.array_equal(kept, screen_ref.in_map(ids, prm).sum(axis=1))
    print(f"{kind} dialect {dialect} fp{dtype} N {nstate} M {M}: {n} slots, worst |nis - ref| / max(ref, 1) = {worst:.2e}; "
          f"against correct_*_nis on the slot alone {worst_twin:.2e}")


# ---- 1. the statistic -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,nstate,M", [(32, 18, 4), (64, 15, 3), (32, 15, 1), (64, 18, 4)])
@pytest.mark.parametrize("kind,dialect", VARIANTS)
def test_statistic_against_the_reference_and_the_nis_entry_points(kind, dialect, dtype, nstate, M):
    prm, st, ids, a, b = scene(kind, B, dtype, nstate, dialect, M)
    check_statistic(kind, dialect, dtype, nstate, prm, st, ids, a, b, range(M), range(0, B, 3 if kind == "pose" else 2))


@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("kind", ["left", "stereo"])
def test_statistic_on_a_tilted_port(kind, dtype):
    """the general-normal instantiations (NZ = false; the left camera then folds in the IMU frame)"""
    prm, st, ids, a, b = scene(kind, B, dtype, 18, 0, 4, tilted=True)
    check_statistic(kind, 0, dtype, 18, prm, st, ids, a, b, range(4), range(0, B, 2), vp=vp_tilted())


def test_statistic_with_16_slots_and_4_in_view():
    """the frame of M = 4 spread over slots 1, 6, 11, 12 of 16; the padding holds id -1 and NaN image points"""
    kind, dtype, nstate = "left", 32, 18
    prm, st, ids4, a4, _ = scene(kind, B, dtype, nstate, 0, 4)
    at = [1, 6, 11, 12]
    ids = np.full((B, 16), -1, np.int32)
    a = np.full((B, 16, 8), np.nan)
    ids[:, at], a[:, at] = ids4, a4
    check_statistic(kind, 0, dtype, nstate, prm, st, ids, a, None, at, range(0, B, 2))


# ---- 2. the decision ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,dialect", VARIANTS)
def test_the_screen_drops_exactly_nis_above_its_threshold(kind, dialect):
    dtype, nstate = 32, 18
    prm, st, ids, a, b = scene(kind, B, dtype, nstate, dialect)
    bad = np.arange(B) % 4 == 1
    a = plant(kind, prm, a, bad)
    thr = gating.chi2_gate(0.999)
    with make_filter(B, prm, dtype, nstate, st) as f:
        f.set_gate(thr)
        ids_out, nis, dof, kept = screen_call(f, kind, ids, a, b)
    judged = dof > 0
    assert np.array_equal(ids_out, np.where(judged & ~(nis <= thr[dof]), -1, ids))
    assert np.array_equal(kept, screen_ref.in_map(ids_out, prm).sum(axis=1))
    assert (ids_out[bad & judged[:, 0], 0] == -1).all() and (bad & judged[:, 0]).sum() >= 40
    assert np.array_equal(judged, screen_ref.in_map(ids, prm))


# ---- 3. its statistics ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["left", "corners"])
def test_planted_outliers_are_dropped_and_clean_slots_are_kept(kind):
    """4096 filters, slot 0 of every eighth with one corner 30 sigma off: every such slot goes, at most 1 % of the clean judged slots
    do.  (tests/screen_ref.py alone on this scene, seed 3: 0 of 4688 clean slots dropped for both kinds -- below half the cap.)"""
    Bn, dtype, nstate = 4096, 32, 18
    prm, st, ids, a, b = scene(kind, Bn, dtype, nstate)
    bad = np.arange(Bn) % 8 == 5
    a = plant(kind, prm, a, bad)
    with make_filter(Bn, prm, dtype, nstate, st) as f:
        f.set_gate(gating.chi2_gate(0.999))
        ids_out, nis, dof, kept = screen_call(f, kind, ids, a, b)
    judged = dof > 0
    assert judged[bad, 0].all()
    assert (ids_out[bad, 0] == -1).all()
    clean = judged.copy()
    clean[bad, 0] = False
    share = float((ids_out[clean] == -1).mean())
    print(f"{kind}: {int(clean.sum())} clean judged slots, {100 * share:.3f} % dropped; {int(bad.sum())} planted, all dropped")
    assert share <= 0.01


# ---- 4. in front of the gated update --------------------------------------------------------------------------------------------------------

def test_the_screened_frame_updates_where_the_whole_frame_gate_cannot():
    """Three handles run correct_pixels_nis with the 0.999 table: (a) the frame as it is, (b) the screen's ids_out, (c) the planted
    slots set to -1 by hand.  A planted filter whose slot 0 was its only marker has no survivor: (b) and (c) leave it alone."""
    Bn, dtype, nstate, kind = 4096, 32, 18, "left"
    prm, st, ids, a, _ = scene(kind, Bn, dtype, nstate)
    bad = np.arange(Bn) % 8 == 5
    a = plant(kind, prm, a, bad)
    thr = gating.chi2_gate(0.999)
    by_hand = ids.copy()
    by_hand[bad, 0] = -1
    with make_filter(Bn, prm, dtype, nstate, st) as fa, make_filter(Bn, prm, dtype, nstate, st) as fb, \
            make_filter(Bn, prm, dtype, nstate, st) as fc:
        for f in (fa, fb, fc):
            f.set_gate(thr)
        prior = fa.get_state()
        nis_a, dof_a = update_call(fa, kind, ids, a, None, nis=True)
        sa, app_a = fa.get_state(), fa.applied()
        ids_out, _, _, kept = screen_call(fb, kind, ids, a, None)
        nis_b, dof_b = update_call(fb, kind, ids_out, a, None, nis=True)
        sb, app_b = fb.get_state(), fb.applied()
        nis_c, dof_c = update_call(fc, kind, by_hand, a, None, nis=True)
        sc, app_c = fc.get_state(), fc.applied()
    # (a) rejected -- the prior's bytes -- or applied with the outlier folded
    rej = bad & (app_a == 0)
    for x, y in zip(sa, prior):
        assert np.array_equal(x[rej], y[rej])
    assert (dof_a[bad & (app_a == 1)] >= 8).all()
    print(f"(a) of {int(bad.sum())} planted filters the whole-frame gate rejects {int(rej.sum())} and applies {int((bad & (app_a == 1)).sum())}")
    # (b) the screen took the planted slot and nothing else of these filters (all but the few the 1 % cap of the clean slots allows)
    same = bad & (ids_out == by_hand).all(axis=1)
    assert same.sum() >= 0.97 * bad.sum()
    for x, y in zip(sb, sc):
        assert np.array_equal(x[same], y[same])             # bit for bit the hand-made frame's update
    assert np.array_equal(app_b[same], app_c[same]) and np.array_equal(dof_b[same], dof_c[same])
    left_over = same & (kept > 0)
    assert left_over.sum() >= 50
    assert app_b[left_over].all()                           # every planted filter with a survivor is applied
    assert (dof_b[left_over] > 0).all() and (dof_b[left_over] < dof_a[left_over]).all()      # the survivors' rows alone
    i = np.arange(nstate)
    pd_b, pd_0 = sb[2][:, i, i][:, J], prior[2][:, i, i][:, J]
    assert (pd_b[left_over] < pd_0[left_over]).all()
    alone = same & (kept == 0)
    assert not app_b[alone].any()
    for x, y in zip(sb, prior):
        assert np.array_equal(x[alone], y[alone])


# ---- 5. read-only ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,dialect", VARIANTS)
def test_the_screen_writes_nothing_but_its_outputs(kind, dialect):
    dtype, nstate = 32, 18
    prm, st, ids, a, b = scene(kind, B, dtype, nstate, dialect)
    a = plant(kind, prm, a, np.arange(B) % 4 == 1)
    with make_filter(B, prm, dtype, nstate, st) as f:
        f.set_gate(gating.chi2_gate(0.999))
        f.loglik_enable(True)
        update_call(f, kind, ids, a, b, nis=True)           # applied flags and likelihood sums that are not all zero
        f.set_state(*st)
        _, _, total = f.records()

        def snap():
            buf = torch.empty(total, dtype=torch.uint8, device="cuda")
            f.copy_records(buf)
            f.sync()
            return buf.cpu().numpy()
        rec0, app0, lik0 = snap(), f.applied(), f.loglik()
        out = screen_call(f, kind, ids, a, b)
        di = to_device(ids.copy(), np.int32)
        inp = screen_call(f, kind, di, a, b, inplace=True)
        assert np.array_equal(di.cpu().numpy(), inp[0])     # written into ids itself
        rec1, app1, lik1 = snap(), f.applied(), f.loglik()
    assert (out[0] == -1).sum() > (ids == -1).sum()
    for x, y in zip(out, inp):
        assert np.array_equal(x, y)
    assert np.array_equal(rec0, rec1) and np.array_equal(app0, app1)
    assert all(np.array_equal(x, y) for x, y in zip(lik0, lik1)) and lik0[1].any()


# ---- 6. edges -------------------------------------------------------------------------------------------------------------------------------

def out_of_view(prm, nom, ids):
    """(filter, id): a marker of the map that filter cannot see"""
    from fbus_ekf import synth
    from support import predicted_rows
    import oracle_capi as oc
    vp = oc.vision_params()
    for k in range(len(nom)):
        for mid in synth.marker_table(prm)[0]:
            if mid not in ids[k] and not predicted_rows(nom[k], np.array([mid]), prm, vp, "left")[1].any():
                return k, int(mid)
    raise AssertionError("every marker of the map is in view of every filter")


@pytest.mark.parametrize("gated", [False, True])
def test_edges(gated):
    kind, dtype, nstate = "left", 32, 18
    prm, st, ids, a, _ = scene(kind, B, dtype, nstate)
    ids, a = ids.copy(), a.copy()
    full = np.nonzero(screen_ref.in_map(ids, prm).sum(axis=1) >= 2)[0]          # filters with two markers in view
    assert len(full) >= 4
    k_skip, k_nan, k_rec = int(full[0]), int(full[1]), int(full[2])
    k_out, id_out = out_of_view(prm, np.asarray(st[0], np.float64), ids)
    assert k_out not in (k_skip, k_nan, k_rec)
    k_unk = next(k for k in range(B) if k not in (k_skip, k_nan, k_rec, k_out) and ids[k, 2] == -1 and ids[k, 3] == -1)
    skip = np.zeros(B, np.uint8)
    skip[k_skip] = 1
    thr = gating.chi2_gate(0.999)
    with make_filter(B, prm, dtype, nstate, st) as f:
        if gated:
            f.set_gate(thr)
        base = screen_call(f, kind, ids, a, None)
        e_ids, e_a = ids.copy(), a.copy()
        free = int(np.nonzero(ids[k_out] == -1)[0][0])
        e_ids[k_out, free], e_a[k_out, free] = id_out, 0.0                      # a marker of the map wholly outside the port's view
        e_ids[k_unk, 3], e_ids[k_unk, 2] = 31, 5000                              # ids outside the map (inside and beyond the id table)
        e_a[k_nan, 0, 3] = np.nan                                                # one coordinate of one slot
        nom, rot, P, prev = (np.array(x) for x in st)
        nom[k_rec, 1] = np.nan                                                   # the record itself
        f.set_state(nom, rot, P, prev)
        edge = screen_call(f, kind, e_ids, e_a, None, skip=skip)
    (b_ids, b_nis, b_dof, b_kept), (o_ids, o_nis, o_dof, o_kept) = base, edge
    inm = screen_ref.in_map(ids, prm)
    # a skipped filter: nothing judged, the ids as they came, kept 0
    assert np.array_equal(o_ids[k_skip], ids[k_skip]) and not o_nis[k_skip].any() and not o_dof[k_skip].any() and o_kept[k_skip] == 0
    # -1 and unknown ids pass through
    pad = e_ids == -1
    assert (o_ids[pad] == -1).all() and not o_nis[pad].any() and not o_dof[pad].any()
    assert not screen_ref.in_map([31, 5000], prm).any()
    for m in (2, 3):
        assert o_ids[k_unk, m] == e_ids[k_unk, m] and o_nis[k_unk, m] == 0 and o_dof[k_unk, m] == 0
    assert o_kept[k_unk] == b_kept[k_unk]
    # out of view: no rows, not judged, kept -- and counted, the update would be handed it
    assert o_ids[k_out, free] == id_out and o_nis[k_out, free] == 0 and o_dof[k_out, free] == 0
    assert o_kept[k_out] == b_kept[k_out] + 1
    # a NaN detection: that slot goes, with and without a table; the filter's other slots are what they were
    assert o_ids[k_nan, 0] == -1 and math.isnan(o_nis[k_nan, 0]) and o_dof[k_nan, 0] == 8
    for x, y in zip(edge[:3], base[:3]):
        assert np.array_equal(x[k_nan, 1:], y[k_nan, 1:])
    assert o_kept[k_nan] == b_kept[k_nan] - 1
    # a NaN record: every slot of the map goes, nothing else of the batch moves
    assert (o_ids[k_rec][inm[k_rec]] == -1).all() and np.isnan(o_nis[k_rec][inm[k_rec]]).all() and o_kept[k_rec] == 0
    assert np.array_equal(o_ids[k_rec][~inm[k_rec]], ids[k_rec][~inm[k_rec]])
    others = np.setdiff1d(np.arange(B), [k_skip, k_nan, k_rec, k_out, k_unk])
    for x, y in zip(edge, base):
        assert np.array_equal(x[others], y[others])


# ---- 7. independence ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,dialect", VARIANTS)
def test_a_filter_is_screened_the_same_whatever_its_place_or_batch(kind, dialect):
    dtype, nstate, Bn = 32, 18, 4096
    prm, st, ids, a, b = scene(kind, Bn, dtype, nstate, dialect)
    a = plant(kind, prm, a, np.arange(Bn) % 4 == 1)
    thr = gating.chi2_gate(0.999)
    take = lambda x, sel: None if x is None else np.ascontiguousarray(x[sel])

    def run(sel):
        with make_filter(len(sel), prm, dtype, nstate, tuple(take(x, sel) for x in st)) as f:
            f.set_gate(thr)
            return screen_call(f, kind, take(ids, sel), take(a, sel), take(b, sel))
    big = run(np.arange(Bn))
    sel = np.arange(1001, 1001 + B)                        # B = 200 filters from the middle of the 4096, starting at lane 41 of a tile
    small = run(sel)
    for x, y in zip(small, big):
        assert np.array_equal(x, y[sel])
    ind = np.arange(B_IND)
    pi = permutation()
    plain, perm = run(ind), run(ind[pi])
    for x, y in zip(perm, plain):
        assert np.array_equal(x, y[pi])
    assert (plain[0] == -1).sum() > (ids[ind] == -1).sum()


# ---- 8. the noise table ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,dialect", VARIANTS)
def test_a_tabled_filter_is_screened_as_its_untabled_twin(kind, dialect):
    dtype, nstate = 32, 18
    prm, st, ids, a, b = scene(kind, B, dtype, nstate, dialect)
    a = plant(kind, prm, a, np.arange(B) % 4 == 1)
    rows, g = rows_of(prm), np.arange(B) % G
    thr = gating.chi2_gate(0.999)
    with make_filter(B, prm, dtype, nstate, st) as f:
        f.set_gate(thr)
        f.set_noise(rows[g])
        got = screen_call(f, kind, ids, a, b)
    differ = 0
    for k in range(G):
        with make_filter(B, with_row(prm, rows[k]), dtype, nstate, st) as t:
            t.set_gate(thr)
            ref = screen_call(t, kind, ids, a, b)
        for x, y in zip(got, ref):
            assert np.array_equal(x[g == k], y[g == k])
            differ += int(not np.array_equal(x[g != k], y[g != k]))
    assert differ > 0                                       # the rows do matter


# ---- 9. refusals, the host form, a captured graph -------------------------------------------------------------------------------------------

def test_validation_host_form_and_graph_replay():
    kind, dtype, nstate, M = "left", 32, 18, 4
    prm, st, ids, a, _ = scene(kind, B, dtype, nstate)
    a = plant(kind, prm, a, np.arange(B) % 4 == 1)
    with make_filter(B, prm, dtype, nstate, st) as f:
        lib, h, p = f._lib, f._h, f._p
        di, da = to_device(ids, np.int32), to_device(a, np.float32)
        o_ids = torch.full((B, M), 77, dtype=torch.int32, device="cuda")
        o_nis = torch.full((B, M), 7.0, dtype=torch.float32, device="cuda")
        o_dof = torch.full((B, M), 77, dtype=torch.int32, device="cuda")
        o_kept = torch.full((B,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                            # (the raw calls below do not order against torch's stream)
        dev = lambda: lib.fbus_ekf_screen_markers_dev(h, capi.SCREEN_PIXELS, M, p(di), p(da), None, 0, None, p(o_ids), p(o_nis), p(o_dof),
                                                      p(o_kept))
        f.set_gate(gating.chi2_gate(0.999, 7))              # the left camera reaches dof 8: one entry short
        assert dev() == 1 and b"fbus_ekf_screen_markers_dev" in lib.fbus_ekf_last_error(h)
        h_ids = np.full((B, M), 77, np.int32)
        assert lib.fbus_ekf_screen_markers(h, capi.SCREEN_PIXELS, M, p(np.ascontiguousarray(ids)), p(np.ascontiguousarray(a, np.float32)), None,
                                           0, None, p(h_ids), None, None, None) == 1
        f.sync()
        assert (h_ids == 77).all() and (o_ids.cpu().numpy() == 77).all() and (o_nis.cpu().numpy() == 7.0).all()
        assert (o_dof.cpu().numpy() == 77).all() and (o_kept.cpu().numpy() == 77).all()        # nothing was launched
        # the other refusals, each with a text that names the entry point
        bad_calls = [(9, M, p(di), p(da)), (capi.SCREEN_PIXELS, 0, p(di), p(da)), (capi.SCREEN_PIXELS, 17, p(di), p(da)),
                     (capi.SCREEN_PIXELS, M, None, p(da)), (capi.SCREEN_PIXELS, M, p(di), None), (capi.SCREEN_POSE, M, p(di), p(da)),
                     (capi.SCREEN_PIXELS, M, p(di), C_off(da, 4))]
        for kd, m, i_, a_ in bad_calls:
            assert lib.fbus_ekf_screen_markers_dev(h, kd, m, i_, a_, None, 0, None, None, None, None, None) == 1, (kd, m)
            assert b"fbus_ekf_screen_markers_dev" in lib.fbus_ekf_last_error(h)
        f.set_gate(gating.chi2_gate(0.999, 8))              # long enough
        assert dev() == 0
        f.sync()
        d_out = (o_ids.cpu().numpy(), o_nis.cpu().numpy().astype(np.float64), o_dof.cpu().numpy(), o_kept.cpu().numpy())
        h_out = screen_call(f, kind, ids, a, None, host=True)
        assert isinstance(h_out[0], np.ndarray) and h_out[2].dtype == np.int32
        for x, y in zip(d_out, h_out):
            assert np.array_equal(x, y)                     # the host form equals the _dev form bit for bit
        assert (d_out[0] == -1).sum() > (ids == -1).sum()
        hi = np.array(ids, np.int32)                        # the host form in place: the screened ids come back into ids itself
        screen_call(f, kind, hi, a, None, host=True, inplace=True)
        assert np.array_equal(hi, d_out[0])
        # a captured _dev call reads the table current at its replay
        f.set_gate(None)
        def cap():
            f._check(dev(), "screen_markers_dev")
            assert lib.fbus_ekf_screen_markers(h, capi.SCREEN_PIXELS, M, p(np.ascontiguousarray(ids)), p(np.ascontiguousarray(a, np.float32)),
                                               None, 0, None, p(h_ids), None, None, None) == 1       # the host form cannot be captured
        gid = f.graph_capture(cap)
        f.graph_launch(gid)
        f.sync()
        assert np.array_equal(o_ids.cpu().numpy(), ids)     # no table: nothing finite is dropped
        tight = np.concatenate([[math.inf], np.full(16, 0.5)])          # far below the clean slots' nis: most of them go
        f.set_gate(tight)
        f.graph_launch(gid)
        f.sync()
        g_ids, g_nis, g_dof = o_ids.cpu().numpy(), o_nis.cpu().numpy().astype(np.float64), o_dof.cpu().numpy()
        assert np.array_equal(g_ids, np.where((g_dof > 0) & ~(g_nis <= tight[g_dof]), -1, ids))
        assert (g_ids == -1).sum() > (d_out[0] == -1).sum()


def C_off(t, nbytes):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + nbytes)
