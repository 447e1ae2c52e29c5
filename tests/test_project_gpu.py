"""GPU suite of the predicted corner pixels (include/fbus_ekf.h, fbus_ekf_project_markers*) against tests/project_ref.py, the fp64 numpy
restatement of the header's definition: parity of the image points, the per-corner visibility and the innovation covariance; partly
visible and hidden markers; slots and filters that produce nothing; read-only; the round trip through correct_pixels; independence of
place and batch; the noise table; forms and refusals.

B = 130: two full tiles and a tail of two lanes.  The scene is support.perturbed_setup(130, dtype, nstate, 0, "stereo", M=4, seed=3,
n=64): every listed corner is in view of both cameras with |lat|^2 / (klim z_w^2) <= 0.68 and max |uv| = 2.35 (tests/test_project_cpu.py
asserts the flags against the oracle); the rim cases are markers the frame does NOT list, chosen by the reference with a 5 mm margin.

Tolerances.  view: exact.  uv, fp64 records: util.F64_TOL.  uv, fp32 records: 2^-22 = twice the half-ulp of a value below 4 -- the
reference gets the same fp32-rounded record, so one output rounding separates the two (|uv| < 4 is asserted on the reference).
Covariance: max |dS_ij| / sqrt(S_ii S_jj) <= util.COV_BLOCK_TOL for both record types (S is formed in double from the same record;
the reference's H is a central difference at 1e-6).  The measured values are printed."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_capi as oc
import project_ref
from fbus_ekf import capi
from support import make_filter, permutation, perturbed_setup, rows_of, same_rows, to_device, update_call, vp_tilted
from util import COV_BLOCK_TOL, F64_TOL

pytestmark = pytest.mark.gpu

B = 130
NAMES = ("left", "right", "view", "cov_left", "cov_right")
_CACHE = {}


def scene(dtype, nstate, tilted=False):
    """(prm, state, ids, reference outputs of the stereo call on project_ref.subset(B)), cached and read-only"""
    key = (dtype, nstate, tilted)
    if key not in _CACHE:
        prm, nom, rot, P, prev, ids, _, _ = perturbed_setup(B, dtype, nstate, 0, "stereo", M=4, seed=3, n=64, tilted=tilted)
        vp = vp_tilted() if tilted else oc.vision_params()
        sub = project_ref.subset(B)
        ref = dict(zip(("left", "right", "cov_left", "cov_right", "view"), project_ref.project((nom, rot, P), ids, prm, 2, sub, vp=vp)))
        for a in (nom, rot, P, prev, ids, *ref.values()):
            a.setflags(write=False)
        _CACHE[key] = (prm, (nom, rot, P, prev), ids, ref)
    return _CACHE[key]


def run(f, ids, cameras=2, skip=None, cov=True, host=False):
    """one call -> the outputs that exist, as numpy arrays by name"""
    if host:
        out = f.project_markers(np.ascontiguousarray(ids, np.int32), cameras, skip, cov)
    else:
        out = f.project_markers(to_device(np.array(ids), np.int32), cameras, to_device(skip, np.uint8), cov)
        f.sync()
    left, right, view, cl, cr = out
    named = {"left": left, "right": right, "view": view, "cov_left": cl, "cov_right": cr}
    return {k: (v if host else v.cpu().numpy()) for k, v in named.items() if v is not None}


def left_only(ref):
    return {"left": ref["left"], "cov_left": ref["cov_left"], "view": ref["view"] & np.uint8(0x0F)}


def assert_parity(got, ref, rows, dtype, what):
    tol = F64_TOL if dtype == 64 else 2.0 ** -22
    assert np.array_equal(got["view"][rows], ref["view"][rows]), what
    for name in ("left", "right"):
        if name in got:
            assert np.abs(ref[name][rows]).max() < 4.0
            err = np.abs(got[name][rows].astype(np.float64) - ref[name][rows]).max()
            print(f"{what} {name}: max |d uv| {err:.3e} (tol {tol:.3e})")
            assert err <= tol, (what, name, err)
    for name in ("cov_left", "cov_right"):
        if name in got:
            err = project_ref.cov_error(got[name][rows], ref[name][rows])
            print(f"{what} {name}: max |dS_ij| / sqrt(S_ii S_jj) {err:.3e} (tol {COV_BLOCK_TOL:.1e})")
            assert err <= COV_BLOCK_TOL, (what, name, err)
            assert np.array_equal(got[name][rows][..., 0] == 0.0, ref[name][rows][..., 0] == 0.0)


# ---- 1. parity --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cameras", [1, 2])
@pytest.mark.parametrize("dtype,nstate,tilted", [(32, 18, False), (32, 15, False), (64, 18, False), (64, 15, False), (32, 18, True),
                                                 (64, 18, True)])
def test_points_view_and_covariance_equal_the_reference(dtype, nstate, tilted, cameras):
    prm, st, ids, ref = scene(dtype, nstate, tilted)
    rows = project_ref.subset(B)
    with make_filter(B, prm, dtype, nstate, st) as f:
        got = run(f, ids, cameras)
    want = ref if cameras == 2 else left_only(ref)
    assert set(got) == set(want)
    assert_parity(got, want, rows, dtype, f"fp{dtype} N{nstate} cam{cameras}{' tilted' if tilted else ''}")
    assert (want["view"][rows] != 0).sum() >= 20                          # the scene lists markers on the subset


# ---- 2. partly visible and hidden markers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tilted", [(32, False), (64, False), (32, True)])
def test_partly_visible_and_hidden_markers_bit_by_bit(dtype, tilted):
    nstate = 18
    prm, st, ids, _ = scene(dtype, nstate, tilted)
    nom, rot, P, prev = st
    pick, partly, n_unlisted, n_unstable = project_ref.rim_scene(nom, rot, ids, prm)
    print(f"unlisted pairs {n_unlisted}, unstable under +-5 mm {n_unstable}, stable partly visible used {int(partly.sum())}")
    assert n_unstable <= 0.05 * n_unlisted                                # at most 5 % are left out as unstable
    assert partly.sum() >= 40 and (pick >= 0).all()
    ids2 = np.array(ids)
    ids2[:, 3] = pick
    view = project_ref.view_bits(nom, rot, ids2, prm, 2)
    assert ((view[partly, 3] != 0) & (view[partly, 3] != 0xFF)).all() and (view[~partly, 3] == 0).all()
    with make_filter(B, prm, dtype, nstate, st) as f:
        got = run(f, ids2, 2)
        got1 = run(f, ids2, 1)
    assert np.array_equal(got["view"], view)
    assert np.array_equal(got1["view"], view & np.uint8(0x0F))
    for c, (pts, cv) in enumerate((("left", "cov_left"), ("right", "cov_right"))):
        for q in range(4):
            off = (view >> (4 * c + q) & 1) == 0
            assert (got[pts][off][:, 2 * q:2 * q + 2] == 0).all() and (got[cv][off][:, q] == 0).all()
            on = ~off
            assert (got[cv][on][:, q, 0] > 0).all() and (got[cv][on][:, q, 2] > 0).all()
    # the partly visible markers against the full reference, on the filters of the subset that hold one
    rows = [b for b in project_ref.subset(B) if partly[b]]
    assert len(rows) >= 5
    vp = vp_tilted() if tilted else oc.vision_params()
    ref = dict(zip(("left", "right", "cov_left", "cov_right", "view"), project_ref.project((nom, rot, P), ids2, prm, 2, rows, vp=vp)))
    assert_parity(got, ref, rows, dtype, f"rim fp{dtype}{' tilted' if tilted else ''}")


# ---- 3. slots and filters that produce nothing --------------------------------------------------------------------------------------------
def _guarded(shape, dt):
    n = int(np.prod(shape))
    big = torch.full((n + 64,), 77, dtype=dt, device="cuda")
    return big, big[:n].view(shape)


@pytest.mark.parametrize("dtype", [32, 64])
def test_padding_unknown_ids_skip_null_outputs_and_guard_words(dtype):
    nstate, M = 18, 16
    prm, st, ids, _ = scene(dtype, nstate)
    ids16 = np.full((B, M), -1, np.int32)
    ids16[:, :4] = ids
    ids16[::2, 4] = ids[::2, 0]                                           # a slot that is padding for some lanes of a wave only
    ids16[:, 5], ids16[:, 6], ids16[:, 7] = 9, -5, 2000                   # not in the map; out of range (slots 8..15: padding for all)
    assert project_ref.slot_of(prm, 9) < 0
    skip = (np.arange(B) % 5 == 2).astype(np.uint8)
    tt = torch.float32 if dtype == 32 else torch.float64
    with make_filter(B, prm, dtype, nstate, st) as f:
        base = run(f, ids, 2)
        got = run(f, ids16, 2)
        sk = run(f, ids16, 2, skip)
        assert same_rows(got, run(f, ids16, 2, host=True))                # the host form equals _dev bit for bit
        one = run(f, ids16, 1, cov=False)
        assert set(one) == {"left", "view"} and same_rows(one, {"left": got["left"], "view": got["view"] & np.uint8(0x0F)})
        for name in NAMES:
            assert same_rows({name: got[name][:, :4]}, {name: base[name]}), name
            assert same_rows({name: got[name][::2, 4]}, {name: base[name][::2, 0]}), name
            assert (got[name][1::2, 4] == 0).all() and (got[name][:, 5:] == 0).all(), name
            assert (sk[name][skip != 0] == 0).all() and same_rows({name: sk[name]}, {name: got[name]}, np.nonzero(skip == 0)[0],
                                                                    np.nonzero(skip == 0)[0]), name
        # each output NULL in turn (and none), into guarded buffers: the tail behind every output survives the ragged last tile
        lib, h, p = f._lib, f._h, f._p
        d_ids = to_device(ids16, np.int32)
        shapes = (((B, M, 8), tt), ((B, M, 8), tt), ((B, M, 4, 3), torch.float64), ((B, M, 4, 3), torch.float64), ((B, M), torch.uint8))
        order = ("left", "right", "cov_left", "cov_right", "view")
        for drop in (None,) + order:
            bufs = [_guarded(s, t) for s, t in shapes]
            torch.cuda.synchronize()
            args = [None if name == drop else p(v) for name, (_, v) in zip(order, bufs)]
            assert lib.fbus_ekf_project_markers_dev(h, M, p(d_ids), 2, None, *args) == 0, drop
            f.sync()
            for name, (big, v) in zip(order, bufs):
                assert (big[v.numel():] == 77).all(), (drop, name)
                if name == drop:
                    assert (big == 77).all(), name
                else:
                    assert same_rows({name: v.cpu().numpy()}, {name: got[name]}), (drop, name)
        # cameras = 1: right and cov_right are not written and may be anything
        bufs = [_guarded(s, t) for s, t in shapes]
        torch.cuda.synchronize()
        bogus = C.c_void_p(12345)
        assert lib.fbus_ekf_project_markers_dev(h, M, p(d_ids), 1, None, p(bufs[0][1]), bogus, p(bufs[2][1]), bogus, p(bufs[4][1])) == 0
        f.sync()
        assert same_rows({"left": bufs[0][1].cpu().numpy(), "cov_left": bufs[2][1].cpu().numpy(), "view": bufs[4][1].cpu().numpy()},
                         {"left": got["left"], "cov_left": got["cov_left"], "view": got["view"] & np.uint8(0x0F)})


# ---- 4. read-only -------------------------------------------------------------------------------------------------------------------------
def test_the_call_writes_nothing_but_its_outputs():
    dtype, nstate = 32, 18
    prm, nom, rot, P, prev, ids, left, right = perturbed_setup(B, dtype, nstate, 0, "stereo", M=4, seed=3, n=64)
    with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as f:
        f.loglik_enable(True)
        update_call(f, "stereo", ids, left, right, nis=True)               # applied flags and likelihood sums that are not all zero
        _, _, total = f.records()

        def snap():
            buf = torch.empty(total, dtype=torch.uint8, device="cuda")
            f.copy_records(buf)
            f.sync()
            return buf.cpu().numpy()
        rec0, app0, lik0 = snap(), f.applied(), f.loglik()
        d = run(f, ids, 2)
        hst = run(f, ids, 2, host=True)
        run(f, ids, 1)
        rec1, app1, lik1 = snap(), f.applied(), f.loglik()
    assert (d["view"][ids >= 0] == 0xFF).all() and same_rows(d, hst)
    assert np.array_equal(rec0, rec1) and np.array_equal(app0, app1) and app0.any()
    assert all(np.array_equal(x, y) for x, y in zip(lik0, lik1)) and lik0[1].any()


# ---- 5. round trip: the output is a ready measurement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cameras", [1, 2])
@pytest.mark.parametrize("dtype,tilted", [(32, False), (64, False), (32, True)])
def test_the_projection_fed_back_to_the_update_has_no_innovation(dtype, tilted, cameras):
    """nis <= sum res^2 / r_pix (S >= r_pix I), and each residual is at most the output rounding of a value below 4, 2^-23, with a
    factor 2 in hand: dof 2^-44 / r_pix for fp32 records; 1e-12 per residual for fp64"""
    nstate = 18
    prm, st, ids, _ = scene(dtype, nstate, tilted)
    nom, rot, _, _ = st
    pick = project_ref.rim_scene(nom, rot, ids, prm)[0]
    ids2 = np.array(ids)
    ids2[:, 3] = pick                                                     # partly visible and hidden markers among them
    with make_filter(B, prm, dtype, nstate, st) as f:
        d_ids = to_device(ids2, np.int32)
        left, right, view, _, _ = f.project_markers(d_ids, cameras, cov=False)
        nis, dof = update_call(f, "stereo" if cameras == 2 else "left", d_ids, left, right, nis=True)
        view = view.cpu().numpy()
    want = 2 * np.array([[bin(int(v)).count("1") for v in row] for row in view]).sum(axis=1)
    assert np.array_equal(dof, want) and (want >= 8).all()
    bound = want * (2.0 ** -44 if dtype == 32 else 1e-24) / prm.r_pix
    print(f"fp{dtype} cam{cameras}{' tilted' if tilted else ''}: max nis / bound {np.max(nis / bound):.3e}, min nis {nis.min():.3e}")
    assert (nis <= bound).all()
    if dtype == 32:
        assert (nis >= 0).all()


# ---- 6. independence ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,nstate", [(32, 18), (64, 15)])
def test_a_filter_projects_the_same_whatever_its_place_or_batch(dtype, nstate):
    prm, st, ids, _ = scene(dtype, nstate)
    sub = lambda rows: tuple(np.ascontiguousarray(x[rows]) for x in st)
    with make_filter(B, prm, dtype, nstate, st) as f:
        full = run(f, ids, 2)
        assert same_rows(full, run(f, ids, 2))                            # twice the same
    n = 127                                                               # prime: support.permutation is a bijection
    pi = permutation(n)
    assert sorted(pi) == list(range(n))
    with make_filter(n, prm, dtype, nstate, sub(pi)) as f:
        assert same_rows(run(f, ids[pi], 2), full, None, pi)
    with make_filter(64, prm, dtype, nstate, sub(np.arange(64))) as f:
        assert same_rows(run(f, ids[:64], 2), full, None, np.arange(64))
    with make_filter(1, prm, dtype, nstate, sub(np.array([129]))) as f:
        assert same_rows(run(f, ids[[129]], 2), full, None, np.array([129]))


# ---- 7. noise table -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [32, 64])
def test_a_noise_table_moves_the_diagonal_of_S_by_its_r_pix_and_nothing_else(dtype):
    nstate = 18
    prm, st, ids, _ = scene(dtype, nstate)
    rows5 = rows_of(prm)
    table = np.ascontiguousarray(rows5[np.arange(B) % len(rows5)])
    with make_filter(B, prm, dtype, nstate, st) as f:
        plain = run(f, ids, 2)
        f.set_noise(table)
        tabled = run(f, ids, 2)
    for name in ("left", "right", "view"):
        assert same_rows({name: tabled[name]}, {name: plain[name]}), name
    shift = (table[:, 6] - prm.r_pix)[:, None, None]
    assert np.unique(table[:, 6]).size > 1
    for c, name in enumerate(("cov_left", "cov_right")):
        on = (plain["view"][..., None] >> (4 * c + np.arange(4)) & 1) != 0              # (B, M, 4)
        d = tabled[name] - plain[name]
        scale = 1e-12 * np.maximum(np.abs(tabled[name]), np.abs(plain[name]))            # relative to the entries themselves
        for j in (0, 2):
            assert (np.abs(d[..., j] - shift * on) <= scale[..., j]).all(), (name, j)
        assert (d[..., 1] == 0).all(), name
        assert on.any() and (tabled[name][~on] == 0).all()


# ---- 8. forms and refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_in_the_headers_order_graph_replay_and_all_null():
    dtype, nstate, M = 32, 18, 4
    prm, st, ids, _ = scene(dtype, nstate)
    ids = np.ascontiguousarray(ids, np.int32)
    with make_filter(B, prm, dtype, nstate, st) as f:
        lib, h, p = f._lib, f._h, f._p
        want = run(f, ids, 2)
        d_ids = to_device(ids, np.int32)
        mk = lambda shape, t: torch.full(shape, 77, dtype=t, device="cuda")
        o = [mk((B, M, 8), torch.float32), mk((B, M, 8), torch.float32), mk((B, M, 4, 3), torch.float64), mk((B, M, 4, 3), torch.float64),
             mk((B, M), torch.uint8)]
        ho = [np.full((B, M, 8), 77, np.float32), np.full((B, M, 8), 77, np.float32), np.full((B, M, 4, 3), 77.0), np.full((B, M, 4, 3), 77.0),
              np.full((B, M), 77, np.uint8)]
        torch.cuda.synchronize()
        recs, _, total = f.records()
        err = lambda: lib.fbus_ekf_last_error(h)
        off4 = lambda t: C.c_void_p(t.data_ptr() + 4)
        inside = C.c_void_p(recs + 1024)
        for fn, name, io, ii in ((lib.fbus_ekf_project_markers_dev, b"fbus_ekf_project_markers_dev", [p(x) for x in o], p(d_ids)),
                                 (lib.fbus_ekf_project_markers, b"fbus_ekf_project_markers", [p(x) for x in ho], p(ids))):
            assert fn(None, M, ii, 2, None, *io) == 1
            for bad in (0, -1, 17):                                       # FBUS_MAX_VISIBLE = 16
                assert fn(h, bad, None, 3, None, *io) == 1 and name + b":" in err() and b"M = " in err(), bad
            assert fn(h, M, None, 3, None, *io) == 1 and name + b":" in err() and b"ids is NULL" in err()
            for cam in (0, 3):
                assert fn(h, M, ii, cam, None, off4(o[0]), *io[1:]) == 1 and name + b":" in err() and b"cameras = " in err(), cam
            assert fn(h, M, ii, 2, None, None, None, None, None, None) == 0                  # all outputs NULL: legal, launches nothing
        dev = lib.fbus_ekf_project_markers_dev
        for k in range(4):                                                # each of left / right / cov_left / cov_right misaligned
            args = [p(x) for x in o]
            args[k] = off4(o[k]) if k != 3 else C.c_void_p(recs + 4)      # (and inside the records: the alignment is tested first)
            assert dev(h, M, p(d_ids), 2, None, *args) == 1 and b"fbus_ekf_project_markers_dev:" in err() and b"16-byte aligned" in err(), k
        for k, bytes_ in enumerate((B * M * 8 * 4, B * M * 8 * 4, B * M * 96, B * M * 96, B * M)):
            for ptr in (recs, recs + total - 16, recs - bytes_ + 16):
                args = [p(x) for x in o]
                args[k] = C.c_void_p(ptr)
                assert dev(h, M, p(d_ids), 2, None, *args) == 1 and b"fbus_ekf_project_markers_dev:" in err() and b"overlaps the records" in err(), k
        with pytest.raises(ValueError):
            f.project_markers(ids, cameras=3)
        f.sync()
        assert all((x == 77).all() for x in o) and all((x == 77).all() for x in ho)          # nothing was launched or copied
        # captured and replayed; the host form cannot be captured
        def cap():
            f._check(dev(h, M, p(d_ids), 2, None, *[p(x) for x in o]), "project_markers_dev")
            assert lib.fbus_ekf_project_markers(h, M, p(ids), 2, None, *[p(x) for x in ho]) == 1
            assert b"fbus_ekf_project_markers:" in err() and b"graph_begin" in err()
        gid = f.graph_capture(cap)
        f.graph_launch(gid)
        f.sync()
        assert all((x == 77).all() for x in ho)
        assert same_rows({n: x.cpu().numpy() for n, x in zip(("left", "right", "cov_left", "cov_right", "view"), o)}, want)
    # r_pix <= 0 is refused behind the alignment and in front of the overlap
    bad = capi.FbusParams.from_buffer_copy(prm)
    bad.r_pix = 0.0
    with make_filter(B, bad, dtype, nstate, st) as f:
        lib, h, p = f._lib, f._h, f._p
        recs, _, _ = f.records()
        d_ids = to_device(ids, np.int32)
        torch.cuda.synchronize()
        err = lambda: lib.fbus_ekf_last_error(h)
        assert lib.fbus_ekf_project_markers_dev(h, M, p(d_ids), 2, None, C.c_void_p(recs + 4), None, None, None, None) == 1
        assert b"16-byte aligned" in err()
        assert lib.fbus_ekf_project_markers_dev(h, M, p(d_ids), 2, None, C.c_void_p(recs), None, None, None, None) == 1
        assert b"fbus_ekf_project_markers_dev:" in err() and b"r_pix must be positive" in err()
        assert lib.fbus_ekf_project_markers(h, M, p(ids), 2, None, None, None, None, None, None) == 1
        assert b"fbus_ekf_project_markers:" in err() and b"r_pix must be positive" in err()
