"""GPU suite: hypothesis groups (fbus_ekf_group_fuse / fbus_ekf_group_collapse, include/fbus_ekf.h).  fuse is held to the fp64
restatement of tests/group_ref.py under the single-step gates of tests/util.py; collapse, the untouched records, the repeat and the
graph replay bit for bit.  Shapes: 192 filters (three tiles) and 96 (a partial last tile); G = 3 leaves a lane of every wave idle
and lets a wave's filters straddle two tiles, G = 64 is one group per wave, G = 2 / 8 / 32 divide the wave."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import group_ref
from fbus_ekf import BatchedFilter, capi, noise, synth
from support import r32, same_state
from util import (COV_BLOCK_TOL, COV_BLOCK_TOL_F64, COV_TOL, F64_TOL, STATE_TOL, cov_rel_err, cov_rel_err_blockwise, state_rel_err,
                  state_rel_err_literal)

pytestmark = pytest.mark.gpu

SHAPES = [(192, 2, 18), (192, 3, 18), (192, 8, 18), (192, 64, 18), (96, 3, 18), (96, 32, 18), (192, 3, 15), (192, 64, 15)]
# one sigma of each error-state block p v theta ba bg g (a converged filter: sigma_theta = 1e-3 rad)
SIGMA = np.repeat([1e-2, 2e-2, 1e-3, 5e-3, 1e-3, 5e-2], 3)


def _inputs(B, G, N, seed=0):
    """per group one base state; every member offset by about one sigma per block (the rotation through the quaternion), with its own
    random SPD covariance; logw spread over a few units, in some groups one entry -inf and one NaN.  fp32-representable."""
    rng = np.random.default_rng(1000 * G + B + N + seed)
    NG = B // G
    prm = capi.default_params(capi.DIALECT_MATLAB)
    base, _, _, _ = synth.initial_state(0, NG, list(prm.p0_diag), N, mixed_cov=True)
    nom = np.repeat(base, G, axis=0)
    off = rng.normal(0, 1.0, (B, 18)) * SIGMA
    nom[:, 0:3] += off[:, 0:3]
    nom[:, 3:6] += off[:, 3:6]
    nom[:, 10:13] += off[:, 9:12]
    nom[:, 13:16] += off[:, 12:15]
    if N == 18:
        nom[:, 16:19] += off[:, 15:18]
    for b in range(B):
        q = group_ref.qmul(nom[b, 6:10], group_ref.dq(off[b, 6:9]))
        nom[b, 6:10] = q / np.linalg.norm(q)
    A = rng.normal(0, 1.0, (B, N, N))
    P = (A @ np.swapaxes(A, 1, 2) / N + np.eye(N)) * (SIGMA[:N, None] * SIGMA[None, :N])
    P = 0.5 * (P + np.swapaxes(P, 1, 2))
    prev = (np.arange(B) * 7 % 5).astype(np.int32)
    logw = rng.uniform(-4.0, 0.0, B) - 250.0
    for j in range(0, NG, 3):                   # every third group: one member excluded by -inf ...
        logw[j * G + int(rng.integers(G))] = -np.inf
    for j in range(1, NG, 3):                   # ... the next one by NaN, and where there is room both
        k = int(rng.integers(G))
        logw[j * G + k] = np.nan
        if G > 2:
            logw[j * G + (k + 1) % G] = -np.inf
    nom = r32(nom)
    return prm, nom, r32(synth.q2R(nom[:, 6:10]).reshape(B, 9)), r32(P), prev, logw


def _flt(B, prm, dtype, N, state):
    f = BatchedFilter(B, prm, device=0, dtype=dtype, nstate=N)
    f.set_state(*state)
    return f


def _np(out):
    return tuple(None if o is None else o.cpu().numpy() for o in out)


@functools.lru_cache(maxsize=None)
def _case(B, G, N, dtype):
    """one handle per shape: the state before, two fuse calls, the pdiag-only call, the state after, and the reference -- computed once"""
    prm, nom, rot, P, prev, logw = _inputs(B, G, N)
    with _flt(B, prm, dtype, N, (nom, rot, P, prev)) as f:
        before, app0 = f.get_state(), f.applied()
        one = f.group_fuse(G, logw)
        two = f.group_fuse(G, torch.from_numpy(logw).cuda())
        diag = f.group_fuse(G, logw, full_cov=False)
        f.sync()
        one, two, diag = _np(one), _np(two), _np(diag)
        after, app1 = f.get_state(), f.applied()
    ref = group_ref.fuse(before[0], before[2], logw, G)
    return {"logw": logw, "before": before, "after": after, "app": (app0, app1), "one": one, "two": two, "diag": diag, "ref": ref}


def _gates(dtype):
    return (F64_TOL, F64_TOL, COV_BLOCK_TOL_F64) if dtype == 64 else (STATE_TOL, COV_TOL, COV_BLOCK_TOL)


def _hold(got_nom, got_P, ref_nom, ref_P, dtype, what):
    """the single-step gates of tests/util.py on a fused state and covariance, every figure printed before it is held"""
    st, cv, cb = _gates(dtype)
    lit = state_rel_err_literal(got_nom, ref_nom)
    sig, blk = state_rel_err(got_nom, ref_nom, ref_P)
    ce, cbe = cov_rel_err(got_P, ref_P), cov_rel_err_blockwise(got_P, ref_P)
    print(f"[group] {what}: literal {lit:.2e}  sigma-aware {sig:.2e} ({blk})  cov {ce:.2e}  cov block-wise {cbe:.2e}")
    assert lit <= min(st, STATE_TOL), f"{what}: literal state rel err {lit:.3g}"
    assert sig <= st, f"{what}: state rel err {sig:.3g} in block {blk}"
    assert ce <= cv, f"{what}: covariance rel err {ce:.3g}"
    assert cbe <= cb, f"{what}: block-wise covariance rel err {cbe:.3g}"


# ---- 1. parity with the fp64 restatement ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("B,G,N", SHAPES)
def test_fuse_matches_the_reference(B, G, N, dtype):
    c = _case(B, G, N, dtype)
    weight, best, nom, P, pdiag = c["one"]
    w_ref, b_ref, nom_ref, P_ref = c["ref"]
    assert weight.dtype == np.float64 and best.dtype == np.int32 and nom.shape == (B // G, 19) and P.shape == (B // G, N, N)
    assert np.array_equal(best, b_ref)
    assert (b_ref >= 0).all() and (w_ref == 0).any()                    # (every group has a usable member, some members are excluded)
    assert np.abs(weight - w_ref).max() <= 1e-12
    assert np.array_equal(weight == 0, w_ref == 0)
    _hold(nom, P, nom_ref, P_ref, dtype, f"fuse B={B} G={G} N={N} fp{dtype}")
    assert np.array_equal(pdiag, np.einsum("bii->bi", P))               # bit for bit
    assert np.array_equal(P, np.swapaxes(P, 1, 2))                      # exactly symmetric
    # the diagonal-only form: the same weights and state, the same diagonal
    assert c["diag"][3] is None
    for i in (0, 1, 2):
        assert np.array_equal(c["diag"][i], c["one"][i])
    st, _, cb = _gates(dtype)
    d_ref = np.einsum("bii->bi", P_ref)
    assert (np.abs(c["diag"][4] - d_ref) / d_ref).max() <= cb


# ---- 2, 3. nothing is touched, and a second call repeats the first --------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("B,G,N", SHAPES)
def test_fuse_leaves_the_records_alone_and_repeats_bit_for_bit(B, G, N, dtype):
    c = _case(B, G, N, dtype)
    for x, y in zip(c["before"], c["after"]):
        assert np.array_equal(x, y)
    assert np.array_equal(c["app"][0], c["app"][1])
    for x, y in zip(c["one"], c["two"]):
        assert np.array_equal(x, y)


# ---- 4. a diverged member does not poison its group ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("B,G,N", [(192, 8, 18), (96, 3, 18), (192, 64, 15)])
def test_a_nan_member_with_nan_logw_is_left_out(B, G, N, dtype):
    prm, nom, rot, P, prev, logw = _inputs(B, G, N, seed=3)
    logw = np.where(np.isfinite(logw), logw, -252.0)
    bad = np.arange(B // G) * G + (np.arange(B // G) * 5 + 1) % G       # one member of every group
    nom_p, rot_p, P_p, logw_p = nom.copy(), rot.copy(), P.copy(), logw.copy()
    nom_p[bad], rot_p[bad], P_p[bad], logw_p[bad] = np.nan, np.nan, np.nan, np.nan
    with _flt(B, prm, dtype, N, (nom_p, rot_p, P_p, prev)) as f:
        assert np.isnan(f.get_state()[0][bad]).all()
        weight, best, fn, fP, fd = _np(f.group_fuse(G, logw_p))
    for a in (weight, fn, fP, fd):
        assert np.isfinite(a).all()
    # the reference with that member removed: groups of G - 1
    keep = np.setdiff1d(np.arange(B), bad)
    with _flt(B, prm, dtype, N, (nom, rot, P, prev)) as f:
        g = f.get_state()
    w_ref, b_ref, nom_ref, P_ref = group_ref.fuse(g[0][keep], g[2][keep], logw[keep], G - 1)
    assert (weight[bad] == 0).all() and np.abs(weight[keep] - w_ref).max() <= 1e-12
    assert np.array_equal(np.arange(B).reshape(-1, G)[np.arange(B // G), best], keep.reshape(-1, G - 1)[np.arange(B // G), b_ref])
    _hold(fn, fP, nom_ref, P_ref, dtype, f"poison B={B} G={G} N={N} fp{dtype}")
    assert np.array_equal(fd, np.einsum("bii->bi", fP))


# ---- 5. a group without a usable member --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("B,G,N", [(192, 3, 18), (192, 64, 15), (96, 32, 18)])
def test_a_group_without_a_usable_member_reports_member_zero(B, G, N, dtype):
    prm, nom, rot, P, prev, logw = _inputs(B, G, N, seed=5)
    NG = B // G
    dead = np.arange(0, NG, 2)
    for j in dead:
        logw[j * G:(j + 1) * G] = np.resize([np.nan, np.inf, -np.inf], G)
    with _flt(B, prm, dtype, N, (nom, rot, P, prev)) as f:
        s_nom, s_pd, _ = _np(f.snapshot())
        g = f.get_state()
        weight, best, fn, fP, fd = _np(f.group_fuse(G, logw))
        _, _, dn, _, dd = _np(f.group_fuse(G, logw, full_cov=False))
    assert (best[dead] == -1).all() and (weight.reshape(NG, G)[dead] == 0).all()
    assert np.array_equal(fn[dead], s_nom[dead * G]) and np.array_equal(fd[dead], s_pd[dead * G])
    assert np.array_equal(dn[dead], s_nom[dead * G]) and np.array_equal(dd[dead], s_pd[dead * G])
    assert np.array_equal(fP[dead], g[2][dead * G])
    live = np.setdiff1d(np.arange(NG), dead)
    w_ref, b_ref, _, _ = group_ref.fuse(g[0], g[2], logw, G)
    assert np.array_equal(best, b_ref) and (best[live] >= 0).all() and np.abs(weight - w_ref).max() <= 1e-12


# ---- 6. collapse ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("B,G,N", [(192, 3, 18), (192, 8, 18), (192, 64, 15), (96, 32, 18), (96, 3, 15)])
def test_collapse_copies_the_source_record_bit_for_bit(B, G, N, dtype):
    prm, nom, rot, P, prev, _ = _inputs(B, G, N, seed=6)
    NG = B // G
    rng = np.random.default_rng(G)
    src = rng.integers(0, G, NG).astype(np.int32)
    src[1::4] = -1                                              # skipped groups
    src_dev = src.copy()
    src_dev[3::8] = G                                           # the device form inspects nothing: outside 0..G-1 = leave the group alone
    src_dev[NG - 1] = 1000 if NG > 7 else G
    members = np.arange(B).reshape(NG, G)
    for form in ("dev", "host"):
        s = src_dev if form == "dev" else src
        hit = np.flatnonzero((s >= 0) & (s < G))
        with _flt(B, prm, dtype, N, (nom, rot, P, prev)) as f:
            before = f.get_state()
            f.group_collapse(G, torch.from_numpy(s).cuda() if form == "dev" else s)
            after = f.get_state()
            want = [x.copy() for x in before]
            for j in hit:
                for x in want:
                    x[members[j]] = x[members[j, s[j]]]
            assert len(hit) and len(hit) < NG
            assert same_state(after, want), f"{form}: collapsed groups / untouched groups"
            assert (after[3][members[hit]] == before[3][members[hit, s[hit]]][:, None]).all()          # prev_id travels with the record
            # one predict with the same IMU sample for every filter: the members of a collapsed group stay bit-equal
            acc = np.tile(np.array([0.1, -0.2, 9.7], f.np_dtype), (1, B, 1))
            gyr = np.tile(np.array([0.01, 0.02, -0.015], f.np_dtype), (1, B, 1))
            f.predict(acc[0], gyr[0], np.array([0.005], f.np_dtype))
            moved = f.get_state()
            assert not np.array_equal(moved[0], after[0])
            for j in hit:
                for x in moved:
                    assert (x[members[j]] == x[members[j, 0]]).all()
    # the host form refuses a member index >= G and changes nothing
    with _flt(B, prm, dtype, N, (nom, rot, P, prev)) as f:
        before = f.get_state()
        with pytest.raises(capi.FbusError) as e:
            f.group_collapse(G, src_dev)
        assert e.value.code == 1 and "src[" in str(e.value)
        assert same_state(f.get_state(), before)


# ---- 7. with the handle's own sums ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [32, 64])
def test_fuse_reads_the_likelihood_sums_of_the_handle(dtype):
    B, G, M = 128, 4, 4
    prm = capi.default_params(capi.DIALECT_MATLAB)
    nom, rot, P, prev = synth.initial_state(0, B // G, list(prm.p0_diag), 18, mixed_cov=True)
    nom, rot, P, prev = (np.repeat(x, G, axis=0) for x in (r32(nom), r32(rot), r32(P), prev))    # a bank: G hypotheses on each filter
    ids, pos, quat = synth.marker_frame(0, B, 0, M, nom, prm)
    pos, quat = r32(pos), r32(quat)
    table, hyp, rows = noise.grid(prm, B, r_pos=[0.5, 2.0], q_v=[0.3, 3.0])
    assert len(rows) == G
    with _flt(B, prm, dtype, 18, (nom, rot, P, prev)) as f:
        with pytest.raises(capi.FbusError) as e:
            f.group_fuse(G)
        assert e.value.code == 1 and "loglik_enable" in str(e.value)
        f.set_noise(table)
        f.loglik_enable()
        for _ in range(3):
            f.correct(ids, pos, quat, capi.MODE_STACKED)
        ll = f.loglik()[0]
        assert np.isfinite(ll).all() and np.ptp(ll.reshape(-1, G), axis=1).min() > 0
        weight, best, fn, fP, fd = _np(f.group_fuse(G))
        w_np, b_np = noise.group_weights(ll, G)
        assert np.abs(weight - w_np).max() <= 1e-12 and np.array_equal(best, b_np)
        g = f.get_state()
        _, _, nom_ref, P_ref = group_ref.fuse(g[0], g[2], ll, G)
        _hold(fn, fP, nom_ref, P_ref, dtype, f"fuse from the sums fp{dtype}")
        # the sums are read, not consumed
        assert np.array_equal(f.loglik()[0], ll)


# ---- 8. captured in a graph --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("B,G,N", [(192, 3, 18), (192, 64, 15)])
def test_fuse_then_collapse_replays_from_a_graph(B, G, N, dtype):
    prm, nom, rot, P, prev, logw = _inputs(B, G, N, seed=8)
    NG = B // G
    logw[0:G] = np.nan                                          # group 0 has no usable member: best = -1, collapse skips it
    tt = torch.float32 if dtype == 32 else torch.float64

    def outputs():
        return (torch.zeros(B, dtype=torch.float64, device="cuda"), torch.zeros(NG, dtype=torch.int32, device="cuda"),
                torch.zeros((NG, 19), dtype=tt, device="cuda"), torch.zeros((NG, N, N), dtype=tt, device="cuda"),
                torch.zeros((NG, N), dtype=tt, device="cuda"))

    d_logw = torch.from_numpy(logw).cuda()
    got = {}
    for how in ("direct", "graph"):
        out = outputs()
        torch.cuda.synchronize()                                # (the raw calls below do not order against torch's stream)
        with _flt(B, prm, dtype, N, (nom, rot, P, prev)) as f:
            def run():
                f._check(f._lib.fbus_ekf_group_fuse_dev(f._h, G, f._p(d_logw), *(f._p(o) for o in out)), "group_fuse_dev")
                f._check(f._lib.fbus_ekf_group_collapse_dev(f._h, G, f._p(out[1])), "group_collapse_dev")
            if how == "graph":
                before = f.get_state()
                gid = f.graph_capture(run)
                f.sync()
                assert same_state(f.get_state(), before) and not out[0].any()             # capture records, it does not execute
                f.graph_launch(gid)
            else:
                run()
            f.sync()
            got[how] = (_np(out), f.get_state())
    for x, y in zip(got["direct"][0], got["graph"][0]):
        assert np.array_equal(x, y)
    assert same_state(got["direct"][1], got["graph"][1])
    best, after = got["graph"][0][1], got["graph"][1]
    assert best[0] == -1 and (best[1:] >= 0).all()
    members = np.arange(B).reshape(NG, G)
    for x in after:                                             # every group but the first sits on its winner
        assert (x[members[1:]] == x[members[np.arange(1, NG), best[1:]]][:, None]).all()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [32, 64])
def test_bad_group_sizes_and_aliased_outputs_are_refused(dtype):
    B, N = 192, 18
    prm, nom, rot, P, prev, logw = _inputs(B, 3, N, seed=9)
    with _flt(B, prm, dtype, N, (nom, rot, P, prev)) as f:
        before = f.get_state()
        lib, h = f._lib, f._h
        d_logw = torch.from_numpy(logw).cuda()
        d_w = torch.zeros(B, dtype=torch.float64, device="cuda")
        d_src = torch.zeros(B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for G in (1, 65, 0, -3, 5, 7, 128):                     # out of range, or not a divisor of 192
            assert lib.fbus_ekf_group_fuse_dev(h, G, f._p(d_logw), f._p(d_w), None, None, None, None) == 1, G
            assert lib.fbus_ekf_last_error(h).decode()
            assert lib.fbus_ekf_group_fuse(h, G, f._p(logw), None, None, None, None, None) == 1, G
            assert lib.fbus_ekf_group_collapse_dev(h, G, f._p(d_src)) == 1, G
            assert lib.fbus_ekf_group_collapse(h, G, f._p(np.zeros(B, np.int32))) == 1, G
            for call in (lambda: f.group_fuse(G, logw), lambda: f.group_collapse(G, np.zeros(max(B // max(G, 1), 1), np.int32))):
                with pytest.raises(capi.FbusError) as e:
                    call()
                assert e.value.code == 1
        assert lib.fbus_ekf_group_collapse_dev(h, 3, None) == 1 and lib.fbus_ekf_group_collapse(h, 3, None) == 1
        # an output inside the records (the rule of fbus_ekf_snapshot_dev)
        ptr, _, total = f.records()
        for k in range(5):
            args = [None] * 5
            args[k] = C.c_void_p(ptr + 64)
            assert lib.fbus_ekf_group_fuse_dev(h, 3, f._p(d_logw), *args) == 1, k
            assert "overlaps the records" in lib.fbus_ekf_last_error(h).decode()
            args[k] = C.c_void_p(ptr + total - 8)
            assert lib.fbus_ekf_group_fuse_dev(h, 3, f._p(d_logw), *args) == 1, k
        f.sync()
        assert same_state(f.get_state(), before) and not d_w.any()
