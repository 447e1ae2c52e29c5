"""GPU suite: IMM mixing of hypothesis groups (fbus_ekf_group_mix, include/fbus_ekf.h).  The mixed records are held to the fp64
restatement of tests/group_mix_ref.py under the single-step gates of tests/util.py; the identity matrix, the untouched targets, the
carried rotation, placement in the batch, the repeat and the graph replay bit for bit.  Inputs and shapes are those of
tests/test_group_gpu.py, restated: 192 filters (three tiles) and 96 (a partial last tile); G = 3 leaves a lane of every wave idle and
lets a wave's filters straddle two tiles, G = 64 is one group per wave, G = 2 / 8 / 32 divide the wave."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import group_mix_ref
import group_ref
from fbus_ekf import BatchedFilter, capi, noise, synth
from support import frozen, r32, same_state
from util import (COV_BLOCK_TOL, COV_BLOCK_TOL_F64, COV_TOL, F64_TOL, STATE_TOL, cov_rel_err, cov_rel_err_blockwise, state_rel_err,
                  state_rel_err_literal)

pytestmark = pytest.mark.gpu

SHAPES = [(192, 2, 18), (192, 3, 18), (192, 8, 18), (192, 64, 18), (96, 3, 18), (96, 32, 18), (192, 3, 15), (192, 64, 15)]
DTYPES = [32, 64]
# one sigma of each error-state block p v theta ba bg g (a converged filter: sigma_theta = 1e-3 rad)
SIGMA = np.repeat([1e-2, 2e-2, 1e-3, 5e-3, 1e-3, 5e-2], 3)
STAY = 0.9


def _inputs(B, G, N, seed=0):
    """tests/test_group_gpu.py::_inputs, restated: per group one base state; every member offset by about one sigma per block (the
    rotation through the quaternion), with its own random SPD covariance; logw spread over a few units, in some groups one entry -inf
    and one NaN.  fp32-representable."""
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


def _mixed(B, G, N, dtype, trans, seed=0, logw=None, rows=None):
    """one handle in the state of _inputs (its first `rows` filters): (before, after, applied before / after, weight, logc, logw)"""
    prm, nom, rot, P, prev, lw = _inputs(B, G, N, seed)
    lw = lw if logw is None else logw
    n = B if rows is None else rows
    with _flt(n, prm, dtype, N, (nom[:n], rot[:n], P[:n], prev[:n])) as f:
        before, app0 = f.get_state(), f.applied()
        weight, logc = _np(f.group_mix(G, trans, lw[:n]))
        after, app1 = f.get_state(), f.applied()
    return before, after, (app0, app1), weight, logc, lw[:n]


@functools.lru_cache(maxsize=None)
def _ref(B, G, N, seed=0):
    """the restatement on the inputs themselves (fp32-representable: both record types hold exactly these values), once per shape"""
    _, nom, rot, P, prev, logw = _inputs(B, G, N, seed)
    return frozen(group_mix_ref.mix((nom, rot, P, prev), logw, noise.imm_transition(G, STAY), G))


@functools.lru_cache(maxsize=None)
def _case(B, G, N, dtype):
    return frozen(_mixed(B, G, N, dtype, noise.imm_transition(G, STAY)))


def _gates(dtype):
    return (F64_TOL, F64_TOL, COV_BLOCK_TOL_F64) if dtype == 64 else (STATE_TOL, COV_TOL, COV_BLOCK_TOL)


def _hold(got_nom, got_P, ref_nom, ref_P, dtype, what):
    """the single-step gates of tests/util.py on a mixed state and covariance, every figure printed before it is held"""
    st, cv, cb = _gates(dtype)
    lit = state_rel_err_literal(got_nom, ref_nom)
    sig, blk = state_rel_err(got_nom, ref_nom, ref_P)
    ce, cbe = cov_rel_err(got_P, ref_P), cov_rel_err_blockwise(got_P, ref_P)
    print(f"[group_mix] {what}: literal {lit:.2e}  sigma-aware {sig:.2e} ({blk})  cov {ce:.2e}  cov block-wise {cbe:.2e}")
    assert lit <= min(st, STATE_TOL), f"{what}: literal state rel err {lit:.3g}"
    assert sig <= st, f"{what}: state rel err {sig:.3g} in block {blk}"
    assert ce <= cv, f"{what}: covariance rel err {ce:.3g}"
    assert cbe <= cb, f"{what}: block-wise covariance rel err {cbe:.3g}"


def _outputs_match(weight, logc, w_ref, lc_ref):
    assert weight.dtype == np.float64 and logc.dtype == np.float64
    assert np.abs(weight - w_ref).max() <= 1e-12 and np.array_equal(weight == 0, w_ref == 0)
    fin = np.isfinite(lc_ref)
    assert np.array_equal(np.isfinite(logc), fin) and (logc[~fin] == -np.inf).all()
    assert np.abs(logc[fin] - lc_ref[fin]).max() <= 1e-12


def _rewritten(logw, trans, G):
    """(which filters the definition rewrites, the batch index of each filter's chart member): c_j > 0 and W_jj != 1"""
    _, logc, W = noise.group_mix_weights(logw, trans, G)
    _, best = noise.group_weights(logw, G)
    jj = np.arange(G)
    chart = np.repeat(np.arange(len(best)) * G + np.maximum(best, 0), G)
    return np.isfinite(logc) & (W[:, jj, jj].ravel() != 1.0), chart


# ---- 1. parity with the fp64 restatement ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,G,N", SHAPES)
def test_mix_matches_the_reference(B, G, N, dtype):
    before, after, app, weight, logc, logw = _case(B, G, N, dtype)
    w_ref, lc_ref, nom_ref, rot_ref, P_ref = _ref(B, G, N)
    _, nom, rot, P, prev, _ = _inputs(B, G, N)
    assert same_state(before, (nom, rot, P, prev))                  # (the restatement ran on exactly the state the handle held)
    _outputs_match(weight, logc, w_ref, lc_ref)
    hit, chart = _rewritten(logw, noise.imm_transition(G, STAY), G)
    assert hit.sum() > B // 2 and (w_ref == 0).any()
    _hold(after[0], after[2], nom_ref, P_ref, dtype, f"mix B={B} G={G} N={N} fp{dtype}")
    # the carried rotation is the chart member's, bit for bit; a target that is not rewritten keeps every byte
    assert np.array_equal(after[1][hit], before[1][chart][hit]) and np.array_equal(after[1], rot_ref)
    assert same_state(after, before, rows=np.flatnonzero(~hit))
    assert not np.array_equal(after[0][hit], before[0][hit])
    assert np.array_equal(after[3], before[3]) and np.array_equal(app[0], app[1])
    assert np.array_equal(after[2], np.swapaxes(after[2], 1, 2))   # exactly symmetric


# ---- 2. the identity changes nothing -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,G,N", SHAPES)
def test_the_identity_matrix_leaves_every_record_bit_equal(B, G, N, dtype):
    before, after, app, weight, logc, logw = _mixed(B, G, N, dtype, np.eye(G))
    assert not np.isfinite(logw).all()                              # (the -inf / NaN entries of _inputs are present)
    assert same_state(after, before) and np.array_equal(app[0], app[1])
    w_ref, lc_ref, _ = noise.group_mix_weights(logw, np.eye(G), G)
    _outputs_match(weight, logc, w_ref, lc_ref)


# ---- 3. the rank-one matrix is group_fuse -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,G,N", SHAPES)
def test_equal_rows_give_every_member_the_fused_estimate(B, G, N, dtype):
    """Every member is a target here (c_j = pi_j > 0).  One kind of target is not rewritten: the only usable member of its group has
    W_jj = mu_j = 1 and keeps its bytes (step 6 of the definition), where fuse returns that same member with its quaternion
    normalised -- the inputs are rounded to fp32, so in an fp64 record |q| is 1 to 3e-8 only (2.6e-9 of the 19-vector, above the fp64
    gate of 1e-9).  Such a member is held to its own bytes, and to fuse's estimate after the normalisation fuse applies."""
    prm, nom, rot, P, prev, logw = _inputs(B, G, N)
    pi = np.random.default_rng(G).uniform(0.2, 1.0, G)
    pi /= pi.sum()
    trans = np.tile(pi, (G, 1))
    with _flt(B, prm, dtype, N, (nom, rot, P, prev)) as f:
        before = f.get_state()
        _, best, f_nom, f_P, _ = _np(f.group_fuse(G, logw))
        weight, logc = _np(f.group_mix(G, trans, logw))
        after = f.get_state()
    assert (best >= 0).all()                                        # every group of _inputs has a usable member: every c_j > 0
    assert np.abs(logc - np.tile(np.log(pi), B // G)).max() <= 1e-12
    grp = np.arange(B) // G
    hit, _ = _rewritten(logw, trans, G)
    kept = np.flatnonzero(~hit)
    assert same_state(after, before, rows=kept) and (weight[kept] == 1.0).all() and len(kept) < B // 2
    want = after[0].astype(np.float64)
    want[kept, 6:10] /= np.linalg.norm(want[kept, 6:10], axis=1, keepdims=True)
    _hold(want, after[2], f_nom.astype(np.float64)[grp], f_P.astype(np.float64)[grp], dtype, f"rank-one B={B} G={G} N={N} fp{dtype}")
    assert np.array_equal(after[1], rot[grp * G + best[grp]])


# ---- 4. a NaN member is re-seeded from the others -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,G,N", [(192, 8, 18), (96, 3, 18), (192, 64, 15)])
def test_a_nan_member_with_nan_logw_is_reseeded(B, G, N, dtype):
    prm, nom, rot, P, prev, logw = _inputs(B, G, N, seed=3)
    logw = np.where(np.isfinite(logw), logw, -252.0)
    bad = np.arange(B // G) * G + (np.arange(B // G) * 5 + 1) % G       # one member of every group
    nom_p, rot_p, P_p, logw_p = nom.copy(), rot.copy(), P.copy(), logw.copy()
    nom_p[bad], rot_p[bad], P_p[bad], logw_p[bad] = np.nan, np.nan, np.nan, np.nan
    trans = noise.imm_transition(G, STAY)                               # strictly positive: every target is reachable
    with _flt(B, prm, dtype, N, (nom_p, rot_p, P_p, prev)) as f:
        assert np.isnan(f.get_state()[0][bad]).all()
        weight, logc = _np(f.group_mix(G, trans, logw_p))
        after = f.get_state()
    for a in (weight, logc) + tuple(after[:3]):
        assert np.isfinite(a).all()
    # the restatement never reads a source of weight 0: run on the records the NaNs replaced, that source is simply left out
    w_ref, lc_ref, nom_ref, rot_ref, P_ref = group_mix_ref.mix((nom, rot, P, prev), logw_p, trans, G)
    assert (weight[bad] == 0).all()
    _outputs_match(weight, logc, w_ref, lc_ref)
    _hold(after[0][bad], after[2][bad], nom_ref[bad], P_ref[bad], dtype, f"re-seeded B={B} G={G} N={N} fp{dtype}")
    _hold(after[0], after[2], nom_ref, P_ref, dtype, f"re-seeding group B={B} G={G} N={N} fp{dtype}")
    assert np.array_equal(after[1], rot_ref) and np.array_equal(after[3], prev)


# ---- 5. a group without a usable member, a target nothing leads to -------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,G,N", [(192, 3, 18), (192, 64, 15), (96, 32, 18)])
def test_a_dead_group_and_an_unreachable_target_keep_their_bytes(B, G, N, dtype):
    _, _, _, _, _, logw = _inputs(B, G, N, seed=5)
    NG = B // G
    dead = np.arange(0, NG, 2)
    for j in dead:
        logw[j * G:(j + 1) * G] = np.resize([np.nan, np.inf, -np.inf], G)
    j0 = G - 2                                                      # nothing leads to model j0: its column is zero
    trans = noise.imm_transition(G, STAY)
    trans[:, j0] = 0.0
    trans /= trans.sum(axis=1, keepdims=True)
    before, after, app, weight, logc, _ = _mixed(B, G, N, dtype, trans, seed=5, logw=logw)
    members = np.arange(B).reshape(NG, G)
    assert same_state(after, before, rows=members[dead].ravel())
    assert (weight[members[dead]] == 0).all() and (logc[members[dead]] == -np.inf).all()
    assert same_state(after, before, rows=members[:, j0]) and (logc[members[:, j0]] == -np.inf).all()
    w_ref, lc_ref, nom_ref, rot_ref, P_ref = group_mix_ref.mix(before, logw, trans, G)
    _outputs_match(weight, logc, w_ref, lc_ref)
    live = np.setdiff1d(np.arange(B), np.concatenate([members[dead].ravel(), members[:, j0]]))
    assert np.isfinite(logc[live]).all() and not np.array_equal(after[0][live], before[0][live])
    _hold(after[0], after[2], nom_ref, P_ref, dtype, f"zero column B={B} G={G} N={N} fp{dtype}")
    assert np.array_equal(after[1], rot_ref) and np.array_equal(app[0], app[1])


# ---- 6. placement in the batch, and the repeat ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G,N", [(3, 18), (32, 18)])
def test_the_bits_depend_neither_on_the_batch_nor_on_the_run(G, N, dtype):
    whole = _case(192, G, N, dtype)
    again = _mixed(192, G, N, dtype, noise.imm_transition(G, STAY))
    alone = _mixed(192, G, N, dtype, noise.imm_transition(G, STAY), rows=96)
    assert same_state(again[1], whole[1]) and np.array_equal(again[3], whole[3]) and np.array_equal(again[4], whole[4])
    for k in (0, 1):                                            # the same groups before, and the same bits after
        assert same_state(alone[k], tuple(x[:96] for x in whole[k]))
    assert np.array_equal(alone[3], whole[3][:96]) and np.array_equal(alone[4], whole[4][:96])


# ---- 7. the handle's own sums, a captured graph, refusals ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_mix_reads_the_likelihood_sums_of_the_handle(dtype):
    B, G, M = 128, 4, 4
    prm = capi.default_params(capi.DIALECT_MATLAB)
    nom, rot, P, prev = synth.initial_state(0, B // G, list(prm.p0_diag), 18, mixed_cov=True)
    nom, rot, P, prev = (np.repeat(x, G, axis=0) for x in (r32(nom), r32(rot), r32(P), prev))    # a bank: G hypotheses on each filter
    ids, pos, quat = synth.marker_frame(0, B, 0, M, nom, prm)
    pos, quat = r32(pos), r32(quat)
    table, _, rows = noise.grid(prm, B, r_pos=[0.5, 2.0], q_v=[0.3, 3.0])
    assert len(rows) == G
    trans = noise.imm_transition(G, STAY)
    got = {}
    for how in ("sums", "explicit"):
        with _flt(B, prm, dtype, 18, (nom, rot, P, prev)) as f:
            if how == "sums":
                before = f.get_state()
                with pytest.raises(capi.FbusError) as e:
                    f.group_mix(G, trans)
                assert e.value.code == 1 and "loglik_enable" in str(e.value) and same_state(f.get_state(), before)
            f.set_noise(table)
            f.loglik_enable()
            for _ in range(3):
                f.correct(ids, pos, quat, capi.MODE_STACKED)
            ll = f.loglik()[0]
            assert np.isfinite(ll).all() and np.ptp(ll.reshape(-1, G), axis=1).min() > 0
            before = f.get_state()
            out = _np(f.group_mix(G, trans) if how == "sums" else f.group_mix(G, trans, ll))
            got[how] = (out, f.get_state(), ll)
            assert np.array_equal(f.loglik()[0], ll)                # the sums are read, not consumed
            assert not np.array_equal(got[how][1][0], before[0])
    assert np.array_equal(got["sums"][2], got["explicit"][2])
    assert same_state(got["sums"][1], got["explicit"][1])
    for x, y in zip(got["sums"][0], got["explicit"][0]):
        assert np.array_equal(x, y)
    w_np, lc_np, _ = noise.group_mix_weights(got["sums"][2], trans, G)
    _outputs_match(*got["sums"][0], w_np, lc_np)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,G,N", [(192, 3, 18), (192, 64, 15)])
def test_fuse_then_mix_replays_from_a_graph(B, G, N, dtype):
    prm, nom, rot, P, prev, logw = _inputs(B, G, N, seed=8)
    NG = B // G
    logw[0:G] = np.nan                                          # group 0 has no usable member: the mix leaves it alone
    tt = torch.float32 if dtype == 32 else torch.float64

    def outputs():
        return (torch.zeros(B, dtype=torch.float64, device="cuda"), torch.zeros(NG, dtype=torch.int32, device="cuda"),
                torch.zeros((NG, 19), dtype=tt, device="cuda"), torch.zeros((NG, N, N), dtype=tt, device="cuda"),
                torch.zeros((NG, N), dtype=tt, device="cuda"), torch.zeros(B, dtype=torch.float64, device="cuda"),
                torch.zeros(B, dtype=torch.float64, device="cuda"))

    d_logw = torch.from_numpy(logw).cuda()
    d_trans = torch.from_numpy(noise.imm_transition(G, STAY)).cuda()
    got = {}
    for how in ("direct", "graph"):
        out = outputs()
        torch.cuda.synchronize()                                # (the raw calls below do not order against torch's stream)
        with _flt(B, prm, dtype, N, (nom, rot, P, prev)) as f:
            def run():
                f._check(f._lib.fbus_ekf_group_fuse_dev(f._h, G, f._p(d_logw), *(f._p(o) for o in out[:5])), "group_fuse_dev")
                f._check(f._lib.fbus_ekf_group_mix_dev(f._h, G, f._p(d_logw), f._p(d_trans), f._p(out[5]), f._p(out[6])), "group_mix_dev")
            before = f.get_state()
            if how == "graph":
                gid = f.graph_capture(run)
                f.sync()
                assert same_state(f.get_state(), before) and not out[0].any() and not out[6].any()   # capture records, it does not execute
                f.graph_launch(gid)
            else:
                run()
            f.sync()
            got[how] = (_np(out), f.get_state())
    for x, y in zip(got["direct"][0], got["graph"][0]):
        assert np.array_equal(x, y)
    assert same_state(got["direct"][1], got["graph"][1])
    out, after = got["graph"]
    assert out[1][0] == -1 and (out[1][1:] >= 0).all() and (out[6][:G] == -np.inf).all() and np.isfinite(out[6][G:]).all()
    assert same_state(after, before, rows=slice(0, G)) and not np.array_equal(after[0][G:], before[0][G:])
    assert np.array_equal(out[0], out[5])                       # fuse's weight is mix's


@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_arguments_are_refused_and_change_nothing(dtype):
    B, N, G = 192, 18, 3
    prm, nom, rot, P, prev, logw = _inputs(B, G, N, seed=9)
    trans = noise.imm_transition(G, STAY)
    with _flt(B, prm, dtype, N, (nom, rot, P, prev)) as f:
        before = f.get_state()
        lib, h = f._lib, f._h
        d_logw, d_trans = torch.from_numpy(logw).cuda(), torch.from_numpy(trans).cuda()
        d_w = torch.zeros(B, dtype=torch.float64, device="cuda")
        d_c = torch.zeros(B, dtype=torch.float64, device="cuda")
        h_w, h_c = np.zeros(B), np.zeros(B)
        big = np.ascontiguousarray(noise.imm_transition(64, STAY))
        torch.cuda.synchronize()
        for bad in (1, 65, 0, -3, 5, 7, 128):                   # out of range, or not a divisor of 192
            assert lib.fbus_ekf_group_mix_dev(h, bad, f._p(d_logw), f._p(d_trans), f._p(d_w), f._p(d_c)) == 1, bad
            assert lib.fbus_ekf_last_error(h).decode()
            assert lib.fbus_ekf_group_mix(h, bad, f._p(logw), f._p(big), f._p(h_w), f._p(h_c)) == 1, bad
            with pytest.raises(capi.FbusError) as e:
                f.group_mix(bad, big[:max(bad, 1), :max(bad, 1)], logw)
            assert e.value.code == 1
        # trans = NULL
        assert lib.fbus_ekf_group_mix_dev(h, G, f._p(d_logw), None, f._p(d_w), f._p(d_c)) == 1
        assert "trans" in lib.fbus_ekf_last_error(h).decode()
        assert lib.fbus_ekf_group_mix(h, G, f._p(logw), None, f._p(h_w), f._p(h_c)) == 1
        with pytest.raises(capi.FbusError) as e:
            f.group_mix(G, None, logw)
        assert e.value.code == 1 and "trans" in str(e.value)
        # an output inside the records (the rule of fbus_ekf_snapshot_dev)
        ptr, _, total = f.records()
        for k in range(2):
            for where in (ptr + 64, ptr + total - 8):
                args = [f._p(d_w), f._p(d_c)]
                args[k] = C.c_void_p(where)
                assert lib.fbus_ekf_group_mix_dev(h, G, f._p(d_logw), f._p(d_trans), *args) == 1, k
                assert "overlaps the records" in lib.fbus_ekf_last_error(h).decode()
        # the host form inspects trans: a row that does not sum to 1, a negative entry, a NaN -- the text names the row
        for val in (0.5, -0.05, np.nan):
            t = trans.copy()
            t[1, 2] = val
            assert lib.fbus_ekf_group_mix(h, G, f._p(logw), f._p(t), f._p(h_w), f._p(h_c)) == 1, val
            assert "row 1" in lib.fbus_ekf_last_error(h).decode()
            with pytest.raises(ValueError) as e:                # host arrays are held to the same rule by the Python layer
                f.group_mix(G, t, logw)
            assert "row 1" in str(e.value)
        f.sync()
        assert same_state(f.get_state(), before) and not d_w.any() and not d_c.any() and not h_w.any() and not h_c.any()
        # and the host form itself, on good arguments, is the device form
        assert lib.fbus_ekf_group_mix(h, G, f._p(logw), f._p(trans), f._p(h_w), f._p(h_c)) == 0
        host_after = f.get_state()
    dev = _mixed(B, G, N, dtype, trans, seed=9)
    assert same_state(host_after, dev[1]) and np.array_equal(h_w, dev[3]) and np.array_equal(h_c, dev[4])
