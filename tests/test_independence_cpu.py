"""CPU suite: the builders of tests/test_independence_gpu.py -- the permutation, the ragged cut, the poison set and its forms, Data.take --
hold the properties that module's variants rest on, and the fp64 C oracle, which runs one filter after the other, gives permuted output
for permuted input bit for bit: the builders move filters, and nothing else."""
import numpy as np
import pytest

from replay_ref import OracleEngine
from route_cells import KC, Data
from support import ALONE, B_IND, POISON_FORMS, SIZE, permutation, poison_set, poisoned_state, ragged_cut, same_rows, with_nan

B = B_IND


@pytest.fixture(scope="module")
def scene():
    return Data(32, 18, 0, B=B, device=False)


def test_the_permutation_moves_every_lane_most_tiles_and_the_tail():
    pi, j = permutation(), np.arange(B)
    assert np.array_equal(np.sort(pi), j)                                  # a bijection
    assert (pi % 64 != j % 64).all()                                       # no filter keeps its lane
    assert (pi // 64 != j // 64).mean() >= 0.5                             # at least half change tile
    assert np.nonzero(pi == B - 1)[0][0] < 192 and pi[B - 1] != B - 1      # the tail tile's filter into a full tile, another in its place
    assert (np.abs(np.diff(pi)) != 1).mean() > 0.9                         # (and neighbours do not travel together)


def test_the_cut_is_ragged():
    lo, hi = ragged_cut()
    assert np.array_equal(np.concatenate([lo, hi]), np.arange(B))
    assert (hi[0] // 64, hi[0] % 64) == (1, 37) and len(hi) % 64 == 28
    assert hi[0] * 3 * 4 == 1212 and 1212 % 16 != 0                         # M = 3: the second shard's ids off the 16-byte boundary


def test_the_poison_set_leaves_a_clean_filter_in_every_tile_and_one_in_a_wave():
    S, form = poison_set()
    clean = np.setdiff1d(np.arange(B), S)
    assert len(S) == 82 == len(set(S)) and 2 * len(S) <= B and len(S) + len(clean) == B
    assert not set(ALONE) & set(S)
    assert all((clean // 64 == t).any() for t in range(4))                 # every tile keeps a clean filter
    assert list(clean[clean // 64 == 1]) == [100]                          # a wave with exactly one clean lane
    assert set(form) == set(range(POISON_FORMS))
    assert all(set(form[S // 64 == t]) == set(range(POISON_FORMS)) for t in range(3))      # every form in every full tile


def test_the_poison_forms_break_what_they_say_and_nothing_else(scene):
    S, form = poison_set()
    clean = np.setdiff1d(np.arange(B), S)
    nom0, rot0, P0, _ = scene.state
    nom, rot, P = poisoned_state(nom0, rot0, P0, S, form)
    assert same_rows({"nominal": nom0, "rot": rot0, "P": P0}, {"nominal": nom, "rot": rot, "P": P}, clean, clean)
    a, b, c, d, e = (S[form == k] for k in range(5))
    assert np.isnan(nom[a]).all() and np.isnan(rot[a]).all() and np.isnan(P[a]).all()
    assert np.isposinf(nom[b, 0:3]).all() and np.isfinite(nom[b, 3:]).all() and (np.diagonal(P[b], axis1=1, axis2=2) == 1e30).all()
    assert np.array_equal(P[c], -P0[c]) and np.array_equal(nom[c], nom0[c])
    assert np.array_equal(nom[d], nom0[d]) and np.array_equal(P[d], P0[d])
    assert (nom[e, 6:10] == 0).all() and (rot[e] == 0).all() and np.array_equal(P[e], P0[e])
    x = with_nan(scene.h["a"], d, 1)
    assert np.isnan(x[:, d]).all() and np.isfinite(np.delete(x, d, axis=1)).all() and np.isfinite(scene.h["a"]).all()
    p = scene.poisoned(S, form)
    assert np.isnan(p.h["dt_b"][:, d]).all() and np.isnan(p.h["rows"]["pose"][1][:, d]).all() and np.isnan(p.h["rows"]["stereo"][2][:, d]).all()
    for k, (ids, _, _) in p.h["rows"].items():                             # ids, skip and the shared period: as they were
        assert np.array_equal(ids, scene.h["rows"][k][0])
    assert np.array_equal(p.h["skip"], scene.h["skip"]) and np.isfinite(p.h["dt"]).all()
    assert np.isfinite(np.delete(p.h["rows"]["corners"][1], S, axis=1)).all() and np.isfinite(np.delete(p.h["dt_b"], S, axis=1)).all()


def test_every_input_differs_from_filter_to_filter(scene):
    h = scene.h
    per_filter = [(h["state"][0], 0), (h["state"][2], 0), (h["meas_state"][0], 0), (h["a"], 1), (h["w"], 1), (h["dt_b"], 1)]
    per_filter += [(x, 1) for v in h["rows"].values() for x in v[1:] if x is not None]
    for x, ax in per_filter:
        flat = np.moveaxis(x, ax, 0).reshape(B, -1)
        assert len(np.unique(flat, axis=0)) == B
    assert (h["dt_b"] >= 0.003).all() and (h["dt_b"] <= 0.007).all() and h["dt_b"].shape == (300, B)
    assert np.array_equal(h["dt_b"], h["dt_b"].astype(np.float32).astype(np.float64))
    assert h["skip"].any() and not h["skip"].all(axis=0).any()


def test_take_returns_the_rows_of_the_whole(scene):
    pi = permutation()
    for ids in (pi, ragged_cut()[1], np.array([100])):
        t, h = scene.take(ids), scene.h
        assert t.B == len(ids) and np.array_equal(t.ids, ids)
        assert same_rows(dict(zip("nrPp", h["state"])), dict(zip("nrPp", t.state)), rows=ids)
        assert same_rows(dict(zip("nrPp", h["meas_state"])), dict(zip("nrPp", t.meas_state)), rows=ids)
        for k in ("a", "w", "dt_b", "skip"):
            assert np.array_equal(h[k][:, ids], t.h[k]), k
        assert np.array_equal(h["dt"], t.h["dt"])
        for k, v in h["rows"].items():
            for x, y in zip(v, t.h["rows"][k]):
                assert (x is None and y is None) or np.array_equal(x[:, ids], y), k
    # skip travels with the filter: the bytes of filter 7 (frame 0) and filter 12 (last frame) are where those filters now stand
    t = scene.take(pi)
    assert t.h["skip"][0, np.nonzero(pi == 7)[0][0]] == 1 and t.h["skip"][len(KC) - 1, np.nonzero(pi == 12)[0][0]] == 1
    # a derivation of a derivation keeps the identities
    assert np.array_equal(scene.take(pi).take(np.argsort(pi)).ids, np.arange(B))
    for how in ("skip", "ids"):
        ab = scene.absent(np.arange(64, 128), how)
        assert ab.h["skip"][:, 64:128].all() if how == "skip" else all((i[:, 64:128] == -1).all() for i, _, _ in ab.h["rows"].values())
        assert np.array_equal(ab.h["skip"][:, :64], h["skip"][:, :64]) and np.array_equal(ab.h["rows"]["pose"][0][:, 128:], h["rows"]["pose"][0][:, 128:])
    out = scene.with_outliers()
    moved = [np.nonzero((out.h["rows"][k][1] != h["rows"][k][1]).reshape(3, B, -1).any(axis=(0, 2)))[0] for k in h["rows"]]
    assert all(np.array_equal(m, np.arange(B)[np.arange(B) % 8 == 5]) for m in moved)


def _oracle(scene, ids):
    """one predict, one pose update and one pixel update of the fp64 oracle on the filters `ids` of the scene, in that order"""
    t = scene.take(ids)
    out = {}
    eng = OracleEngine(t.B, 0, 18)
    eng.set_state(*t.state)
    eng.predict(t.h["a"][0], t.h["w"][0], t.h["dt"][:1])
    out.update(zip(("predict nominal", "predict rot", "predict P", "predict prev"), eng.get_state()))
    i, pos, quat = (x[0] for x in t.h["rows"]["pose"])
    eng.correct(i, pos, quat, 1)
    out.update(zip(("pose nominal", "pose rot", "pose P", "pose prev"), eng.get_state()))
    eng = OracleEngine(t.B, 0, 18)
    eng.marker_size, eng.r_pix = SIZE, scene.meas_prm.r_pix
    eng.set_state(*t.meas_state)
    i, left, right = (x[0] for x in t.h["rows"]["stereo"])
    eng.correct_pixels(i, left, right)
    out.update(zip(("pixel nominal", "pixel rot", "pixel P", "pixel prev"), eng.get_state()))
    return out


def test_the_oracle_gives_permuted_output_for_permuted_input(scene):
    whole, pi = _oracle(scene, np.arange(B)), permutation()
    moved = _oracle(scene, pi)
    assert same_rows(whole, moved, rows=pi)
    assert not same_rows({"n": whole["pose nominal"]}, {"n": moved["pose nominal"]})        # (the rows did move)
    for step, before in (("predict", scene.state[2]), ("pose", whole["predict P"]), ("pixel", scene.meas_state[2])):
        assert (whole[f"{step} P"] != before).any(axis=(1, 2)).mean() > 0.9, step           # (and every step did something)
