"""GPU suite: a filter's results depend on the filter alone -- not on its place in the batch, the batch's size, or what its neighbours hold
(include/fbus_ekf.h: "filters are independent"; what sharding, one-hypothesis-per-filter sweeps and hypothesis groups rest on).

The cells: every handle state of tests/route_cells.py (each placed in its size class with set_policy_batch) x its window shapes, single
frames at K = 0, 1 and 7 with M = 3 and 4, and the six NIS entry points (fp32 on the library's own team choice and pinned to one wave,
fp64; one gated cell per kind) -- at B = 193 filters: three full 64-filter tiles and a tile of one.  Every per-filter input differs from
filter to filter and belongs to the filter's identity; about half the cells give every filter its own IMU period.

Each cell runs once as it is (V0) and then
  V1  the same filters in the order support.permutation(): no filter keeps its lane, most change tile, the tail filter sits in a full tile
  V2  as two handles of filters 0 .. 100 and 101 .. 192: a cut inside a tile; single frames pass SLICES of the whole job's arrays (with
      M = 3 the second handle's ids start 1212 bytes in, off the 16-byte boundary of the vector fetch)
  V3  as handles of ONE filter, for filters 0, 100 and 192
  V4  with 82 filters broken (support.poison_set: every seventh, a whole wave but one lane, the last but one; NaN / Inf / -P / NaN inputs /
      zero rotation): every call returns OK and the 111 clean filters are compared, nothing is asked of the broken ones
  V5  with tile 1 absent (all skip bytes set; all ids -1): the other 129 filters are compared, the absent tile reports applied = 0 and
      finite records -- the initial ones, bit for bit, where the cell has no IMU sample
and every output -- get_state(), applied(), NIS and dof, the likelihood sums, the trajectory rows -- holds the same BITS as V0's for the
same filter.  No tolerance anywhere."""
import collections

import numpy as np
import pytest

from fbus_ekf import gating
from route_cells import CFGS, NEAREST, STACKED, Cfg, data_of, frame_route, frame_rows, make, one_frame, shapes_of, update_nis, window, window_route
from support import ALONE, B_IND, permutation, poison_set, ragged_cut, same_rows

pytestmark = pytest.mark.gpu

B = B_IND
TILE1 = np.arange(64, 128)
VARIANTS = ("V1 permuted", "V2 ragged cut", "V3 alone", "V4 poisoned neighbours", "V5 absent tile")

# call: "window" (arg = (kcount, rows)) | "frame" (arg = K) | "nis" (the per-call update's NIS entry point); per: every filter its own IMU period
Cell = collections.namedtuple("Cell", "call kind mode M arg per gate", defaults=(None, False, False))
FRAMES = [Cell("frame", "pose", STACKED, 4, 0), Cell("frame", "pose", NEAREST, 3, 1, True), Cell("frame", "pose", STACKED, 4, 7, True),
          Cell("frame", "stereo", STACKED, 4, 0), Cell("frame", "left", STACKED, 3, 1), Cell("frame", "stereo", STACKED, 4, 7, True),
          Cell("frame", "corners", NEAREST, 3, 0), Cell("frame", "corners", STACKED, 3, 1), Cell("frame", "corners", STACKED, 4, 7, True)]
NIS = [Cell("nis", "pose", NEAREST, 4), Cell("nis", "pose", STACKED, 3), Cell("nis", "left", STACKED, 4), Cell("nis", "stereo", STACKED, 3),
       Cell("nis", "corners", NEAREST, 3), Cell("nis", "corners", STACKED, 4)]
GATED = [Cell("nis", kind, STACKED, 4, gate=True) for kind in ("pose", "left", "stereo", "corners")]
# the NIS cells' handle states: the policy batch is the job's own 193 filters (four tiles: the team forms wherever the library chooses them)
NIS_CFGS = [Cfg("nis f32", B), Cfg("nis f32 set_team(0,1)", B, team=(0, 1)), Cfg("nis f64", B, dtype=64)]


def cells_of(cfg):
    if cfg in NIS_CFGS:
        return NIS + (GATED if cfg is NIS_CFGS[0] else [])
    return [Cell("window", kind, mode, M, (kc, rows), i % 2 == 1) for i, (kind, mode, M, kc, rows) in enumerate(shapes_of(cfg))] + FRAMES


# ---- scenes: the whole job and what each variant makes of it, once per (record type, state size, dialect) ----------------------------------
_SCENES = {}


def scene(cfg, gate, variant):
    """the Data objects of a variant ("V0": the one of the whole job)"""
    base = data_of(cfg, B)
    key = (id(base), gate, variant)
    if key not in _SCENES:
        d = scene(cfg, False, "V0").with_outliers() if gate else base
        if variant == "V0":
            out = d
        elif variant == VARIANTS[0]:
            out = [d.take(permutation())]
        elif variant == VARIANTS[1]:
            out = [d.take(part) for part in ragged_cut()]
        elif variant == VARIANTS[2]:
            out = [d.take([b]) for b in ALONE]
        elif variant == VARIANTS[3]:
            out = [d.poisoned(*poison_set())]
        else:
            out = [d.absent(TILE1, how) for how in ("skip", "ids")]
        _SCENES[key] = out
    return _SCENES[key]


# ---- one cell on one handle ---------------------------------------------------------------------------------------------------------------------
def run(cfg, d, cell):
    """every output of the cell as {name: array, filters along axis 0}, from a fresh handle of d's filters in the cell's state"""
    with make(cfg, d, cell.kind != "pose", filters=d.ids) as f:
        nis = traj = None
        if cell.call == "window":
            traj = window(f, d, cell.kind, cell.mode, cell.M, cell.arg[0], cell.arg[1], per=cell.per)
        elif cell.call == "frame":
            one_frame(f, d, cell.kind, cell.mode, cell.M, cell.arg, per=cell.per)
        else:
            if cell.gate:
                f.set_gate(gating.chi2_gate(0.999))
            nis = update_nis(f, d, cell.kind, cell.mode, cell.M)
        f.sync()                                                       # (a call that did not return OK has raised)
        out = dict(zip(("nominal", "rot", "P", "prev"), f.get_state()), applied=f.applied())
        if nis is not None:
            out["nis"], out["dof"] = nis
        if cfg.lik:
            out.update(zip(("ll", "ll rows", "ll applied", "ll rejected"), f.loglik()))
        if traj is not None:
            out.update((name, np.moveaxis(t.cpu().numpy(), 0, 1)) for name, t in zip(("traj nominal", "traj pdiag", "traj applied"), traj))
    return out


_V0 = {}


def baseline(cfg):
    """V0 of every cell of a handle state, computed once and kept while that state's tests run"""
    if cfg.name not in _V0:
        _V0.clear()
        _V0[cfg.name] = [run(cfg, scene(cfg, cell.gate, "V0"), cell) for cell in cells_of(cfg)]
        for out in _V0[cfg.name]:
            for x in out.values():
                x.setflags(write=False)
    return _V0[cfg.name]


def samples_of(cell):
    return sum(cell.arg[0]) if cell.call == "window" else (cell.arg if cell.call == "frame" else 0)


def check(variant, cfg, cell, v0):
    what = f"{cfg}: {cell}: {variant}"
    scenes = scene(cfg, cell.gate, variant)
    if variant in VARIANTS[:3]:                                        # the same filters elsewhere: every filter of every handle
        for d in scenes:
            assert same_rows(v0, run(cfg, d, cell), rows=d.ids), what
    elif variant == VARIANTS[3]:
        clean = np.setdiff1d(np.arange(B), poison_set()[0])
        assert same_rows(v0, run(cfg, scenes[0], cell), clean, clean), what
    else:
        others = np.setdiff1d(np.arange(B), TILE1)
        for d in scenes:
            out = run(cfg, d, cell)
            assert same_rows(v0, out, others, others), what
            assert (out["applied"][TILE1] == 0).all() and all(np.isfinite(out[k][TILE1]).all() for k in ("nominal", "rot", "P")), what
            if "traj applied" in out:
                assert (out["traj applied"][TILE1] == 0).all() and np.isfinite(out["traj nominal"][TILE1]).all(), what
            if samples_of(cell) == 0:                                    # nothing has touched the absent tile's records
                first = d.meas_state if cell.kind != "pose" else d.state
                first = {k: np.asarray(x, out[k].dtype) for k, x in zip(("nominal", "rot", "P", "prev"), first)}
                assert same_rows(first, out, TILE1, TILE1), what


ALL_CFGS = CFGS + NIS_CFGS


@pytest.mark.parametrize("cfg,variant", [(c, v) for c in ALL_CFGS for v in VARIANTS], ids=lambda x: x if isinstance(x, str) else repr(x))
def test_a_filter_is_itself_wherever_it_stands(cfg, variant):
    failed = []
    for cell, v0 in zip(cells_of(cfg), baseline(cfg)):
        try:
            check(variant, cfg, cell, v0)
        except AssertionError as e:                                    # (every cell of the state is reported, not the first alone)
            print(f"FAILED {cfg}: {cell}: {variant}: {str(e).splitlines()[0] if str(e) else ''}")
            failed.append(cell)
    assert not failed, f"{len(failed)} of {len(cells_of(cfg))} cells"


def test_the_gated_cells_reject_and_accept():
    """the gate's branch is taken both ways beside each other: at least a tenth of the filters rejected, at least half accepted"""
    cfg = NIS_CFGS[0]
    for cell, v0 in zip(cells_of(cfg), baseline(cfg)):
        if cell.gate:
            rejected = (v0["applied"] == 0) & (v0["dof"] > 0)
            print(f"{cell.kind}: rejected {rejected.mean():.3f}, accepted {(v0['applied'] == 1).mean():.3f}")
            assert rejected.mean() >= 0.1 and (v0["applied"] == 1).mean() >= 0.5, cell


def test_the_baseline_does_something_everywhere():
    """V0 itself: applied flags both ways beside each other, and the filters' results differ from filter to filter"""
    for cfg in (CFGS[0], CFGS[12], NIS_CFGS[0]):
        for cell, v0 in zip(cells_of(cfg), baseline(cfg)):
            if cell.M > 0:
                assert 0 < v0["applied"].sum() < B, (cfg, cell)
            assert len(np.unique(v0["P"].reshape(B, -1), axis=0)) == B, (cfg, cell)


def test_the_cut_hands_over_slices_of_the_whole_jobs_arrays():
    """V2's second handle reads the whole job's single-frame arrays from filter 101 on, no copies: with M = 3 its ids start 1212 bytes into
    their array, off the 16-byte boundary; one filter alone (V3) likewise"""
    d = scene(CFGS[0], False, VARIANTS[1])[1]
    ids, pos, _, skip = frame_rows(d, "pose", 0, 3)
    assert (ids.storage_offset(), pos.storage_offset(), skip.storage_offset()) == (101 * 3, 101 * 9, 101) and ids.is_contiguous()
    assert ids.data_ptr() % 16 == 1212 % 16 != 0 and len(ids) == 92
    ids4 = frame_rows(d, "pose", 0, 4)[0]
    assert ids4.data_ptr() - d.src.rows["pose"][0].data_ptr() == 101 * 16               # (M = 4: the owner's own tensor)
    one = scene(CFGS[0], False, VARIANTS[2])[1]
    assert frame_rows(one, "stereo", 0, 3)[1].storage_offset() == 100 * 24 and one.B == 1


def test_the_poison_is_in_the_records():
    """V4's handles hold what support.poisoned_state made, NaN, Inf and -P included: set_state passes it on as it is (what the kernels make
    of those filters is not asked)"""
    S, form = poison_set()
    for cfg in (CFGS[0], CFGS[12]):
        d = scene(cfg, False, VARIANTS[3])[0]
        with make(cfg, d, False, filters=d.ids) as f:
            got = dict(zip(("nominal", "rot", "P", "prev"), f.get_state()))
        assert same_rows({k: np.asarray(x, got[k].dtype) for k, x in zip(("nominal", "rot", "P", "prev"), d.state)}, got)
        assert np.isnan(got["nominal"][S[form == 0]]).all() and np.isposinf(got["nominal"][S[form == 1], 0]).all()
        assert (got["P"][S[form == 2], 0, 0] < 0).all() and (got["rot"][S[form == 4]] == 0).all()


def test_the_cells_reach_every_route():
    """the cells visit every value of both route enums (asked of the handles, nothing launched)"""
    frames, windows = set(), set()
    for cfg in CFGS:
        with make(cfg, data_of(cfg, B), False) as f:
            for cell in cells_of(cfg):
                if cell.call == "window":
                    windows.add(window_route(f, cfg, cell.kind, cell.mode, cell.M, len(cell.arg[0]), cell.arg[1]))
                    frames.update(frame_route(f, cfg, cell.kind, cell.mode, cell.M, K) for K in cell.arg[0])
                else:
                    frames.add(frame_route(f, cfg, cell.kind, cell.mode, cell.M, cell.arg))
    assert frames == {"per_call", "f64_fused", "fused", "team", "tabled_resident", "meas_resident"}
    assert windows == {"one_wave", "team", "team_frames", "by_frame"}
