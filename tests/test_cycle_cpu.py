"""CPU suite: the composed fp64 reference of the IMM cycle (tests/cycle_ref.py) ALONE -- the conditions under which holding the device to
it (tests/test_cycle_gpu.py) means something.  Every decision of the mission has margin, the bank is alive, the counters follow the
header's rules in closed form, the mission is well conditioned in double (the oracle's literal covariance form against Joseph's), and
the reference SEES the slips the per-feature suites are blind to: each mutation of cycle_ref.MUTATIONS moves a compared output far
beyond its gate.  Every check prints its figure."""
import functools

import numpy as np
import pytest

import cycle_ref as R
from exits_plan import HALF_WIDTH

CELLS = ("A", "B", "C")


@functools.lru_cache(maxsize=None)
def base(name):
    return R.run_ref(name)


# ---- 1. decisions have margin ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CELLS)
def test_decisions_have_margin(name):
    cell, m, out = R.CELLS[name], R.mission(name), base(name)
    for c, o in enumerate(out):
        for kind in R.KINDS:
            nis, dof = o[kind]["nis"], o[kind]["dof"]
            assert (dof > 0).all()
            thr = m.gate[dof]
            margin = (np.abs(nis - thr) / thr).min()
            print(f"cell {name} stretch {c} {kind}: smallest |nis - thr| / thr = {margin:.3f}")
            assert margin >= HALF_WIDTH                      # (a failure here: another seed or outlier size, not another margin)
        lw = o["logw"].reshape(-1, cell.G)
        bound = o["ll_bound"][32].reshape(-1, cell.G)
        order = np.argsort(lw, axis=1)
        i, j = order[:, -1], order[:, -2]
        rows = np.arange(len(lw))
        gap = lw[rows, i] - lw[rows, j]
        ratio = gap / np.maximum(bound[rows, i], bound[rows, j])
        print(f"cell {name} stretch {c}: top two logw differ by {gap.min():.3f} .. {gap.max():.3f} nats, at least {ratio.min():.0f} x the fp32 ll bound "
              f"({bound.max():.2e})")
        assert ratio.min() >= 100
        cj = np.exp(o["mix"]["logc"])
        print(f"cell {name} stretch {c}: smallest c_j = {cj.min():.3e}")
        assert (cj > 0).all()


# ---- 2. the bank is alive -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CELLS)
def test_the_bank_is_alive(name):
    cell, out = R.CELLS[name], base(name)
    for c, o in enumerate(out):
        top = o["fuse"]["weight"].reshape(-1, cell.G).max(axis=1)
        alive = ((top > 0.4) & (top < 0.999)).mean()
        best = np.bincount(o["fuse"]["best"], minlength=cell.G)
        print(f"cell {name} stretch {c}: largest weight {top.min():.3f} .. {top.max():.3f}, inside (0.4, 0.999) in {alive:.2f} of the groups; best by member "
              f"{best}; applied / rejected {o['count']}")
        assert alive >= 0.5
        assert (best > 0).sum() >= 2                         # `best` names different members in different groups
        assert np.array_equal(o["fuse"]["weight"], o["mix"]["weight"])
        for kind in R.KINDS:
            assert o["count"][kind][0] > 0 and o["count"][kind][1] > 0, (c, kind)
    # mixing moved every member: no record of the last stretch equals its own before the mix
    last = out[-1]
    assert not np.array_equal(last["mix"]["state"][0], last["rows"]["state"][0])


# ---- 3. bookkeeping in closed form -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CELLS)
def test_the_counters_follow_the_headers_rules(name):
    """rows: all 7 rows of each used marker per pose frame (28 stacked with M = 4, 7 nearest; the Matlab dialect's dof is 3 per marker, its
    rows are 7), 8 per marker in view of the left camera; depth 1, velocity 3, rows m = 2, each only where applied.  applied: one per
    window frame and applied sensor update; rejected: one per sensor update the gate refused."""
    cell, m, out = R.CELLS[name], R.mission(name), base(name)
    for c, o in enumerate(out):
        app = {k: o[k]["applied"].astype(np.int64) for k in R.KINDS}
        per_frame = sum(R.rows_per_frame(cell, m.ids[c, f]) for f in range(R.F_WIN))
        rows = per_frame + 1 * app["depth"] + 3 * app["velocity"] + R.M_ROWS * app["rows"]
        applied = R.F_WIN + app["depth"] + app["velocity"] + app["rows"]
        rejected = 3 - (app["depth"] + app["velocity"] + app["rows"])
        print(f"cell {name} stretch {c}: rows {rows.min()} .. {rows.max()}, applied {applied.min()} .. {applied.max()}, rejected up to {rejected.max()}")
        assert np.array_equal(o["sums"][1], rows) and np.array_equal(o["sums"][2], applied) and np.array_equal(o["sums"][3], rejected)
        assert (o["window"]["applied"] == 1).all()
        for k in R.KINDS:
            assert (o[k]["dof"] == {"depth": 1, "velocity": 3, "rows": R.M_ROWS}[k]).all()
            # the outlier lanes are the rejected ones, and only they (the other lanes' readings are drawn at the sensor's own size)
            assert not o[k]["applied"][R.outlier_lanes(cell, k)].any()
    if cell.window != "left":
        assert (m.ids >= 0).all() and rows.min() >= 3 * R.rows_per_frame(cell, m.ids[0, 0]).min()


# ---- 4. well conditioned in double -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CELLS)
def test_the_literal_and_the_joseph_form_agree(name):
    """the whole mission in the oracle's literal covariance form (I - K H) P and in Joseph's: every stage within HALF of the fp64 gates"""
    clean = base(name)
    rows = R.compare(name, R.run_ref(name, joseph=True, seeds=[dict(logw=o["logw"]) for o in clean]), clean, 64)
    ratio, w = R.worst(rows)
    print(f"cell {name}: literal against Joseph, worst figure / fp64 gate = {ratio:.3g} ({w[0]}: {w[1]} {w[2]:.3e} against {w[3]:.1e})")
    assert ratio <= 0.5, R.failing([(a, b, e, 0.5 * g) for a, b, e, g in rows])


# ---- 5. the reference sees the slips ---------------------------------------------------------------------------------------------------------

CASES = [(mut, cell if cell != "any" else "B") for mut, cell in R.MUTATIONS.items()] + [("depth_var", "A"), ("wrong_member", "A")]


@pytest.mark.parametrize("mutation,name", CASES)
def test_the_reference_sees_the_slip(mutation, name):
    """free-running against the fp64 gates, and re-seeded per stretch from the clean run (as tests/test_cycle_gpu.py re-seeds the reference
    from the device) against the fp32 gates"""
    clean = base(name)
    free = R.compare(name, R.run_ref(name, mutation=mutation), clean, 64)
    seeded = R.compare(name, R.run_ref(name, mutation=mutation, seeds=R.seeds_of(clean)), clean, 32, seeded=True)
    # fp64, free-running: the factor is taken over the figures that HAVE a gate (what the slip does downstream); the exact figures
    # (integers, bits) that differ are listed beside it.  fp32: the reference is re-seeded behind every mix, which erases what a slip
    # INSIDE the mix (the rotation, prev_id) does downstream -- there the exact figure of the mix itself is what sees it, and a
    # differing exact figure counts as beyond any factor
    f64, w64 = R.worst([r for r in free if r[3] > 0])
    f32, w32 = R.worst(seeded)
    exact = sorted({f"{r[0].split()[1]} {r[1]}" for r in free + seeded if r[3] == 0 and r[2] > 0})
    print(f"{mutation} in cell {name}: {f64:.3g} x the fp64 gate ({w64[0]}: {w64[1]}), {f32:.3g} x the fp32 gate ({w32[0]}: {w32[1]}); exact figures "
          f"that differ: {', '.join(exact) or 'none'}")
    assert f64 >= 100 and f32 >= 10


def test_the_reseeded_clean_reference_is_the_clean_reference():
    """the re-seeding itself moves nothing: a clean reference restarted from the clean run's own states repeats it"""
    clean = base("B")
    again = R.run_ref("B", seeds=R.seeds_of(clean))
    ratio, w = R.worst(R.compare("B", again, clean, 64))
    print(f"re-seeded clean run against the free-running one: worst figure / fp64 gate = {ratio:.3g}")
    assert ratio == 0
