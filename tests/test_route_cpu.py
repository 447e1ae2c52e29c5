"""The launch policy (fbus-ekf_amd/csrc/ekf_route.hpp): which kernels a frame or a window call runs, as pure host functions.  A short
program, compiled with plain g++ against the header alone, prints frame_route / window_route / window_pack and the five predicates
that fbus_ekf_launch_info answers from, over the full cross product of handle states and call shapes; the rules are asserted here as
properties, restated from the documentation (include/fbus_ekf.h) -- never against a table printed by the code under test."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SIMDS = 1024
TILES = (SIMDS // 4, SIMDS // 2, SIMDS // 2 + 1, SIMDS + 1)     # <= a quarter, exactly half, half + 1, one round + 1
KS = (0, 7, 255, 256)
# the program's own names for the enum values (its switch fails to compile when a value is added or renamed)
PER_CALL, F64_FUSED, FUSED, TEAM, TABLED_RESIDENT, MEAS_RESIDENT = range(6)
W_ONE_WAVE, W_TEAM, W_TEAM_FRAMES, W_BY_FRAME = range(4)
PACK_NONE, PACK_TRAJ, PACK_TRAJ_NOISE = range(3)
POSE, PIXELS, CORNERS = -1, 0, 1
NEAREST, STACKED = 0, 1
COLS = ("dtype joseph mode noise lik tp tc tf nfm tiles kind M fr0 fr7 fr255 fr256 w0 w1 pack0 pack1 "
        "nr tf_st rpix rpred1 rpred8 split_auto split_off split_2 split_skew").split()

PROGRAM = r'''
#include "ekf_route.hpp"
#include <cstdio>
#include <cstdlib>
using namespace fbus;
static int fr(FrameRoute r)
{
    switch (r) {
        case FRAME_PER_CALL: return 0; case FRAME_F64_FUSED: return 1; case FRAME_FUSED: return 2; case FRAME_TEAM: return 3;
        case FRAME_TABLED_RESIDENT: return 4; case FRAME_MEAS_RESIDENT: return 5;
    }
    return -1;
}
static int wr(WindowRoute r)
{
    switch (r) { case WINDOW_ONE_WAVE: return 0; case WINDOW_TEAM: return 1; case WINDOW_TEAM_FRAMES: return 2; case WINDOW_BY_FRAME: return 3; }
    return -1;
}
static int pk(WindowPack p)
{
    switch (p) { case PACK_NONE: return 0; case PACK_TRAJ: return 1; case PACK_TRAJ_NOISE: return 2; }
    return -1;
}
static const int Ms4[5] = { 0, 1, 64, 65, 65536 }, Bs[5] = { 1, 63, 64, 100, 4197 };
int main(int argc, char** argv)
{
    // argv[1]: filters short of a whole number of tiles (0..63): the batch is given in FILTERS and reaches the key through tiles_of
    const int ragged = std::atoi(argv[1]);
    if (ragged < 0) {       // where the batch enters the key: (policy batch, the handle's own) -> tiles
        for (int pb : Ms4) for (int B : Bs) std::printf("%%d %%d %%d\n", pb, B, policy_tiles_of(pb, B));
        return 0;
    }
    const int tiles[4] = { %(tiles)s }, teams[4] = { 0, 1, 2, 4 }, Ms[3] = { 0, 1, 4 }, Ks[4] = { %(ks)s };
    for (int dtype = 32; dtype <= 64; dtype += 32) for (int joseph = 0; joseph < 2; ++joseph) for (int mode = 0; mode < 2; ++mode)
    for (int noise = 0; noise < 2; ++noise) for (int lik = 0; lik < 2; ++lik)
    for (int tp : teams) for (int tc : teams) for (int tf = 0; tf < 3; ++tf) for (int nfm = 0; nfm < 2; ++nfm)
    for (int t : tiles) for (int kind = -1; kind < 2; ++kind) for (int M : Ms) {
        RouteKey k;
        k.dtype = dtype; k.joseph = joseph; k.noise_on = noise; k.lik_on = lik; k.tiles = tiles_of(64 * t - ragged); k.simds = %(simds)d;
        k.team_predict = tp; k.team_correct = tc; k.team_frame = tf; k.no_frame_meas = nfm;
        std::printf("%%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d", dtype, joseph, mode, noise, lik, tp, tc, tf, nfm, t, kind, M);
        for (int K : Ks) std::printf(" %%d", fr(frame_route(k, (RouteKind)kind, mode, M, K)));
        for (int rows = 0; rows < 2; ++rows) std::printf(" %%d", wr(window_route(k, (RouteKind)kind, mode, M, rows)));
        for (int rows = 0; rows < 2; ++rows) std::printf(" %%d", pk(window_pack(k, rows)));
        // what fbus_ekf_launch_info answers from
        std::printf(" %%d %%d %%d %%d %%d", (int)noise_resident(k), (int)team_frames(k, ROUTE_MODE_STACKED), team_roles_pixels(k, M),
                    team_roles_predict(k, 1), team_roles_predict(k, 8));
        RouteKey s = k;
        std::printf(" %%d", meas_split_roles(s, M));
        s.meas_split = 0; std::printf(" %%d", meas_split_roles(s, M));
        s.meas_split = 2; std::printf(" %%d", meas_split_roles(s, M));
        s.square_port = false; std::printf(" %%d\n", meas_split_roles(s, M));
    }
    return 0;
}
''' % {"tiles": ", ".join(map(str, TILES)), "ks": ", ".join(map(str, KS)), "simds": SIMDS}


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    """{column: int array over the cross product}, and the same walk with every batch 63 filters short of its last tile"""
    d = tmp_path_factory.mktemp("route")
    src = d / "routes.cpp"
    src.write_text(PROGRAM)
    exe = d / "routes"
    # plain g++, the header alone: no HIP, no other header of the library
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fbus-ekf_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    out = []
    for ragged in (0, 63):
        r = subprocess.run([str(exe), str(ragged)], capture_output=True, text=True, check=True)
        out.append(np.array(r.stdout.split(), dtype=np.int64).reshape(-1, len(COLS)))
    n = 2 * 2 * 2 * 2 * 2 * 4 * 4 * 3 * 2 * 4 * 3 * 3
    assert out[0].shape == (n, len(COLS)) and (out[0] >= -1).all()
    batch = subprocess.run([str(exe), "-1"], capture_output=True, text=True, check=True).stdout
    return {c: out[0][:, i] for i, c in enumerate(COLS)}, out, np.array(batch.split(), dtype=np.int64).reshape(-1, 3)


# ---- the documented rules, restated -------------------------------------------------------------------------------------------------------
def _state(r):
    fp32, tab = r["dtype"] == 32, (r["noise"] | r["lik"]) == 1
    nr = (r["noise"] == 1) & (r["lik"] == 0) & fp32 & (r["tiles"] > SIMDS // 2)
    return fp32, tab, nr


def _team_frames(r, fp32, tab):
    follows = np.where(r["tf"] == 0, r["tp"] != 1, r["tf"] == 2)            # FBUS_TEAM_FRAME=1|2 overrides fbus_ekf_set_team
    always = (r["tf"] == 2) | (r["tp"] >= 2)
    return fp32 & (r["joseph"] == 0) & ~tab & follows & (always | (r["tiles"] <= SIMDS // 2))


def _roles_pixels(r, tab):
    by_size = np.where(r["tiles"] <= SIMDS // 4, 4, np.where(r["tiles"] <= SIMDS // 2, 2, 1))
    roles = np.where(r["tc"] >= 2, np.where(r["tc"] >= 3, 4, 2), by_size)
    return np.where((r["M"] < 2) | (r["tc"] == 1) | tab, 1, roles)


def _frames(r):
    return [(K, r[f"fr{K}"]) for K in KS]


def test_fp64_runs_per_call_or_its_one_fused_frame(routes):
    r = routes[0]
    fp32, tab, _ = _state(r)
    for K, fr in _frames(r):
        fused = ~fp32 & (r["kind"] == POSE) & (r["mode"] == STACKED) & (r["joseph"] == 0) & ~tab & (1 <= K <= 255)
        assert np.isin(fr[~fp32], (PER_CALL, F64_FUSED)).all()
        assert np.array_equal(fr == F64_FUSED, fused)
    assert (r["w0"][~fp32] == W_BY_FRAME).all() and (r["w1"][~fp32] == W_BY_FRAME).all()


def test_joseph_nearest_pose_frames_and_likelihood_frames_run_per_call(routes):
    r = routes[0]
    jn = (r["kind"] == POSE) & (r["joseph"] == 1) & (r["mode"] == NEAREST)
    for _, fr in _frames(r):
        assert (fr[jn] == PER_CALL).all()
        assert (fr[r["lik"] == 1] == PER_CALL).all()
    for w in (r["w0"], r["w1"]):
        assert (w[jn | (r["lik"] == 1)] == W_BY_FRAME).all()


def test_a_tabled_frame_is_resident_exactly_where_noise_resident_holds_and_the_call_is_not_excluded(routes):
    r = routes[0]
    fp32, tab, nr = _state(r)
    pose = r["kind"] == POSE
    for K, fr in _frames(r):
        excluded = np.where(pose, (r["joseph"] == 1) & (r["mode"] == NEAREST), (r["M"] == 0) | (r["nfm"] == 1)) | (K > 255)
        on = r["noise"] == 1
        assert np.array_equal((fr != PER_CALL)[on], (nr & ~excluded)[on])
        assert np.array_equal(fr == TABLED_RESIDENT, on & nr & ~excluded)         # ... and then it is the window kernel with the table
    # fbus_ekf_set_team, FBUS_TEAM_FRAME: ignored while a table is set -- a pure size rule
    assert (nr[r["tiles"] <= SIMDS // 2] == 0).all() and nr[(r["noise"] == 1) & (r["lik"] == 0) & fp32 & (r["tiles"] > SIMDS // 2)].all()


def test_untabled_fp32_frames(routes):
    r = routes[0]
    fp32, tab, _ = _state(r)
    tf, pose = _team_frames(r, fp32, tab), r["kind"] == POSE
    roles = np.where((r["kind"] == CORNERS) & (r["mode"] != STACKED), 1, _roles_pixels(r, tab))
    plain = fp32 & ~tab
    for K, fr in _frames(r):
        sel = plain & pose & ~((r["joseph"] == 1) & (r["mode"] == NEAREST))
        assert np.array_equal(fr[sel], np.where(tf & (K <= 255), TEAM, FUSED)[sel])     # (the fp32 fused frame takes any K)
        sel = plain & ~pose
        resident = (r["M"] > 0) & (r["nfm"] == 0) & (roles == 1) & (K <= 255)
        assert np.array_equal(fr[sel], np.where(resident, MEAS_RESIDENT, PER_CALL)[sel])
        assert not np.isin(fr[pose], (MEAS_RESIDENT,)).any() and not np.isin(fr[~pose], (FUSED, TEAM, F64_FUSED)).any()


def test_no_team_route_on_a_tabled_handle_without_team_predict_or_with_joseph(routes):
    r = routes[0]
    fp32, tab, _ = _state(r)
    team = np.zeros(len(tab), bool)
    for _, fr in _frames(r):
        team |= fr == TEAM
    team |= np.isin(r["w0"], (W_TEAM, W_TEAM_FRAMES)) | np.isin(r["w1"], (W_TEAM, W_TEAM_FRAMES))
    # (team_predict == 1 is "never" unless FBUS_TEAM_FRAME=2 overrides it: include/fbus_ekf.h, fbus_ekf_set_team)
    assert not team[tab | (r["joseph"] == 1) | ~fp32 | (r["kind"] != POSE) | ((r["tp"] == 1) & (r["tf"] != 2)) | (r["tf"] == 1)].any()
    forced = fp32 & ~tab & (r["joseph"] == 0) & (r["kind"] == POSE) & (r["tf"] == 2)
    assert (r["fr7"][forced] == TEAM).all() and (r["w0"][forced] == W_TEAM).all()


def test_a_resident_window_has_resident_frames_of_the_same_family(routes):
    """the premise of window == frames, bit for bit"""
    r = routes[0]
    for rows, w in ((0, r["w0"]), (1, r["w1"])):
        for K, fr in _frames(r):
            if K > 255:
                continue        # (a window's counts fit a byte)
            assert np.isin(fr[w == W_ONE_WAVE], (FUSED, TABLED_RESIDENT, MEAS_RESIDENT)).all()
            assert (fr[np.isin(w, (W_TEAM, W_TEAM_FRAMES))] == TEAM).all()
            assert np.isin(fr[w == W_BY_FRAME], (PER_CALL, F64_FUSED)).all()
        assert not (w == (W_TEAM_FRAMES, W_TEAM)[rows]).any()          # the team window writes no rows itself
    same = lambda w: np.where(np.isin(w, (W_TEAM, W_TEAM_FRAMES)), W_TEAM, w)
    assert np.array_equal(same(r["w0"]), same(r["w1"]))               # asking for rows moves no window between the kernel families
    # the family of a one-wave window follows the rows and the table
    one = r["w0"] == W_ONE_WAVE
    assert np.array_equal(r["fr7"][one] == TABLED_RESIDENT, r["noise"][one] == 1)
    assert np.array_equal(r["fr7"][one & (r["noise"] == 0)] == MEAS_RESIDENT, r["kind"][one & (r["noise"] == 0)] != POSE)


def test_window_pack(routes):
    r = routes[0]
    _, _, nr = _state(r)
    assert np.array_equal(r["pack0"], np.where(nr, PACK_TRAJ_NOISE, PACK_NONE))
    assert np.array_equal(r["pack1"], np.where(nr, PACK_TRAJ_NOISE, PACK_TRAJ))
    # on the one-wave routes (the only ones that ask): the table is read exactly where the frames read it
    one = r["w0"] == W_ONE_WAVE
    assert np.array_equal(r["pack0"][one] == PACK_TRAJ_NOISE, r["fr7"][one] == TABLED_RESIDENT)


def test_every_answer_depends_on_the_batch_through_its_tiles_alone(routes):
    _, (whole, ragged), batch = routes
    assert np.array_equal(whole, ragged)
    # ... and the batch is the policy batch where one is set, else the handle's own
    assert len(batch) == 25
    for pb, B, tiles in batch:
        assert tiles == -(-(pb if pb > 0 else B) // 64)


def test_launch_info_predicates_are_the_ones_the_routes_use(routes):
    r = routes[0]
    fp32, tab, nr = _state(r)
    assert np.array_equal(r["nr"] == 1, nr)
    assert np.array_equal(r["tf_st"] == 1, _team_frames(r, fp32, tab))      # (no mode in it: asked with the stacked mode)
    assert np.array_equal(r["rpix"], _roles_pixels(r, tab))
    one = ~fp32 | (r["tp"] == 1) | tab
    assert np.array_equal(r["rpred1"], np.where(one, 1, np.where(r["tp"] >= 2, np.minimum(r["tp"], 4), np.where(r["tiles"] <= SIMDS // 4, 3, 1))))
    assert np.array_equal(r["rpred8"], np.where(one, 1, np.where(r["tp"] >= 2, 4, np.where(r["tiles"] <= SIMDS // 2, 4, 1))))
    off = ~fp32 | (r["M"] < 2) | (r["tc"] == 1) | tab
    by_size = np.where(r["tiles"] <= SIMDS // 4, 4, np.where(r["tiles"] <= SIMDS // 2, 2, 0))
    assert np.array_equal(r["split_auto"], np.where(off, 0, np.where(r["tc"] >= 2, np.where(r["tc"] >= 3, 4, 2), by_size)))
    assert (r["split_off"] == 0).all() and (r["split_skew"] == 0).all()
    assert np.array_equal(r["split_2"], np.where(off, 0, 2))
    # ... and the routes follow them: the team frame where team_frames says so, the resident measurement frame where the update is one wave
    sel = fp32 & ~tab & (r["kind"] == POSE) & (r["mode"] == STACKED)
    assert np.array_equal(r["fr7"][sel] == TEAM, r["tf_st"][sel] == 1)
    sel = fp32 & ~tab & (r["kind"] == PIXELS) & (r["M"] > 0) & (r["nfm"] == 0)
    assert np.array_equal(r["fr7"][sel] == MEAS_RESIDENT, r["rpix"][sel] == 1)
    assert np.array_equal(r["fr7"][r["noise"] == 1] != PER_CALL,
                          ((r["nr"] == 1) & (r["fr7"] == TABLED_RESIDENT))[r["noise"] == 1])
