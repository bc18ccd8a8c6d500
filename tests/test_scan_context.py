"""Place recognition on the device (include/fbr.h "place recognition", csrc/k_scancontext.hip):
descriptors against the model cell for cell, the exhaustive search against the model (keyframe and
shift exact, distance within 1e-9), the incremental store, the loop closure that the radius search
has lost to drift, and relocalisation without a pose guess.

Bars:
  * descriptors: bytes equal to the model's with the probe's cells (tests/native/sc_probe.cpp is the
    device's own bin function, checked against the float64 bins in tests/test_sc_model.py);
  * search: both sides sum at most 64 terms of magnitude at most 1 in double in the same order, so
    they differ by about 1e-14; 1e-9 leaves five orders of magnitude and sits three below the 1e-6
    margin every compared ranking has (tests/test_sc_model.py);
  * loop closure under drift: the fields of test_loop_closure_matches_model against loop_model.perform
    on the poses with keyframe 19 re-anchored at the hypothesis; pose_corrected within twice the
    model's own error of ground truth (the model's: 0.0078 m / 8.4e-5 rad, sc_fixtures.MODEL_LOOP_ERR);
  * relocalisation: the winner within 1e-4 m / 1e-4 rad of the oracle registered from the same
    hypothesis, and within 0.05 m / 0.01 rad of ground truth.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import loop_model as LM
import sc_fixtures as F
import sc_model as SM
import test_loop_closure as TL
from feature_base_pointcloud_registration_amd import api
from feature_base_pointcloud_registration_amd.fbr_types import (FBR_LOOP_CLOSED, FBR_LOOP_NO_CANDIDATE, KEYPOSE,
                                                                POINT_XYZI, FbrScMatch, FbrScParams, default_params,
                                                                loop_params, sc_params)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fbr_sc_params_default", "fbr_sc_describe", "fbr_sc_update", "fbr_sc_descriptor", "fbr_sc_query",
               "fbr_sc_detect_loop_closure", "fbr_perform_loop_closure_sc")
DIST_TOL = 1e-9
EMPTY = np.zeros(0, POINT_XYZI)


def test_sc_structs_defaults_and_symbols():
    lib = ctypes.CDLL(api.lib_path())
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in api.EXPORTED_SYMBOLS
    assert ctypes.sizeof(FbrScParams) == 32 and ctypes.sizeof(FbrScMatch) == 48
    p = FbrScParams()
    api.lib().fbr_sc_params_default(ctypes.byref(p))
    assert (p.n_ring, p.n_sector, p.max_radius, p.lidar_height, p.dist_threshold) == (20, 60, 80.0, 2.0, np.float32(0.2))
    assert bytes(p) == bytes(sc_params())
    assert api.lib().fbr_abi_version() == 4
    for name in ("sc_describe", "sc_update", "sc_descriptor", "sc_query", "sc_detect_loop_closure",
                 "perform_loop_closure_sc", "relocalize"):
        assert callable(getattr(api.Context, name))


def cloud(xyz):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    c = np.zeros(len(xyz), POINT_XYZI)
    c["x"], c["y"], c["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return c


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    with api.Context(default_params(16, 1800)) as c:
        yield c


# ---- descriptors -----------------------------------------------------------------------------------
def random_cloud(rng, sp, n):
    r = rng.uniform(0.0, float(np.float32(sp.max_radius)) * 1.05, n)
    th = rng.uniform(-np.pi, np.pi, n)
    return np.stack([r * np.cos(th), r * np.sin(th), rng.uniform(-4.0, 6.0, n)], 1).astype(np.float32)


def descriptor_cases():
    sp = sc_params()
    R = np.float32(sp.max_radius)
    below = np.nextafter(R, np.float32(0))
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    rng = np.random.default_rng(21)
    edge = np.float32([[1.0, 0.0, 0.5], [1.0, -0.0, 0.25], [-1.0, 0.0, 1.0], [-1.0, -0.0, 0.75], [R, 0.0, 3.0],
                       [below, 0.0, 1.5], [0.0, 0.0, 1.0], [1.0, -1e-30, 2.0], [0.0, R, 1.0], [0.0, -below, 0.125]])
    cases = {
        "empty": (sp, np.zeros((0, 3), np.float32)),
        "one_point": (sp, np.float32([[10.0, 3.0, -0.5]])),
        "two_in_one_cell": (sp, np.float32([[10.0, 3.0, -0.5], [10.1, 3.05, 0.25], [10.05, 3.0, -1.0]])),
        "below_ground": (sp, np.float32([[10.0, 3.0, -2.0], [5.0, 5.0, -7.5], [20.0, -3.0, -2.125]])),
        "non_finite": (sp, np.float32([[nan, 1.0, 1.0], [1.0, inf, 1.0], [2.0, 2.0, nan], [2.0, 2.0, inf], [2.0, 2.0, -inf],
                                       [-inf, nan, 0.0], [30.0, 30.0, 1.0]])),
        "edges": (sp, edge),
        "shape_1x2": (sc_params(n_ring=1, n_sector=2), random_cloud(rng, sp, 500)),
        "shape_20x60": (sp, random_cloud(rng, sp, 3000)),
        "shape_32x64": (sc_params(n_ring=32, n_sector=64, max_radius=55.5, lidar_height=1.25), random_cloud(rng, sp, 3000)),
        # more than one 4096-point pass per workgroup column: 18 passes merge in the slot
        "n70000": (sp, random_cloud(rng, sp, 70000)),
        "n4097": (sp, random_cloud(rng, sp, 4097)),
    }
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(descriptor_cases()))
def test_descriptor_matches_model(ctx, name):
    sp, pts = descriptor_cases()[name]
    ref = SM.descriptor(pts, sp, SM.probe_cells(pts, sp))
    n_c = len(pts) // 3
    d = ctx.sc_describe(cloud(pts[:n_c]), cloud(pts[n_c:]), sp)  # corner then surf
    assert d.shape == (sp.n_ring, sp.n_sector)
    assert np.array_equal(bits(d), bits(ref)), np.argwhere(bits(d) != bits(ref))[:5]
    assert np.array_equal(bits(SM.probe_descriptor(pts, sp)), bits(ref))
    # any point order, any corner / surf split: the same bytes
    perm = np.random.default_rng(3).permutation(len(pts))
    assert ctx.sc_describe(cloud(pts[perm]), EMPTY, sp).tobytes() == d.tobytes()
    assert ctx.sc_describe(EMPTY, cloud(pts[perm[::-1]]), sp).tobytes() == d.tobytes()
    away = SM.edge_margin(pts, sp) >= 1e-3 if len(pts) else np.zeros(0, bool)
    if name in ("shape_20x60", "shape_32x64", "n70000"):  # and the pure float64 model away from the bin edges
        p = pts[away]
        assert np.array_equal(bits(ctx.sc_describe(cloud(p), EMPTY, sp)), bits(SM.descriptor(p, sp)))
    if name == "empty" or name == "below_ground":
        assert not d.any()
    if name == "one_point":
        assert np.count_nonzero(d) == 1 and d.max() == 1.5
    if name == "two_in_one_cell":
        assert np.count_nonzero(d) == 1 and d.max() == 2.25
    if name == "non_finite":
        assert np.count_nonzero(d) == 1 and d.max() == 3.0
    if name == "edges":
        S = sp.n_sector
        assert (d[0, 0], d[0, S // 2], d[-1, 0], d[0, S - 1], d[-1, 3 * S // 4]) == (3.0, 3.0, 3.5, 4.0, 2.125)
        assert np.count_nonzero(d) == 5
    if name == "n70000":
        assert np.count_nonzero(d) == d.size


def add_keyframes(ctx, poses, corners, surfs):
    for k in range(len(poses)):
        ctx.keyframes_add(poses[k], corners[k], surfs[k])


@pytest.mark.gpu
def test_pending_keyframes_are_described_in_one_update(ctx):
    """Five pending keyframes whose third is empty; fbr_sc_descriptor equals fbr_sc_describe."""
    sp = sc_params()
    rng = np.random.default_rng(8)
    sizes = [(300, 2500), (0, 900), (0, 0), (5000, 4200), (17, 0)]
    clouds = [(cloud(random_cloud(rng, sp, a)), cloud(random_cloud(rng, sp, b))) for a, b in sizes]
    ctx.keyframes_reset()
    add_keyframes(ctx, F.search_poses(5), [c for c, _ in clouds], [s for _, s in clouds])
    assert ctx.sc_update(sp) == 5 and ctx.sc_update(sp) == 0
    for k, (c, s) in enumerate(clouds):
        stored = ctx.sc_descriptor(k, sp)
        assert stored.tobytes() == ctx.sc_describe(c, s, sp).tobytes(), k
        pts = np.concatenate([SM.xyz(c), SM.xyz(s)])
        assert np.array_equal(bits(stored), bits(SM.descriptor(pts, sp, SM.probe_cells(pts, sp)))), k
    assert not ctx.sc_descriptor(2, sp).any()
    with pytest.raises(api.FbrError):
        ctx.sc_descriptor(5, sp)
    ctx.keyframes_reset()


# ---- search ----------------------------------------------------------------------------------------
def load_candidates(ctx, case):
    sp, cands = case["sp"], case["cands"]
    poses = F.search_poses(len(cands))
    ctx.keyframes_reset()
    add_keyframes(ctx, poses, [F.cloud_of(C, sp) for C in cands], [EMPTY] * len(cands))
    return poses


def check_matches(got, want, poses, sp):
    assert [(m["keyframe"], m["shift"]) for m in got] == [(k, s) for k, s, _ in want]
    for m, (k, s, d) in zip(got, want):
        assert abs(m["distance"] - d) <= DIST_TOL, (m, d)
        assert np.array_equal(bits(m["pose_guess"]), bits(SM.pose_guess(LM.pose_of(poses[k]), s, sp.n_sector))), m


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(F.search_cases()))
def test_search_matches_model(ctx, name):
    case = F.search_cases()[name]
    sp, q, cands = case["sp"], case["query"], case["cands"]
    poses = load_candidates(ctx, case)
    qc = F.cloud_of(q, sp)
    assert np.array_equal(ctx.sc_describe(qc, EMPTY, sp), q)
    ref = SM.rank(q, cands)
    for k in case["ks"]:
        got = ctx.sc_query(EMPTY, qc, k, sp)  # (the query as a surf cloud: the split does not matter)
        assert len(got) == min(k, len(cands))
        print(name, "k =", k, [(m["keyframe"], m["shift"], m["distance"]) for m in got[:4]])
        check_matches(got, ref[:k], poses, sp)
    if cands:
        assert ctx.sc_update(sp) == 0 and np.array_equal(ctx.sc_descriptor(len(cands) - 1, sp), cands[-1])
    if name == "edges":
        got = ctx.sc_query(qc, EMPTY, 8, sp)
        assert [(m["keyframe"], m["shift"]) for m in got[:3]] == [(0, 59), (1, 0), (2, 1)]
        assert got[-1]["keyframe"] == 6 and got[-1]["distance"] == 1.0
    if name == "period":
        assert (got[0]["keyframe"], got[0]["shift"]) == (0, 7)
    ctx.keyframes_reset()


@pytest.mark.gpu
def test_query_rejects_bad_arguments(ctx):
    qc = F.cloud_of(F.search_cases()["n1"]["query"], sc_params())
    for bad in (dict(n_ring=0), dict(n_ring=33), dict(n_sector=1), dict(n_sector=65), dict(max_radius=0.0),
                dict(max_radius=np.inf), dict(lidar_height=np.nan), dict(dist_threshold=-1.0)):
        with pytest.raises(api.FbrError) as e:
            ctx.sc_query(qc, EMPTY, 4, sc_params(**bad))
        assert e.value.status == -1, bad
        with pytest.raises(api.FbrError):
            ctx.sc_update(sc_params(**bad))
    for k in (0, 17):
        with pytest.raises(api.FbrError) as e:
            ctx.sc_query(qc, EMPTY, k)
        assert e.value.status == -1


# ---- the incremental store -------------------------------------------------------------------------
@pytest.mark.gpu
def test_store_is_incremental(ctx):
    case = F.search_cases()["n65"]
    sp, q, cands = case["sp"], case["query"], case["cands"][:12]
    poses = F.search_poses(len(cands))
    clouds = [F.cloud_of(C, sp) for C in cands]
    qc = F.cloud_of(q, sp)
    ctx.keyframes_reset()
    add_keyframes(ctx, poses[:9], clouds[:9], [EMPTY] * 9)
    assert ctx.sc_update(sp) == 9
    add_keyframes(ctx, poses[9:], clouds[9:], [EMPTY] * 3)
    assert ctx.sc_update(sp) == 3 and ctx.sc_update(sp) == 0
    ref = SM.rank(q, cands)
    r1, n1 = ctx.sc_query(qc, EMPTY, 12, sp, raw=True)
    r2, n2 = ctx.sc_query(qc, EMPTY, 12, sp, raw=True)
    assert n1 == n2 == 12 and bytes(r1) == bytes(r2)  # identical queries: identical bytes
    got = [r1[i].as_dict() for i in range(n1)]
    check_matches(got, ref, poses, sp)
    # set_pose moves the hypothesis and nothing else; no descriptor is computed again
    best = ref[0][0]
    moved = poses.copy()
    moved["x"][best] += np.float32(7.5)
    moved["yaw"][best] = np.float32(1.1)
    ctx.keyframes_set_pose(best, moved[best])
    assert ctx.sc_update(sp) == 0
    again = ctx.sc_query(qc, EMPTY, 12, sp)
    assert [(m["keyframe"], m["shift"], m["distance"]) for m in again] == [(m["keyframe"], m["shift"], m["distance"])
                                                                          for m in got]
    check_matches(again, ref, moved, sp)
    assert not np.array_equal(again[0]["pose_guess"], got[0]["pose_guess"])
    assert all(np.array_equal(a["pose_guess"], b["pose_guess"]) for a, b in zip(again[1:], got[1:]))
    # another n_sector rebuilds the store
    sp2 = sc_params(n_sector=40)
    assert ctx.sc_update(sp2) == 12
    pts = SM.xyz(clouds[4])
    assert np.array_equal(bits(ctx.sc_descriptor(4, sp2)), bits(SM.descriptor(pts, sp2, SM.probe_cells(pts, sp2))))
    assert ctx.sc_update(sp) == 12 and np.array_equal(ctx.sc_descriptor(4, sp), cands[4])
    # keyframes_reset empties it
    ctx.keyframes_reset()
    assert ctx.sc_update(sp) == 0 and ctx.sc_query(qc, EMPTY, 4, sp) == []
    with pytest.raises(api.FbrError):
        ctx.sc_descriptor(0, sp)
    add_keyframes(ctx, poses[:2], clouds[:2], [EMPTY] * 2)
    assert ctx.sc_update(sp) == 2 and np.array_equal(ctx.sc_descriptor(1, sp), cands[1])
    ctx.keyframes_reset()


# ---- loop closure under drift ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def drift_ctx():
    L = F.loop_drift()
    with api.Context(L["P"]) as c:
        add_keyframes(c, L["poses"], L["corners"], L["surfs"])
        yield c


def raw_bytes(r):
    return ctypes.string_at(ctypes.addressof(r), ctypes.sizeof(r))


def stored_poses(c, L):
    """The key poses as the radius search sees them: detect from every prefix would be long; the
    calls that read them are compared before and after instead."""
    return c.detect_loop_closure(TL.STAMP, L["lp"]), c.detect_loop_closure(TL.STAMP, loop_params(search_radius=100.0))


@pytest.mark.gpu
def test_loop_closure_under_drift_matches_model(drift_ctx):
    L = F.loop_drift()
    c, lp, sp, m = drift_ctx, L["lp"], L["sp"], L["model"]
    before = stored_poses(c, L)
    assert before[0] is None and before[1] is not None  # the radius search has lost the loop
    found, match = c.sc_detect_loop_closure(TL.STAMP, lp, sp)
    assert found == (19, 0) == L["found"]
    assert (match["keyframe"], match["shift"]) == L["best"][:2] and abs(match["distance"] - L["best"][2]) <= DIST_TOL
    assert np.array_equal(bits(match["pose_guess"]), bits(L["guess"]))
    for k in range(TL.N_KF):  # the stored descriptors are the model's
        assert np.array_equal(bits(c.sc_descriptor(k, sp)), bits(L["descs"][k])), k

    (r1, m1), (r2, m2) = (c.perform_loop_closure_sc(TL.STAMP, lp, sp, raw=True) for _ in range(2))
    assert raw_bytes(r1) == raw_bytes(r2) and raw_bytes(m1) == raw_bytes(m2)
    assert m1.as_dict()["distance"] == match["distance"] and m1.keyframe == 0
    d, mi = r1.as_dict(), m["icp"]
    print("device:", d["icp"]["iterations"], d["icp"]["convergence"], d["icp"]["fitness"], d["pose_corrected"])
    print("model: ", mi["iterations"], mi["convergence"], mi["fitness"], m["pose_corrected"])
    assert d["status"] == FBR_LOOP_CLOSED and (d["latest_id"], d["closest_id"]) == (19, 0)
    assert (d["n_source"], d["n_target"]) == (m["n_source"], m["n_target"])
    assert (d["icp"]["iterations"], d["icp"]["convergence"]) == (mi["iterations"], mi["convergence"])
    assert d["icp"]["converged"] == 1
    pc, pm = np.asarray(d["pose_corrected"], np.float64), np.asarray(m["pose_corrected"], np.float64)
    dpos = np.abs(pc[3:] - pm[3:]).max()
    drot = np.abs(np.angle(np.exp(1j * (pc[:3] - pm[:3])))).max()
    print("device - model pose difference: %.3g m, %.3g rad" % (dpos, drot))
    assert dpos <= TL.POSE_TOL and drot <= TL.POSE_TOL
    assert np.array_equal(d["pose_closest"], LM.pose_of(L["poses"][0]))
    T = d["icp"]["transform"].reshape(4, 4)
    assert list(T[3]) == [0.0, 0.0, 0.0, 1.0]
    fit = LM.fitness(LM.xyz(m["source"]), LM.xyz(m["target"]), T)
    assert abs(d["icp"]["fitness"] - fit) <= 1e-5 * fit, (d["icp"]["fitness"], fit)
    btw = LM.between(d["pose_corrected"], d["pose_closest"])
    assert np.abs(d["between"].reshape(4, 4) - btw).max() <= 1e-5
    # against ground truth: twice the model's own error, recorded on the CPU
    dt, dyaw = TL.pose_err(d["pose_corrected"], TL.gt_pose(19))
    print("device pose_corrected from ground truth: %.4g m, %.3g rad" % (dt, dyaw))
    assert dt <= 2.0 * F.MODEL_LOOP_ERR[0] and dyaw <= 2.0 * F.MODEL_LOOP_ERR[1]
    # no key pose has changed
    assert stored_poses(c, L) == before and c.keyframes_count() == TL.N_KF
    assert c.perform_loop_closure(TL.STAMP, lp)["status"] == FBR_LOOP_NO_CANDIDATE

    # a threshold below the best distance: no candidate, and the match still says what was seen
    tight = sc_params(dist_threshold=float(match["distance"]) * 0.99)
    r, mm = c.perform_loop_closure_sc(TL.STAMP, lp, tight, raw=True)
    zero = type(r)()
    zero.status, zero.latest_id, zero.closest_id = FBR_LOOP_NO_CANDIDATE, -1, -1
    assert raw_bytes(r) == raw_bytes(zero) and raw_bytes(mm) == raw_bytes(m1)
    found, mt = c.sc_detect_loop_closure(TL.STAMP, lp, tight)
    assert found is None and mt["keyframe"] == 0
    # nobody old enough: no candidate at all
    found, mt = c.sc_detect_loop_closure(TL.STAMP, loop_params(search_num=3, search_time_diff=100.0), sp)
    assert found is None and mt is None


@pytest.mark.gpu
def test_loop_closure_sc_leaves_the_registration_map_alone():
    L = F.loop_drift()
    R = F.reloc()
    Q = R["queries"][0]
    with api.Context(L["P"]) as c:
        c.set_map(*R["map"])
        add_keyframes(c, L["poses"], L["corners"], L["surfs"])
        c0, s0 = c.get_map()
        p0, st0 = c.register(Q["feat"]["corner"], Q["feat"]["surf"], Q["guess"])
        r, _ = c.perform_loop_closure_sc(TL.STAMP, L["lp"], L["sp"])
        assert r["status"] == FBR_LOOP_CLOSED
        c1, s1 = c.get_map()
        p1, st1 = c.register(Q["feat"]["corner"], Q["feat"]["surf"], Q["guess"])
    assert c0.tobytes() == c1.tobytes() and s0.tobytes() == s1.tobytes()
    assert p0.tobytes() == p1.tobytes() and st0 == st1


@pytest.mark.gpu
def test_sc_loop_calls_without_history(ctx):
    L = F.loop_drift()
    ctx.keyframes_reset()
    assert ctx.sc_detect_loop_closure(0.5, L["lp"]) == (None, None)
    r, m = ctx.perform_loop_closure_sc(0.5, L["lp"])
    assert r["status"] == FBR_LOOP_NO_CANDIDATE and m is None
    add_keyframes(ctx, L["poses"][:1], L["corners"][:1], L["surfs"][:1])
    assert ctx.sc_detect_loop_closure(100.0, L["lp"]) == (None, None)  # only the last keyframe itself
    ctx.keyframes_reset()


# ---- relocalisation --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_relocalize_finds_the_pose_without_a_guess():
    R = F.reloc()
    sp = R["sp"]
    omap = F._oracle_map()
    with api.Context(default_params(16, 1800, exact_voxel_order=1)) as c:
        c.set_map(*R["map"])
        map0 = c.get_map()
        add_keyframes(c, R["poses"], R["corners"], R["surfs"])
        for q in (1, 3):
            Q = R["queries"][q]
            hyps, win = c.relocalize(Q["scan"], k=4, sc=sp)
            assert len(hyps) == 4 and win >= 0
            match, pose, st = hyps[win]
            print("query", q, "winner", win, match["keyframe"], match["shift"], match["distance"], st)
            assert [h[0]["keyframe"] for h in hyps] == [t[0] for t in Q["rank"][:4]]
            assert (match["keyframe"], match["shift"]) == Q["rank"][0][:2] and match["keyframe"] == F.QUERIES[q][0]
            assert st["converged"] == 1 and st["degenerate"] == 0
            assert all(st["n_sel"] >= h[2]["n_sel"] for h in hyps if h[2]["converged"] and not h[2]["degenerate"])
            # the project's parity bound against the oracle registered from the same hypothesis
            po, so, _ = omap.register(Q["feat"]["corner"], Q["feat"]["surf"], match["pose_guess"])
            assert so["converged"] == 1
            dpos = np.abs(pose[3:].astype(np.float64) - po[3:]).max()
            drot = np.abs(np.angle(np.exp(1j * (pose[:3].astype(np.float64) - po[:3])))).max()
            print("   device - oracle: %.3g m, %.3g rad" % (dpos, drot))
            assert dpos <= 1e-4 and drot <= 1e-4
            dt, dr = F.pose_err(pose, Q["gt"])
            print("   from ground truth: %.4g m, %.3g rad" % (dt, dr))
            assert dt <= F.RELOC_BOUND[0] and dr <= F.RELOC_BOUND[1]
            # why the feature is needed: the same scan from the identity guess (the reference's start,
            # imageProjection.cpp:206-218) does not get there, on the oracle
            p0, _ = F.reloc_oracle(q, True)
            dt0, dr0 = F.pose_err(p0, Q["gt"])
            assert dt0 > F.RELOC_BOUND[0] or dr0 > F.RELOC_BOUND[1]
        # the keyframes are only the place database: the registration map is still the prior map
        map1 = c.get_map()
        assert map0[0].tobytes() == map1[0].tobytes() and map0[1].tobytes() == map1[1].tobytes()
        assert c.keyframes_count() == len(R["poses"])


# ---- resources -------------------------------------------------------------------------------------
LIFE_CYCLE = """
import json
import numpy as np
from feature_base_pointcloud_registration_amd import api
from feature_base_pointcloud_registration_amd.fbr_types import KEYPOSE, POINT_XYZI, default_params, loop_params, sc_params

rng = np.random.default_rng(1)
def cloud(n):
    c = np.zeros(n, POINT_XYZI)
    c["x"], c["y"], c["z"] = rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), rng.uniform(-2, 3, n)
    return c

base = api.live_resources()
ctx = api.Context(default_params(16, 1800))
alive = api.live_resources()
for k in range(6):
    pose = np.zeros(1, KEYPOSE)
    pose["time"] = 40.0 * k
    ctx.keyframes_add(pose[0], cloud(500), cloud(3000))
ctx.sc_update()
ctx.sc_query(cloud(400), cloud(2500), 4)
for k in range(2000):  # the store, the records and the pinned block grow
    ctx.keyframes_add(np.zeros(1, KEYPOSE)[0], cloud(3), cloud(0))
ctx.sc_query(cloud(400), cloud(9000), 16)  # a larger query cloud
ctx.sc_update(sc_params(n_ring=32, n_sector=64))
ctx.sc_detect_loop_closure(1e4, loop_params())
ctx.perform_loop_closure_sc(1e4, loop_params(search_num=1), sc_params(dist_threshold=1.0))
used = api.live_resources()
ctx.close()
print(json.dumps(dict(base=base, alive=alive, used=used, closed=api.live_resources())))
"""


@pytest.mark.gpu
def test_place_recognition_releases_what_it_allocates():
    r = subprocess.run([sys.executable, "-c", LIFE_CYCLE], capture_output=True, text=True, timeout=240, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print(out)
    assert out["closed"] == out["base"]
    assert out["used"][0] > out["alive"][0] and out["used"][1] > out["alive"][1]  # device and pinned blocks were taken
    assert out["used"][2:] == out["alive"][2:]  # no stream or event of its own
