"""Place recognition on the CPU: the NumPy model of include/fbr.h's scan-context contract
(tests/sc_model.py), the CPU build of the kernels' arithmetic (tests/native/sc_probe.cpp over
csrc/fbr_sc.h), and the conditions on the fixtures that the GPU tests (tests/test_scan_context.py)
rely on.  No GPU is needed.

Measured here on the CPU (the bounds below are the issue's, not these figures):
  loop fixture, keyframe 19 against 0..4: 0.0424 for keyframe 0, 0.1407 for keyframe 1; the loop
    closure from the hypothesis closes in 7 iterations, 0.0078 m / 8.4e-5 rad from ground truth;
  relocalisation grid: right keyframe 0.096 .. 0.353, runner-up at least 0.128 above it; the oracle
    from the hypothesis within 0.036 m / 0.0024 rad of ground truth (bound 0.05 / 0.01).
"""
import numpy as np
import pytest

import loop_model as LM
import sc_fixtures as F
import sc_model as SM
import test_loop_closure as TL
from feature_base_pointcloud_registration_amd.fbr_types import FBR_LOOP_CLOSED, sc_params

MARGIN = 1e-6  # adjacent distances of a compared ranking differ by at least this, or are equal bit for bit


def away_from_edges(rng, sp, n, margin=1e-3):
    """n random points kept at least `margin` of a bin away from every ring / sector edge."""
    out = np.zeros((0, 3), np.float32)
    while len(out) < n:
        r = rng.uniform(0.0, float(np.float32(sp.max_radius)) * 1.1, 2 * n)
        th = rng.uniform(-np.pi, np.pi, 2 * n)
        p = np.stack([r * np.cos(th), r * np.sin(th), rng.uniform(-3.0, 3.0, 2 * n)], 1).astype(np.float32)
        out = np.concatenate([out, p[SM.edge_margin(p, sp) >= margin]])
    return out[:n]


@pytest.mark.parametrize("shape", [(20, 60), (32, 64), (1, 2), (7, 13)])
def test_probe_bins_equal_the_model(shape):
    sp = sc_params(n_ring=shape[0], n_sector=shape[1])
    p = away_from_edges(np.random.default_rng(1), sp, 10000)
    cm, cp = SM.bins(p, sp), SM.probe_cells(p, sp)
    assert (cm >= 0).sum() > 8000 and (cm < 0).sum() > 300  # points beyond max_radius are dropped
    assert np.array_equal(cm, cp)
    assert np.array_equal(SM.descriptor(p, sp).view(np.uint32), SM.probe_descriptor(p, sp).view(np.uint32))


def test_probe_edge_behaviour_is_the_headers():
    sp = sc_params()
    S = sp.n_sector
    R = np.float32(sp.max_radius)
    below = np.nextafter(R, np.float32(0))
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    pts = np.float32([
        [1.0, 0.0, 0.0],        # theta = 0: sector 0
        [1.0, -0.0, 0.0],       # y = -0, x > 0: atan2 = -0, not below zero: sector 0
        [-1.0, 0.0, 0.0],       # y = +0, x < 0: theta = pi
        [-1.0, -0.0, 0.0],      # y = -0, x < 0: theta = -pi + 2 pi
        [R, 0.0, 0.0],          # r == max_radius: dropped
        [below, 0.0, 0.0],      # the largest float below it: the last ring
        [0.0, 0.0, 1.0],        # the origin: ring 0, atan2(0, 0) = 0: sector 0
        [1.0, -1e-30, 0.0],     # theta + 2 pi rounds to 2 pi: the last sector
        [nan, 1.0, 0.0], [1.0, inf, 0.0], [1.0, 1.0, nan], [1.0, 1.0, -inf], [inf, inf, 0.0],
        [0.0, R, 0.0], [0.0, -below, 0.0],
    ])
    cell = SM.probe_cells(pts, sp)
    last = (sp.n_ring - 1) * S
    assert list(cell[:8]) == [0, 0, S // 2, S // 2, -1, last, 0, S - 1]
    assert list(cell[8:13]) == [-1] * 5
    assert cell[13] == -1 and cell[14] == last + (3 * S) // 4
    # values: z + h <= 0 gives an empty cell; -0 never appears
    d = SM.probe_descriptor(np.float32([[1.0, 1.0, -2.0], [1.0, 1.0, -5.0], [3.0, 40.0, -1.5]]), sp)
    assert np.count_nonzero(d) == 1 and d.max() == 0.5 and not np.signbit(d).any()


@pytest.mark.parametrize("shape", [(20, 60), (5, 8)])
def test_rotation_shifts_the_descriptor(shape):
    sp = sc_params(n_ring=shape[0], n_sector=shape[1])
    rng = np.random.default_rng(2)
    p = away_from_edges(rng, sp, 4000, margin=2e-3).astype(np.float64)
    d0 = SM.descriptor(p.astype(np.float32), sp)
    for j in (0, 1, 7 % sp.n_sector, sp.n_sector - 1):
        a = j * 2.0 * np.pi / sp.n_sector
        q = np.stack([np.cos(a) * p[:, 0] - np.sin(a) * p[:, 1], np.sin(a) * p[:, 0] + np.cos(a) * p[:, 1], p[:, 2]], 1)
        q = q.astype(np.float32)
        assert (SM.edge_margin(q, sp) >= 1e-3).all()
        dj = SM.descriptor(q, sp)
        assert np.array_equal(dj, np.roll(d0, j, axis=1))
        # the rotated scan is the query, the original the candidate: a scan whose yaw grew by
        # j 2 pi / n_sector sees the world turned the other way, and matches at shift j
        dist = SM.distances(SM.descriptor(rotate_scan(p, -a), sp), d0)
        assert dist[j] <= 1e-12 and int(np.argmin(dist)) == j
        assert np.abs(SM.probe_distances(dj, d0) - SM.distances(dj, d0)).max() <= 1e-12


def rotate_scan(p, a):
    return np.stack([np.cos(a) * p[:, 0] - np.sin(a) * p[:, 1], np.sin(a) * p[:, 0] + np.cos(a) * p[:, 1], p[:, 2]],
                    1).astype(np.float32)


def test_probe_distance_equals_the_model():
    for name, case in F.search_cases().items():
        for C in case["cands"]:
            dm, dp = SM.distances(case["query"], C), SM.probe_distances(case["query"], C)
            assert np.abs(dm - dp).max() <= 1e-12, name
            assert int(np.argmin(dm)) == int(np.argmin(dp)), name
    z = np.zeros((20, 60), np.float32)
    assert (SM.distances(F.search_cases()["edges"]["query"], z) == 1.0).all()
    assert (SM.probe_distances(z, z) == 1.0).all()


def check_margin(rank, upto):
    for a, b in zip(rank[:upto], rank[1:upto + 1]):
        assert b[2] - a[2] >= MARGIN or b[2] == a[2], (a, b)


def test_search_cases_are_decidable():
    """The rankings the GPU search tests compare: margins, and the cases are what they claim."""
    cases = F.search_cases()
    for name, case in cases.items():
        r = SM.rank(case["query"], case["cands"])
        check_margin(r, min(max(case["ks"]), len(r)))
        for i, C in enumerate(case["cands"]):  # the synthetic clouds reproduce the descriptors
            assert np.array_equal(SM.probe_descriptor(F.cloud_of(C, case["sp"]), case["sp"]), C), (name, i)
            d = np.sort(SM.distances(case["query"], C))
            assert d[1] - d[0] >= MARGIN or d[1] == d[0], (name, i)  # the shift is decidable too
    r = SM.rank(cases["edges"]["query"], cases["edges"]["cands"])
    assert [t[0] for t in r[:3]] == [0, 1, 2] and [t[1] for t in r[:3]] == [59, 0, 1]
    assert r[0][2] == r[1][2] == r[2][2] and r[0][2] <= 1e-12
    order = [t[0] for t in r]
    assert order.index(5) == order.index(3) + 1 and r[order.index(3)][2] == r[order.index(5)][2]
    print("edges ranking:", [(k, s, round(d, 6)) for k, s, d in r])
    assert r[-1][0] == 6 and r[-1][2] == 1.0
    r = SM.rank(cases["period"]["query"], cases["period"]["cands"])
    assert r[0][:2] == (0, 7) and SM.distances(cases["period"]["query"], cases["period"]["cands"][0])[37] == r[0][2]
    assert [t[0] for t in SM.rank(cases["n3_1x2"]["query"], cases["n3_1x2"]["cands"])] == [0, 1, 2]
    r = SM.rank(cases["n65"]["query"], cases["n65"]["cands"])
    assert len({t[1] for t in r[:16]}) > 8  # many different shifts among the best


def test_pose_guess_turns_the_sensor_about_its_own_z():
    pose = np.float32([0.01, 0.01, 0.4, 3.0, -2.0, 1.8])
    assert np.array_equal(SM.pose_guess(pose, 0, 60), pose) or np.abs(SM.pose_guess(pose, 0, 60) - pose).max() < 1e-6
    g = SM.pose_guess(pose, 15, 60).astype(np.float64)
    A = LM.pose3(pose) @ LM.pose3([0, 0, np.pi / 2, 0, 0, 0])
    assert np.abs(LM.pose3(g) - A).max() < 1e-6
    assert np.array_equal(g[3:], pose[3:].astype(np.float64))


# ---- fixture conditions: they guard the GPU tests ---------------------------------------------------
def test_loop_fixture_is_found_by_appearance():
    L = F.loop_drift()
    assert LM.detect(L["poses"], TL.STAMP, L["lp"]) is None  # the radius search has lost the loop
    assert L["found"] == (19, 0) and L["best"][:2] == (0, 0)
    r = SM.rank(L["descs"][19], L["descs"][:5])
    print("loop fixture distances:", [(k, s, round(d, 4)) for k, s, d in r])
    assert r[0][0] == 0 and r[1][2] - r[0][2] >= 0.05
    assert r[0][2] < L["sp"].dist_threshold
    check_margin(r, len(r) - 1)
    # only keyframes 0..4 are older than search_time_diff
    assert [i for i in range(19) if abs(L["poses"]["time"][i] - TL.STAMP) > L["lp"].search_time_diff] == [0, 1, 2, 3, 4]
    # float64 bins give the same descriptors on this fixture (no point within rounding of an edge)
    assert all(np.array_equal(a, b) for a, b in zip(F.descriptors(L["corners"], L["surfs"], L["sp"], exact=False),
                                                    L["descs"]))


def test_loop_fixture_closes_from_the_hypothesis():
    L = F.loop_drift()
    m = L["model"]
    assert m["status"] == FBR_LOOP_CLOSED and (m["latest_id"], m["closest_id"]) == (19, 0)
    assert m["icp"]["converged"] == 1 and 3 <= m["icp"]["iterations"] <= 30
    for tests in m["icp"]["log"]:  # no convergence test decided within 10 % of its threshold
        for value, thr in tests:
            assert not 0.9 * thr <= value <= 1.1 * thr, (value, thr)
    dt, dyaw = TL.pose_err(m["pose_corrected"], TL.gt_pose(19))
    print("model loop closure from the hypothesis: %d iterations, %.4g m, %.3g rad" % (m["icp"]["iterations"], dt, dyaw))
    # the figures the GPU test doubles for its bound
    assert dt <= F.MODEL_LOOP_ERR[0] * 1.01 and dyaw <= F.MODEL_LOOP_ERR[1] * 1.01


def test_relocalisation_fixture():
    R = F.reloc()
    for q, Q in enumerate(R["queries"]):
        r = Q["rank"]
        print("query", q, "rank", [(k, s, round(d, 4)) for k, s, d in r[:3]])
        assert r[0][0] == F.QUERIES[q][0] and r[1][2] - r[0][2] >= 0.05
        check_margin(r, 4)
        # the shift gives the yaw turn to within a sector and a bit
        dyaw = np.angle(np.exp(1j * (Q["guess"][2] - Q["gt"][2])))
        assert abs(dyaw) <= 1.2 * 2.0 * np.pi / R["sp"].n_sector
        pose, st = F.reloc_oracle(q)
        dt, dr = F.pose_err(pose, Q["gt"])
        print("   oracle from the hypothesis: %d iterations, %.4g m, %.3g rad" % (st["iterations"], dt, dr))
        assert st["converged"] == 1 and st["degenerate"] == 0
        assert dt <= F.RELOC_BOUND[0] and dr <= F.RELOC_BOUND[1]
        # today: the same scan from the identity guess does not get there
        p0, st0 = F.reloc_oracle(q, True)
        dt0, dr0 = F.pose_err(p0, Q["gt"])
        assert dt0 > 1.0
