"""tests/kf_model.py (the keyframe selection and concatenation restated in NumPy from
mapOptmization.h:857-955) pinned to the oracle's extractSurroundingKeyFrames, on every input of
tests/kf_cases.py that tests/test_keyframe_map.py gives the device; and every case held to the shape it
is meant to have (the boundary pose missed by the search, kept by the gate; the merged record's
truncated mean index; the segment sizes; the mapping loop's concatenated surf totals on both sides of
the 32768-point switch of the device VoxelGrid), so that none degenerates unnoticed.
"""
import numpy as np
import pytest

import kf_cases as C
import kf_model as M
import pyoracle as O
from feature_base_pointcloud_registration_amd.fbr_types import POINT_XYZI, keyframe_params


def same_bytes(a, b):
    return len(a) == len(b) and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def check_against_oracle(poses, corners, surfs, kp, stamp):
    P = C.params()
    oc, os_, onf = O.kf_extract(P, poses, corners, surfs, kp, stamp)
    mc, ms, nf, entries, n_cc, n_cs = M.local_map(poses, corners, surfs, kp, stamp, P)
    assert nf == onf
    assert same_bytes(mc, oc) and same_bytes(ms, os_)
    return entries, n_cc, n_cs, (oc, os_, onf)


@pytest.mark.parametrize("case", C.selection_cases(), ids=lambda c: c["name"])
def test_model_matches_oracle_and_case_has_its_shape(case):
    poses, kp = case["poses"], C.kparams(case)
    entries, n_cc, n_cs, (oc, os_, onf) = check_against_oracle(poses, case["corners"], case["surfs"], kp, case["stamp"])
    sh = case["shape"]
    assert onf == sh["n_frames"]
    assert [e.key for e in entries] == sh["keys"]
    assert [i for i, e in enumerate(entries) if e.dropped] == sh["dropped"]
    if "hits" in sh:
        assert list(M.radius_hits(poses, kp.search_radius)[0]) == sh["hits"]
    if "sources" in sh:
        assert [e.source for e in entries] == sh["sources"]
    for k in sh.get("absent", []):
        assert k not in [e.key for e in entries]
    if sh.get("large"):
        assert n_cs >= C.VG_LARGE_MIN > n_cc > 0  # the surf filter is voxel_grid_large, the corner one is not
    if "corner_points" in sh:
        assert n_cc == sh["corner_points"] == len(oc) and n_cs > 0
    # the map's input size names the selected keys: the clouds' sizes are distinct sums
    kept = [e.key for e in entries if not e.dropped]
    assert n_cc == sum(len(case["corners"][k]) for k in kept) and n_cs == sum(len(case["surfs"][k]) for k in kept)


def _case(name):
    return next(c for c in C.selection_cases() if c["name"] == name)


def test_boundary_pose_is_missed_by_the_search_and_kept_by_the_gate():
    c = _case("boundary_long_window")
    poses, kp = c["poses"], C.kparams(c)
    back = poses[-1]
    assert M.gate_distance(np.array([poses["x"][0], poses["y"][0], poses["z"][0]], np.float32), back) == np.float32(kp.search_radius)
    assert 0 not in M.radius_hits(poses, kp.search_radius)[0]
    e0 = [e for e in M.select(poses, kp, c["stamp"]) if e.key == 0]
    assert len(e0) == 1 and e0[0].source == "recent" and not e0[0].dropped
    # with the short window the same pose is not selected at all, and key 2 is extracted twice
    s = _case("boundary_short_window")
    es = M.select(s["poses"], C.kparams(s), s["stamp"])
    assert [(e.key, e.source, e.dropped) for e in es] == [(2, "ds", False), (2, "recent", False)]
    # the window-stop case reuses the geometry: its key 1 is on the radius and would be kept if reached
    w = _case("window_stop")
    wp = w["poses"]
    assert M.gate_distance(np.array([wp["x"][1], wp["y"][1], wp["z"][1]], np.float32), wp[-1]) == np.float32(5.0)
    assert wp["time"][1] > wp["time"][2] and w["stamp"] - wp["time"][1] < 3.0 <= w["stamp"] - wp["time"][2]


def test_merged_record_carries_the_truncated_mean_index_and_the_centroid():
    c = _case("merged_poses")
    poses, kp = c["poses"], C.kparams(c)
    idx, _ = M.radius_hits(poses, kp.search_radius)
    sur = np.zeros(len(idx), POINT_XYZI)
    for k in ("x", "y", "z", "intensity"):
        sur[k] = poses[k][idx]
    ds = O.voxel_grid(sur, kp.pose_density)
    assert len(ds) == 2 and ds["intensity"][0] == np.float32(1.5) and ds["intensity"][1] == np.float32(4.0)
    e = M.select(poses, kp, c["stamp"])[0]
    assert e.key == 1 and e.source == "ds"
    assert np.allclose(e.pos, [poses[k][:4].mean() for k in "xyz"], atol=1e-6)
    assert not any(np.array_equal(e.pos, [poses["x"][k], poses["y"][k], poses["z"][k]]) for k in range(4))
    # the cloud sizes name key 1, under key 1's own pose
    cs = M.concat([e], poses, c["surfs"])
    assert len(cs) == 61 and same_bytes(cs, M.concat([M.Entry(1, None, "ds", False)], poses, c["surfs"]))


def test_segment_sizes_cover_the_launch_shape():
    c = _case("segment_sizes")
    nc, ns = [len(x) for x in c["corners"]], [len(x) for x in c["surfs"]]
    assert set(ns) == set(C.SEG_SIZES) and set(nc) == set(C.SEG_SIZES) - {16384, 40000}
    assert max(nc) < max(ns) and max(nc) > 64 * 256  # the shared max_cnt is the surf side's; both loop
    both = [k for k in range(len(nc)) if nc[k] == 0 and ns[k] == 0]
    corner_only = [k for k in range(len(nc)) if nc[k] == 0 and ns[k] > 0]
    assert len(both) == 1 and len(corner_only) >= 2


def test_many_segments_model_matches_oracle():
    c = C.many_segments_case()
    entries, n_cc, n_cs, _ = check_against_oracle(c["poses"], c["corners"], c["surfs"], C.kparams(c), c["stamp"])
    assert len(entries) == C.N_MANY > 65535 and not any(e.dropped for e in entries)
    assert n_cc == n_cs == C.N_MANY and [e.key for e in entries[:2]] == [C.N_MANY - 1, C.N_MANY - 2]


def test_mapping_loop_model_matches_oracle_and_crosses_the_large_filter_switch():
    L = C.loop_inputs()
    kp = keyframe_params(**L["kp"])
    P = C.params()
    totals, frames, converged = [], [], 0
    for s in L["steps"]:
        k = s["k"]
        entries, _, n_cs, (oc, os_, onf) = check_against_oracle(L["poses"][:k + 1], L["corners"][:k + 1], L["surfs"][:k + 1], kp,
                                                                 s["stamp"])
        totals.append(n_cs)
        frames.append(onf)
        assert 5900 <= len(os_) <= 9900
        _, st, _ = O.Map(P, oc, os_, raw=True).register(s["corner"], s["surf"], s["guess"])
        converged += int(st["status"] == 0 and st["converged"] == 1)
        assert (st["n_corner_map"], st["n_surf_map"]) == (len(oc), len(os_))
    assert min(frames) == 4 and max(frames) == 8
    assert converged >= 13  # 14 here: step 12 runs to the iteration cap; the device tests may leave out 2 at most
    below = [t < C.VG_LARGE_MIN for t in totals]
    ups = sum(1 for a, b in zip(below, below[1:]) if a and not b)
    downs = sum(1 for a, b in zip(below, below[1:]) if not a and b)
    assert ups >= 1 and downs >= 1, totals  # the rebuilds switch filter in each direction
    # the corrected poses and the shrunken map of the loop's end
    n = len(L["poses"])
    stamp = L["steps"][-1]["stamp"]
    check_against_oracle(L["moved"], L["corners"], L["surfs"], kp, stamp)
    e, _, n_cs, (_, os_, _) = check_against_oracle(L["poses"], L["corners"], L["surfs"], keyframe_params(**L["shrunk_kp"]), stamp)
    assert {x.key for x in e if not x.dropped} == {n - 1} and n_cs < totals[-1] and len(os_) < 5900
