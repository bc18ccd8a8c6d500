"""The keyframe local map (fbr_extract_surrounding_keyframes: the host's key-pose selection,
k_kf_transform, the two device VoxelGrids and the rebuild of the kNN grids) across rebuilds in one
context, at the selection's edges, at the launch shapes of k_kf_transform, and under every
registration path, against the CPU oracle's extractSurroundingKeyFrames (tests/kf_cases.py has the
inputs; tests/test_kf_model.py pins them and their shapes to a NumPy model on the CPU).

Bars:
  * exact_voxel_order = 1 (the device VoxelGrid is bit-identical to the oracle's there):
    (n_corner, n_surf, n_frames) equal and get_map() byte-equal to the oracle's maps;
  * the default voxel order: tests/test_keyframes.py's bars (equal sizes, same order, |d xyz| <= 2e-4);
  * registered poses within 1e-4 m / 1e-4 rad of the oracle's with equal iteration counts, on every
    step the oracle marks converged (kf_cases: 14 of the loop's 15).

The tile kNN is chosen by environment knobs read once per process, so the mapping loop also runs in
two child processes (this file run as a script), whose poses, statistics and maps must be the same
bytes.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import kf_cases as C  # noqa: E402
from feature_base_pointcloud_registration_amd.fbr_types import REG_STATS_FIELDS, keyframe_params, score_params  # noqa: E402

FBR_ERR_INVALID_ARG = -1
POSE_TOL = 1e-4
TILE_ENV = {"FBR_KNN_TILE": "1", "FBR_KNN_CELL": "0.5", "FBR_KNN_CELL_X": "0.125"}
KNOBS = ("FBR_KNN_LPQ", "FBR_KNN_FLAT", "FBR_KNN_CELL", "FBR_KNN_CELL_X", "FBR_GRID_SPARSE", "FBR_GN_TAIL", "FBR_KNN_TILE",
         "FBR_KNN_TILE_STATS", "FBR_GN_LAG", "FBR_FIT_CACHE")


def add_keyframes(ctx, poses, corners, surfs, lo, hi):
    for k in range(lo, hi):
        ctx.keyframes_add(poses[k], corners[k], surfs[k])


def run_loop(ctx, L, tiles=None):
    """The mapping loop in one context: per step add keyframe k, extract, read the map back and
    register the next scan.  Returns one dict per step."""
    kp = keyframe_params(**L["kp"])
    add_keyframes(ctx, L["poses"], L["corners"], L["surfs"], 0, 1)
    out = []
    for s in L["steps"]:
        k = s["k"]
        add_keyframes(ctx, L["poses"], L["corners"], L["surfs"], k, k + 1)
        sizes = ctx.extract_surrounding_keyframes(s["stamp"], kp)
        mc, ms = ctx.get_map()
        pose, st = ctx.register(s["corner"], s["surf"], s["guess"])
        if tiles is not None:
            tiles.append(ctx.diag_knn_last()["desc"]["tiles"])
        out.append(dict(k=k, sizes=sizes, map_c=mc, map_s=ms, pose=pose, stats=st))
    return out


# ------------------------------------------------------------------------------------ the child
def child(out_path):
    from feature_base_pointcloud_registration_amd import api
    L = C.loop_inputs()
    tiles = []
    with api.Context(C.params(0)) as ctx:
        steps = run_loop(ctx, L, tiles)
    out = {"tiles": np.array(tiles, np.int32),
           "poses": np.stack([s["pose"] for s in steps]),
           "stats": np.array([[s["stats"][f] for f in REG_STATS_FIELDS] for s in steps], np.int32),
           "sizes": np.array([s["sizes"] for s in steps], np.int64)}
    for s in steps:
        out["map_c/%d" % s["k"]], out["map_s/%d" % s["k"]] = s["map_c"], s["map_s"]
    np.savez(out_path, **out)


if __name__ == "__main__":
    child(sys.argv[1])
    sys.exit(0)


# ------------------------------------------------------------------------------------ the parent
import pyoracle as O  # noqa: E402
import score_model as S  # noqa: E402
from feature_base_pointcloud_registration_amd import api  # noqa: E402
from test_keyframes import _close_maps, _pose_close  # noqa: E402

pytestmark = pytest.mark.gpu

_ORACLE = {}


def oracle_map(name, P, poses, corners, surfs, kp, stamp):
    """O.kf_extract, computed once per input: both voxel orders share the reference."""
    if name not in _ORACLE:
        _ORACLE[name] = O.kf_extract(P, poses, corners, surfs, kp, stamp)
    return _ORACLE[name]


def same_bytes(a, b):
    return len(a) == len(b) and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def check_map(ctx, sizes, ref, exact, where):
    oc, os_, onf = ref
    assert tuple(sizes) == (len(oc), len(os_), onf), (where, sizes, (len(oc), len(os_), onf))
    gc, gs = ctx.get_map()
    if exact:
        assert same_bytes(gc, oc), (where, "corner")
        assert same_bytes(gs, os_), (where, "surf")
    else:
        _close_maps(gc, oc)
        _close_maps(gs, os_)
    return gc, gs


def extract_case(case, exact):
    P = C.params(exact)
    kp = C.kparams(case)
    ref = oracle_map(case["name"], P, case["poses"], case["corners"], case["surfs"], kp, case["stamp"])
    with api.Context(P) as ctx:
        t0 = time.perf_counter()
        add_keyframes(ctx, case["poses"], case["corners"], case["surfs"], 0, len(case["poses"]))
        t_add = time.perf_counter() - t0
        t0 = time.perf_counter()
        sizes = ctx.extract_surrounding_keyframes(case["stamp"], kp)
        t_ext = time.perf_counter() - t0
        check_map(ctx, sizes, ref, exact, case["name"])
    return ref, t_add, t_ext


# ------------------------------------------------------------------------------------ §2 selection, launch shapes
@pytest.mark.parametrize("exact", [1, 0], ids=["exact", "default"])
@pytest.mark.parametrize("case", C.selection_cases(), ids=lambda c: c["name"])
def test_selection_and_segment_cases_match_the_oracle(case, exact):
    """Each case of kf_cases.selection_cases in a fresh context: the radius' strictness in the search
    and not in the gate, radius 0, merged poses' truncated mean index, the window's stop, loop mode's
    submap_size + 1, and k_kf_transform's segments of 0 to 40000 points (its grid-stride loop from
    16385 on, the shared max_cnt, an empty corner launch beside a surf one)."""
    (oc, os_, onf), _, _ = extract_case(case, exact)
    assert onf == case["shape"]["n_frames"]
    if case["name"] == "segment_sizes_no_corner":
        assert len(oc) == 0 and len(os_) > 0


@pytest.mark.parametrize("exact", [1, 0], ids=["exact", "default"])
def test_more_than_65535_segments_reach_the_second_launch_chunk(exact):
    """65537 selected keyframes of one corner and one surf point: launch_kf_transform's second
    blockIdx.y chunk, and a keyframe pool regrown many times.  The device side is bound by the 65537
    keyframes_add calls: measured with an MI355X, 1.4 s for the adds and 0.017 s (exact order) / 0.014 s
    (default order) for the extraction; the whole test 1.8 s / 1.5 s, the oracle's extraction 1.5 s of it
    once."""
    case = C.many_segments_case()
    (oc, os_, onf), t_add, t_ext = extract_case(case, exact)
    print("many_segments exact=%d: keyframes_add %.2f s, extract %.3f s" % (exact, t_add, t_ext))
    assert onf == C.N_MANY and len(oc) > 0 and len(os_) > 0


def test_rejected_arguments_leave_the_map_as_it_is():
    case = next(c for c in C.selection_cases() if c["name"] == "loop_submap_4")
    with api.Context(C.params(0)) as ctx:
        add_keyframes(ctx, case["poses"], case["corners"], case["surfs"], 0, len(case["poses"]))
        sizes = ctx.extract_surrounding_keyframes(case["stamp"], C.kparams(case))
        mc, ms = ctx.get_map()
        for bad in (dict(search_radius=-1.0), dict(search_radius=float("nan")), dict(pose_density=0.0),
                    dict(pose_density=-2.0), dict(pose_density=float("nan")), dict(search_radius=-0.5, loop_closure=1)):
            with pytest.raises(api.FbrError) as e:
                ctx.extract_surrounding_keyframes(case["stamp"], keyframe_params(**bad))
            assert e.value.status == FBR_ERR_INVALID_ARG, bad
            gc, gs = ctx.get_map()
            assert same_bytes(gc, mc) and same_bytes(gs, ms), bad
            info = ctx.map_grid_info()
            assert (info["n_corner"], info["n_surf"]) == sizes[:2], bad
        assert ctx.keyframes_count() == len(case["poses"])
        assert ctx.extract_surrounding_keyframes(case["stamp"], C.kparams(case)) == sizes


# ------------------------------------------------------------------------------------ §3 the mapping loop
@pytest.fixture(scope="module")
def loop_ref():
    """The oracle's map, n_frames and registration of every step, computed once."""
    L = C.loop_inputs()
    P = C.params(0)
    kp = keyframe_params(**L["kp"])
    steps = []
    for s in L["steps"]:
        k = s["k"]
        oc, os_, onf = O.kf_extract(P, L["poses"][:k + 1], L["corners"][:k + 1], L["surfs"][:k + 1], kp, s["stamp"])
        pose, st, _ = O.Map(P, oc, os_, raw=True).register(s["corner"], s["surf"], s["guess"])
        steps.append(dict(k=k, ref=(oc, os_, onf), pose=pose, stats=st))
    stamp = L["steps"][-1]["stamp"]
    moved = O.kf_extract(P, L["moved"], L["corners"], L["surfs"], kp, stamp)
    shrunk = O.kf_extract(P, L["moved"], L["corners"], L["surfs"], keyframe_params(**L["shrunk_kp"]), stamp)
    assert sum(1 for s in steps if s["stats"]["converged"]) >= 13  # the issue's cap: at most 2 steps left out
    return dict(L=L, steps=steps, moved=moved, shrunk=shrunk)


@pytest.mark.parametrize("exact", [1, 0], ids=["exact", "default"])
def test_mapping_loop_in_one_context(loop_ref, exact):
    """Fifteen rebuilds in one context (d_kraw grown and never shrunk, d_kf_segs reused, d_kds and the
    grids rebuilt, the keyframe pool regrown between extractions, the surf VoxelGrid switching between
    the one-workgroup filter and voxel_grid_large in both directions), each registered from; then the
    corrected poses, a map shrunk to one frame after the largest, and every step again in a fresh
    context."""
    L = loop_ref["L"]
    P = C.params(exact)
    with api.Context(P) as ctx:
        steps = run_loop(ctx, L)
        for g, r in zip(steps, loop_ref["steps"]):
            where = ("step", g["k"])
            oc, os_, onf = r["ref"]
            assert g["sizes"] == (len(oc), len(os_), onf), where
            if exact:
                assert same_bytes(g["map_c"], oc) and same_bytes(g["map_s"], os_), where
            else:
                _close_maps(g["map_c"], oc)
                _close_maps(g["map_s"], os_)
            so, sg = r["stats"], g["stats"]
            assert (sg["n_corner_map"], sg["n_surf_map"]) == (so["n_corner_map"], so["n_surf_map"]) == (len(oc), len(os_)), where
            assert (sg["n_corner_ds"], sg["n_surf_ds"]) == (so["n_corner_ds"], so["n_surf_ds"]), where
            if so["converged"]:
                assert sg["status"] == so["status"] == 0 and sg["converged"] == 1, where
                assert sg["iterations"] == so["iterations"], (where, sg, so)
                _pose_close(g["pose"], r["pose"])
                if exact:
                    assert sg["n_sel"] == so["n_sel"], (where, sg, so)
        # correctPoses: every key pose moves, the clouds stay
        for k in range(len(L["poses"])):
            ctx.keyframes_set_pose(k, L["moved"][k])
        stamp = L["steps"][-1]["stamp"]
        sizes = ctx.extract_surrounding_keyframes(stamp, keyframe_params(**L["kp"]))
        check_map(ctx, sizes, loop_ref["moved"], exact, "moved")
        # radius 1: one frame's map after the largest; a stale tail of d_kraw or of the grids would show
        sizes = ctx.extract_surrounding_keyframes(stamp, keyframe_params(**L["shrunk_kp"]))
        shrunk = check_map(ctx, sizes, loop_ref["shrunk"], exact, "shrunk")
        assert sizes[1] < min(len(s["map_s"]) for s in steps)
        info = ctx.map_grid_info()
        assert (info["n_corner"], info["n_surf"]) == sizes[:2]
        last = L["steps"][-1]
        pose, st = ctx.register(last["corner"], last["surf"], last["guess"])
        po, so, _ = O.Map(P, *loop_ref["shrunk"][:2], raw=True).register(last["corner"], last["surf"], last["guess"])
        assert (st["n_corner_map"], st["n_surf_map"]) == (so["n_corner_map"], so["n_surf_map"]) == sizes[:2]
        if so["converged"]:
            assert st["converged"] == 1 and st["iterations"] == so["iterations"]
            _pose_close(pose, po)
    # a fresh context given the same keyframes makes the same bytes, at every step and at the end
    kp = keyframe_params(**L["kp"])
    for g in steps:
        k = g["k"]
        with api.Context(P) as ctx:
            add_keyframes(ctx, L["poses"], L["corners"], L["surfs"], 0, k + 1)
            assert ctx.extract_surrounding_keyframes(L["steps"][k - 1]["stamp"], kp) == g["sizes"]
            fc, fs = ctx.get_map()
            assert same_bytes(fc, g["map_c"]) and same_bytes(fs, g["map_s"]), ("fresh", k)
            if k == len(L["poses"]) - 1:
                for j in range(len(L["poses"])):
                    ctx.keyframes_set_pose(j, L["moved"][j])
                ctx.extract_surrounding_keyframes(stamp, keyframe_params(**L["shrunk_kp"]))
                fc, fs = ctx.get_map()
                assert same_bytes(fc, shrunk[0]) and same_bytes(fs, shrunk[1]), "fresh shrunk"


def test_mapping_loop_tile_knn_gives_the_default_bytes(tmp_path):
    """The block-tile kNN on rebuilt maps (d_bin / bin_nb rebuilt per map, d_fb_list kept): the loop in
    a child process with the tile knobs against a child with the defaults."""
    res = {}
    for name, env_set in (("default", {}), ("tiles", TILE_ENV)):
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update(env_set)
        out = str(tmp_path / (name + ".npz"))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True,
                           timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
        res[name] = np.load(out)
    d, t = res["default"], res["tiles"]
    assert not d["tiles"].any() and t["tiles"].all(), (d["tiles"], t["tiles"])  # the variant meant ran
    assert d["poses"].tobytes() == t["poses"].tobytes()
    assert d["stats"].tobytes() == t["stats"].tobytes() and (d["stats"][:, 0] == 0).all()
    assert d["sizes"].tobytes() == t["sizes"].tobytes()
    for k in range(1, C.LOOP_N):
        for m in ("map_c/%d", "map_s/%d"):
            assert d[m % k].tobytes() == t[m % k].tobytes(), (m, k)


# ------------------------------------------------------------------------------------ §4 the other registration paths
PATH_STEP = 9
PATH_SCANS = (7, 8, 9, 10, 11)  # the loop's steps whose next scans are registered on step 9's map


@pytest.fixture(scope="module")
def paths():
    """Step 9's map in a context of max_batch = 3, five scans near it, and the oracle's process_scan
    of each on the oracle's map."""
    L = C.loop_inputs()
    P = C.params(0)
    P.max_batch = 3
    k = PATH_STEP
    kp = keyframe_params(**L["kp"])
    stamp = L["steps"][k - 1]["stamp"]
    assert L["steps"][k - 1]["k"] == k
    ref = O.kf_extract(C.params(0), L["poses"][:k + 1], L["corners"][:k + 1], L["surfs"][:k + 1], kp, stamp)
    jobs = [L["steps"][j - 1] for j in PATH_SCANS]
    omap = O.Map(P, ref[0], ref[1], raw=True)
    oracle = [O.Stream(P).process_scan(omap, j["scan"], 0.0, j["guess"]) for j in jobs]
    assert all(st["status"] == 0 and st["converged"] for _, st in oracle)
    with api.Context(P) as ctx:
        add_keyframes(ctx, L["poses"], L["corners"], L["surfs"], 0, k + 1)
        sizes = ctx.extract_surrounding_keyframes(stamp, kp)
        check_map(ctx, sizes, ref, 0, "paths")
        yield dict(ctx=ctx, L=L, P=P, kp=kp, stamp=stamp, ref=ref, sizes=sizes, jobs=jobs, oracle=oracle,
                   scans=[j["scan"] for j in jobs], guesses=np.stack([j["guess"] for j in jobs]))


def check_job(pose, st, oracle, sizes, where):
    po, so = oracle
    for f in ("status", "n_points", "n_corner", "n_surf", "iterations"):
        assert int(st[f]) == so[f], (where, f, int(st[f]), so[f])
    assert (int(st["n_corner_map"]), int(st["n_surf_map"])) == tuple(sizes[:2]), where
    assert (so["n_corner_map"], so["n_surf_map"]) == tuple(sizes[:2]), where
    _pose_close(pose, po)


def test_process_scan_on_a_keyframe_map(paths):
    ctx = paths["ctx"]
    ctx.reset_stream()
    for i, (scan, guess) in enumerate(zip(paths["scans"], paths["guesses"])):
        ctx.reset_stream()  # every scan as the first of its stream, as the oracle's fresh Stream takes it
        pose, st = ctx.process_scan(scan, 0.0, guess)
        check_job(pose, st, paths["oracle"][i], paths["sizes"], ("process_scan", i))


def test_process_batch_on_a_keyframe_map(paths):
    """Five jobs at max_batch = 3: two device batches through ingest_stage's crop_stats."""
    poses, stats = paths["ctx"].process_batch(paths["scans"], paths["guesses"])
    for i in range(len(poses)):
        check_job(poses[i], stats[i], paths["oracle"][i], paths["sizes"], ("process_batch", i))


def staged(ctx, scans, guesses):
    ctx.batch_stage(scans, guesses)
    ctx.batch_launch()
    ctx.batch_wait()
    return ctx.batch_results()


def test_staged_batches_on_a_keyframe_map(paths):
    """fbr_batch_stage's crop_stats and crop_cached: every job carries the whole map's sizes."""
    ctx = paths["ctx"]
    for lo, hi in ((0, 3), (3, 5)):
        poses, stats = staged(ctx, paths["scans"][lo:hi], paths["guesses"][lo:hi])
        for i in range(hi - lo):
            check_job(poses[i], stats[i], paths["oracle"][lo + i], paths["sizes"], ("staged", lo + i))


def test_extract_between_stage_and_launch(paths):
    """A batch staged on map A and launched after the extraction of map B registers on B, with B's
    sizes: the same bytes as staging after the extraction."""
    ctx, L = paths["ctx"], paths["L"]
    scans, guesses = paths["scans"][:3], paths["guesses"][:3]
    kp_b = keyframe_params(**dict(L["kp"], search_radius=4.0))
    try:
        pa, sa = staged(ctx, scans, guesses)
        ctx.batch_stage(scans, guesses)  # staged on A
        sizes_b = ctx.extract_surrounding_keyframes(paths["stamp"], kp_b)
        assert sizes_b[1] < paths["sizes"][1]
        ctx.batch_launch()
        ctx.batch_wait()
        p1, s1 = ctx.batch_results()
        p2, s2 = staged(ctx, scans, guesses)  # staged on B
        assert p1.tobytes() == p2.tobytes() and s1.tobytes() == s2.tobytes()
        assert (s1["n_corner_map"] == sizes_b[0]).all() and (s1["n_surf_map"] == sizes_b[1]).all()
        assert s1.tobytes() != sa.tobytes()
    finally:
        assert ctx.extract_surrounding_keyframes(paths["stamp"], paths["kp"]) == paths["sizes"]
    pa2, sa2 = staged(ctx, scans, guesses)
    assert pa2.tobytes() == pa.tobytes() and sa2.tobytes() == sa.tobytes()


def test_score_poses_ignores_the_crop_on_a_keyframe_map(paths):
    """fbr_score_poses' use_crop && !map_nocrop: on a keyframe map the whole map is searched either
    way, and the records are the model's (tests/test_pose_score.py's bar)."""
    from test_pose_score import assert_record
    ctx, P = paths["ctx"], paths["P"]
    job = paths["jobs"][2]
    corner = O.voxel_grid(job["corner"], P.mapping_corner_leaf_size)
    surf = O.voxel_grid(job["surf"], P.mapping_surf_leaf_size)
    far = job["gt"].copy()
    far[3] += 40.0  # the registration's box around this pose holds no map point: the crop would leave no inlier
    poses = np.stack([job["gt"], job["guess"], far])
    r1, k1 = ctx.score_poses(corner, surf, poses, score_params(use_crop=1), keys=True)
    r0, k0 = ctx.score_poses(corner, surf, poses, score_params(use_crop=0), keys=True)
    assert r1.tobytes() == r0.tobytes() and k1.tobytes() == k0.tobytes()
    mc, ms = ctx.get_map()
    xyz = lambda c: np.stack([c["x"], c["y"], c["z"]], 1)  # noqa: E731
    for i, pose in enumerate(poses):
        want, wkeys = S.score(xyz(mc), xyz(ms), xyz(corner), xyz(surf), S.affine32(pose), list(P.crop_half), 1.0, False)
        assert_record(r1[i], want, k1[i], wkeys, i)
        if i == 0:  # the box would have mattered: the model loses inliers to it at this pose
            cropped, _ = S.score(xyz(mc), xyz(ms), xyz(corner), xyz(surf), S.affine32(pose), list(P.crop_half), 1.0, True)
            assert cropped["n_in"].sum() < want["n_in"].sum()
    assert r1["n_in"][0].sum() > 0.5 * r1["n"][0].sum() and r1["fitness"][0] < r1["fitness"][1]


def test_map_switch_restores_both_maps(paths):
    """fbr_set_map after a keyframe map, then the extraction again: each map's earlier results byte
    for byte (map, registration, a staged batch)."""
    from feature_base_pointcloud_registration_amd import synth
    ctx = paths["ctx"]
    job = paths["jobs"][2]
    scans, guesses = paths["scans"][:3], paths["guesses"][:3]
    cmap, smap = synth.config_map("C1")
    gt, guess = synth.job(1)
    f = O.Stream(paths["P"]).features(synth.scan(gt, 16, 1800, seed=1))

    def on_keyframe_map():
        assert ctx.extract_surrounding_keyframes(paths["stamp"], paths["kp"]) == paths["sizes"]
        mc, ms = ctx.get_map()
        pose, st = ctx.register(job["corner"], job["surf"], job["guess"])
        pb, sb = staged(ctx, scans, guesses)
        return mc.tobytes(), ms.tobytes(), pose.tobytes(), sorted(st.items()), pb.tobytes(), sb.tobytes()

    def on_prior_map():
        ctx.set_map(cmap, smap)
        mc, ms = ctx.get_map()
        pose, st = ctx.register(f["corner"], f["surf"], guess)
        return mc.tobytes(), ms.tobytes(), pose.tobytes(), sorted(st.items())

    try:
        a0 = on_keyframe_map()
        b0 = on_prior_map()
        assert dict(b0[3])["n_surf_map"] not in (0, paths["sizes"][1])  # the CropBox counts, not the keyframe map's
        a1 = on_keyframe_map()
        b1 = on_prior_map()
        assert a0 == a1 and b0 == b1
    finally:
        ctx.extract_surrounding_keyframes(paths["stamp"], paths["kp"])
