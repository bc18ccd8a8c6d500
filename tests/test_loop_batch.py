"""Loop closure for many keyframe pairs: fbr_loop_candidates, fbr_perform_loop_closures and
fbr_icp_align_batch.  The reference for every equality is the single-pair call
(fbr_perform_loop_closure on a store holding keyframes 0..i, fbr_icp_align,
fbr_perform_loop_closure_sc), which this file does not re-test (tests/test_loop_closure.py does).

The fixture is test_loop_closure.fixture()'s out-and-back run of 20 keyframes with keyframe 19's
drift removed, search_num = 2, search_time_diff = 10, and the offsets of OFFSETS added to the stored
poses.  tests/loop_model.py on prefix stores gives 14 pairs, (6,0) .. (19,0), keyframes 1-5 none;
model iteration counts 10, 18, 22, 10, 12, 7, 7, 5, 8, 4, 10, 2, 12, 7; pairs 6-10 end
FBR_LOOP_REJECTED_FITNESS (fitness 0.32-0.43) and pairs 11-19 FBR_LOOP_CLOSED (0.013-0.033);
n_source 590 .. 3,398 (3 to 14 query blocks, none a multiple of 256), n_target 4,001 .. 5,146.  The
pairs stop at nine different iteration counts and in two statuses: the batch's hard case.

Bars:
  * batch against single, chunk sizes, pair orders, two calls: the result structures byte for byte;
  * against the model (only pairs whose model log keeps every convergence test outside +-10 % of its
    threshold, the condition of test_loop_closure's fixture; at least 8 of the 14):
    test_loop_closure_matches_model's bars: status, sizes and iteration count equal, pose within
    1e-4, fitness within relative 1e-5 at the device's transform, between within 1e-5.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import loop_model as M
import test_loop_closure as TL
from feature_base_pointcloud_registration_amd import api
from feature_base_pointcloud_registration_amd.fbr_types import (FBR_LOOP_CLOSED, FBR_LOOP_REJECTED_FITNESS, POINT_XYZI,
                                                                FbrLoopPair, FbrLoopResult, default_params, icp_params,
                                                                loop_params, sc_params)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "feature_base_pointcloud_registration_amd", "csrc")
NATIVE = os.path.join(REPO, "tests", "native")
NEW_SYMBOLS = ("fbr_loop_candidates", "fbr_perform_loop_closures", "fbr_icp_align_batch")
# keyframe: (yaw, x, y, z) added to the stored pose
OFFSETS = {12: (0.01, 0.1, 0.05, 0.0), 14: (-0.02, -0.2, 0.15, 0.05), 16: (0.03, 0.35, -0.25, 0.1),
           18: (0.05, 0.6, 0.4, -0.1), 19: (0.03, 0.35, -0.25, 0.1)}
PAIRS = [(6, 0), (7, 1), (8, 2), (9, 3), (10, 4), (11, 5), (12, 6), (13, 6), (14, 5), (15, 4), (16, 3), (17, 2), (18, 1),
         (19, 0)]
POSE_TOL = 1e-4
INVALID_ARG, CAPACITY = -1, -4

raw_bytes = TL.raw_bytes


# ---- the fixture and the candidates model ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    """(P, stored poses, corner clouds, surf clouds, loop params)."""
    P, poses0, corners, surfs, _, _ = TL.fixture()
    poses = poses0.copy()
    gt = TL.gt_pose(TL.N_KF - 1)  # keyframe 19 as the fixture stored it before its drift
    poses[TL.N_KF - 1] = (gt[3], gt[4], gt[5], TL.N_KF - 1, gt[0], gt[1], gt[2], 0.0, 2.0 * (TL.N_KF - 1))
    for k, off in OFFSETS.items():
        for name, v in zip(("yaw", "x", "y", "z"), off):
            poses[name][k] += np.float32(v)
    return P, poses, corners, surfs, loop_params(search_num=2, search_time_diff=10.0)


def candidates(poses, lp, first=0):
    """fbr_loop_candidates: detectLoopClosure's rule for every keyframe i >= first on the store that
    held keyframes 0..i, at that keyframe's own stamp."""
    out = []
    for i in range(first, len(poses)):
        c = M.detect(poses[:i + 1], float(poses["time"][i]), lp)
        if c is not None:
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def model(i):
    P, poses, corners, surfs, lp = fixture()
    return M.perform(P, poses[:i + 1], corners, surfs, float(poses["time"][i]), lp)


# ---- CPU -------------------------------------------------------------------------------------------
def test_batch_symbols_are_exported():
    lib = ctypes.CDLL(api.lib_path())
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in api.EXPORTED_SYMBOLS
    assert ctypes.sizeof(FbrLoopPair) == 40
    assert api.lib().fbr_abi_version() == 4
    for name in ("loop_candidates", "perform_loop_closures", "icp_align_batch"):
        assert callable(getattr(api.Context, name))
    hdr = open(os.path.join(REPO, "include", "fbr.hpp")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name  # the C++ mirror calls each of them


def test_candidates_model_on_the_fixture():
    _, poses, _, _, lp = fixture()
    assert candidates(poses, lp) == PAIRS
    assert candidates(poses, loop_params(search_num=2, search_time_diff=100.0)) == []
    assert candidates(poses, lp, first=13) == PAIRS[7:]
    assert candidates(poses, lp, first=19) == [(19, 0)] and candidates(poses, lp, first=20) == []
    assert candidates(poses[:6], lp) == []  # keyframes 1-5: nobody old enough within the radius


def test_loop_plan_under_sanitizers():
    """csrc/fbr_loop_plan.h alone (tests/native/loop_plan_check.cpp says what it checks), as its own
    program with the sanitizer runtimes linked statically."""
    out_dir = os.path.join(NATIVE, "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "loop_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", CSRC, "-o", exe,
                           os.path.join(NATIVE, "loop_plan_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "loop_plan_check: ok" in r.stdout


# ---- GPU: contexts and the single-pair reference -----------------------------------------------------
def params(exact):
    return fixture()[0] if exact else default_params(16, 1800)


@functools.lru_cache(maxsize=None)
def single_results(exact):
    """{i: fbr_perform_loop_closure's FbrLoopResult when keyframe i was the last one}: one context
    that grows a keyframe at a time."""
    _, poses, corners, surfs, lp = fixture()
    out = {}
    with api.Context(params(exact)) as ctx:
        for i in range(TL.N_KF):
            ctx.keyframes_add(poses[i], corners[i], surfs[i])
            if i >= PAIRS[0][0]:
                out[i] = ctx.perform_loop_closure(float(poses["time"][i]), lp, raw=True)
    return out


@pytest.fixture(scope="module")
def full_ctx():
    P, poses, corners, surfs, _ = fixture()
    with api.Context(P) as ctx:
        TL.add_keyframes(ctx, poses, corners, surfs)
        yield ctx


@pytest.fixture(scope="module")
def plain_full_ctx():
    _, poses, corners, surfs, _ = fixture()
    with api.Context(default_params(16, 1800)) as ctx:
        TL.add_keyframes(ctx, poses, corners, surfs)
        yield ctx


def single_bytes(exact=True):
    return [raw_bytes(single_results(exact)[i]) for i, _ in PAIRS]


# ---- GPU: fbr_loop_candidates ------------------------------------------------------------------------
@pytest.mark.gpu
def test_candidates_equal_the_model(full_ctx):
    _, poses, corners, surfs, lp = fixture()
    assert full_ctx.loop_candidates(lp) == PAIRS == candidates(poses, lp)
    assert full_ctx.loop_candidates(lp, first=13) == PAIRS[7:]
    assert full_ctx.loop_candidates(lp, first=20) == [] and full_ctx.loop_candidates(lp, first=1000) == []
    assert full_ctx.loop_candidates(loop_params(search_num=2, search_time_diff=100.0)) == []
    # detectLoopClosure on the store as it was: keyframes 0..i
    with api.Context(default_params(16, 1800)) as ctx:
        n = 0
        for i in (3, 13, 18):
            while n <= i:
                ctx.keyframes_add(poses[n], corners[n], surfs[n])
                n += 1
            want = ctx.detect_loop_closure(float(poses["time"][i]), lp)
            got = [p for p in full_ctx.loop_candidates(lp) if p[0] == i]
            assert got == ([want] if want is not None else []), i
            assert ctx.loop_candidates(lp, first=i) == got
    # the size query, a capacity that is too small, and one that fits
    L, n = api.lib(), ctypes.c_int64(-1)
    assert L.fbr_loop_candidates(full_ctx._h, ctypes.byref(lp), 0, None, 0, ctypes.byref(n)) == CAPACITY and n.value == 14
    buf = (FbrLoopPair * 14)()
    n.value = -1
    assert L.fbr_loop_candidates(full_ctx._h, ctypes.byref(lp), 0, buf, 5, ctypes.byref(n)) == CAPACITY and n.value == 14
    assert [(p.latest_id, p.closest_id) for p in buf[:5]] == PAIRS[:5] and buf[5].latest_id == 0 == buf[5].closest_id
    assert L.fbr_loop_candidates(full_ctx._h, ctypes.byref(lp), 0, buf, 14, ctypes.byref(n)) == 0 and n.value == 14
    assert all(p.use_guess == 0 and p.reserved_ == 0 and list(p.pose_guess) == [0.0] * 6 for p in buf)
    assert L.fbr_loop_candidates(full_ctx._h, ctypes.byref(lp), 20, None, 0, ctypes.byref(n)) == 0 and n.value == 0
    assert L.fbr_loop_candidates(full_ctx._h, ctypes.byref(lp), 0, None, 3, ctypes.byref(n)) == INVALID_ARG
    assert L.fbr_loop_candidates(full_ctx._h, ctypes.byref(lp), -1, None, 0, ctypes.byref(n)) == INVALID_ARG
    assert L.fbr_loop_candidates(full_ctx._h, ctypes.byref(lp), 0, None, 0, None) == INVALID_ARG


# ---- GPU: the batch against the single call ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact_voxel_order", "default_voxel_order"])
def test_batch_equals_single_byte_for_byte(full_ctx, plain_full_ctx, exact):
    _, _, _, _, lp = fixture()
    single = single_results(exact)
    # the fixture's property, on the reference itself: the pairs stop at many different iterations and
    # in both statuses
    iters = [single[i].icp.iterations for i, _ in PAIRS]
    status = [single[i].status for i, _ in PAIRS]
    print("single iterations:", iters, "status:", status)
    assert len(set(iters)) >= 5 and {FBR_LOOP_CLOSED, FBR_LOOP_REJECTED_FITNESS} <= set(status)
    assert [(single[i].latest_id, single[i].closest_id) for i, _ in PAIRS] == PAIRS
    ctx = full_ctx if exact else plain_full_ctx
    batch = ctx.perform_loop_closures(PAIRS, lp, raw=True)
    assert len(batch) == 14
    for (i, j), r in zip(PAIRS, batch):
        assert raw_bytes(r) == raw_bytes(single[i]), (i, j, r.as_dict(), single[i].as_dict())


@pytest.mark.gpu
def test_chunk_size_and_repetition_do_not_change_a_byte(full_ctx):
    _, _, _, _, lp = fixture()
    want = single_bytes()
    for chunk in (1, 3, 0, 0):
        got = [raw_bytes(r) for r in full_ctx.perform_loop_closures(PAIRS, lp, chunk=chunk, raw=True)]
        assert got == want, chunk


@pytest.mark.gpu
def test_pair_order_and_duplicates_do_not_change_a_byte(full_ctx):
    _, _, _, _, lp = fixture()
    want = dict(zip(PAIRS, single_bytes()))
    rev = PAIRS[::-1]
    assert [raw_bytes(r) for r in full_ctx.perform_loop_closures(rev, lp, raw=True)] == [want[p] for p in rev]
    dup = [PAIRS[13], PAIRS[2], PAIRS[13], PAIRS[7], PAIRS[2]]
    for chunk in (0, 2):
        got = [raw_bytes(r) for r in full_ctx.perform_loop_closures(dup, lp, chunk=chunk, raw=True)]
        assert got == [want[p] for p in dup], chunk


@pytest.mark.gpu
def test_batch_matches_the_model(full_ctx):
    P, poses, corners, surfs, lp = fixture()
    batch = full_ctx.perform_loop_closures(PAIRS, lp)
    compared = []
    for (i, j), d in zip(PAIRS, batch):
        m = model(i)
        assert (m["latest_id"], m["closest_id"]) == (i, j)
        mi = m["icp"]
        if any(0.9 * thr <= value <= 1.1 * thr for tests in mi["log"] for value, thr in tests):
            continue  # a convergence test decided within 10 % of its threshold: rounding may move the count
        compared.append(i)
        assert d["status"] == m["status"] and (d["latest_id"], d["closest_id"]) == (i, j)
        assert (d["n_source"], d["n_target"]) == (m["n_source"], m["n_target"])
        assert (d["icp"]["iterations"], d["icp"]["convergence"]) == (mi["iterations"], mi["convergence"]), i
        assert d["icp"]["converged"] == mi["converged"]
        pc, pm = np.asarray(d["pose_corrected"], np.float64), np.asarray(m["pose_corrected"], np.float64)
        dpos = np.abs(pc[3:] - pm[3:]).max()
        drot = np.abs(np.angle(np.exp(1j * (pc[:3] - pm[:3])))).max()
        print("pair (%d, %d): device - model pose difference %.3g m, %.3g rad" % (i, j, dpos, drot))
        assert dpos <= POSE_TOL and drot <= POSE_TOL, i
        assert np.array_equal(d["pose_closest"], M.pose_of(poses[j]))
        T = d["icp"]["transform"].reshape(4, 4)
        fit = M.fitness(M.xyz(m["source"]), M.xyz(m["target"]), T)
        assert abs(d["icp"]["fitness"] - fit) <= 1e-5 * fit, (i, d["icp"]["fitness"], fit)
        btw = M.between(d["pose_corrected"], d["pose_closest"])
        assert np.abs(d["between"].reshape(4, 4) - btw).max() <= 1e-5, i
    print("compared with the model:", compared)
    assert len(compared) >= 8


@pytest.mark.gpu
def test_pair_with_a_pose_guess_equals_the_scan_context_call(full_ctx):
    _, poses, _, _, lp = fixture()
    sp = sc_params(dist_threshold=1.0)  # any candidate is taken: the test is about the guess
    r, m = full_ctx.perform_loop_closure_sc(float(poses["time"][19]), lp, sp, raw=True)
    assert r.latest_id == 19 and r.closest_id == m.keyframe and r.closest_id != 19
    guess = np.array(list(m.pose_guess), np.float32)
    pair = FbrLoopPair(19, r.closest_id, 1)
    pair.pose_guess[:] = list(m.pose_guess)
    got = full_ctx.perform_loop_closures([pair, (19, r.closest_id, guess)], lp, raw=True)
    assert raw_bytes(got[0]) == raw_bytes(r) and raw_bytes(got[1]) == raw_bytes(r)
    # a guess of the test's own, so that the guess certainly differs from the stored pose: the single
    # call on a store whose keyframe 19 has the guess as its pose reads it in the same places
    P, _, corners, surfs, _ = fixture()
    moved = poses.copy()
    moved["yaw"][19] += np.float32(0.02)
    moved["x"][19] += np.float32(0.2)
    with api.Context(P) as ctx:
        TL.add_keyframes(ctx, moved, corners, surfs)
        want = ctx.perform_loop_closure(float(poses["time"][19]), lp, raw=True)
    assert (want.latest_id, want.closest_id) == (19, 0)
    got = full_ctx.perform_loop_closures([(19, 0, M.pose_of(moved[19])), (19, 0)], lp, raw=True)
    assert raw_bytes(got[0]) == raw_bytes(want)
    assert raw_bytes(got[1]) == raw_bytes(single_results(True)[19]) != raw_bytes(want)


# ---- GPU: fbr_icp_align_batch ------------------------------------------------------------------------
def icp_batch_cases():
    """[(source, target)] with what each case is about."""
    rng = np.random.default_rng(21)
    cube = lambda n, lo=0.0, hi=6.0: rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    tgt = cube(700)

    def moved(n):  # n target points under a small motion: a source that converges
        p = tgt[rng.permutation(len(tgt))[:n]].astype(np.float64)
        c, s = np.cos(0.02), np.sin(0.02)
        return (p @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]).T + [0.05, -0.03, 0.02]).astype(np.float32)

    empty = np.zeros((0, 3), np.float32)
    nan_src = moved(300)
    nan_src[[0, 17, 255, 299]] = np.nan
    nan_src[40, 1] = np.nan
    P, poses, corners, surfs, lp = fixture()
    src19, tgt19, _ = M.loop_clouds(P, poses, corners, surfs, 19, 0, lp)
    cases = [("empty_source", empty, tgt), ("empty_target", moved(65), empty)]
    cases += [("source_%d" % n, moved(n), tgt) for n in (1, 2, 255, 256, 257)]
    cases += [("nan_source", nan_src, tgt),
              ("far_source", moved(300) + np.float32([40.0 + 6.0, 0.0, 0.0]), tgt),  # 40 m outside the box
              ("fixture_19_0", src19, tgt19)]
    return [(name, s if s.dtype == POINT_XYZI else TL.cloud(s), t if t.dtype == POINT_XYZI else TL.cloud(t))
            for name, s, t in cases]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["default", "gate_1e-4", "max_iterations_1", "max_iterations_3"])
def test_icp_align_batch_equals_icp_align(full_ctx, which):
    ip = {"default": icp_params(), "gate_1e-4": icp_params(max_correspondence_distance=1e-4),
          "max_iterations_1": icp_params(max_iterations=1), "max_iterations_3": icp_params(max_iterations=3)}[which]
    cases = icp_batch_cases()
    single = [full_ctx.icp_align(s, t, ip, raw=True) for _, s, t in cases]
    if which == "gate_1e-4":  # fewer than 3 correspondences everywhere
        assert all(r.n_correspondences < 3 and r.converged == 0 for r in single)
    if which == "default":
        by = {name: r for (name, _, _), r in zip(cases, single)}
        assert by["source_255"].converged == 1 and by["source_255"].iterations > 1
        assert by["source_2"].n_correspondences == 2 and by["empty_source"].n_correspondences == 0
        assert by["empty_target"].n_correspondences == 0 and by["nan_source"].n_correspondences == 295
        assert by["far_source"].converged == 1
        print("single iterations:", {name: r.iterations for (name, _, _), r in zip(cases, single)})
    for chunk in (0, 4):
        batch = full_ctx.icp_align_batch([s for _, s, _ in cases], [t for _, _, t in cases], ip, chunk=chunk, raw=True)
        for (name, _, _), a, b in zip(cases, batch, single):
            assert raw_bytes(a) == raw_bytes(b), (which, chunk, name, a.as_dict(), b.as_dict())
    assert full_ctx.icp_align_batch([], [], ip) == []


# ---- GPU: arguments, side effects, the pose graph ------------------------------------------------------
@pytest.mark.gpu
def test_invalid_input_is_refused_and_harmless(full_ctx):
    _, _, _, _, lp = fixture()
    L, h = api.lib(), full_ctx._h
    out = (FbrLoopResult * 2)()

    def call(pairs, n=None, chunk=0, res=out):
        arr = (FbrLoopPair * max(len(pairs), 1))(*[FbrLoopPair(a, b) for a, b in pairs])
        return L.fbr_perform_loop_closures(h, ctypes.byref(lp), arr, len(pairs) if n is None else n, chunk, res)

    for bad in ((20, 0), (19, 20), (-1, 0), (19, -1), (7, 7)):
        assert call([(19, 0), bad]) == INVALID_ARG, bad
    assert call([(19, 0)], res=None) == INVALID_ARG
    assert call([(19, 0)], n=-1) == INVALID_ARG
    assert call([(19, 0)], chunk=-1) == INVALID_ARG
    assert L.fbr_perform_loop_closures(h, ctypes.byref(lp), None, 1, 0, out) == INVALID_ARG
    assert L.fbr_perform_loop_closures(h, None, None, 0, 0, None) == INVALID_ARG
    assert L.fbr_perform_loop_closures(h, ctypes.byref(lp), None, 0, 0, None) == 0  # no pairs: nothing to do
    assert full_ctx.perform_loop_closures([], lp) == []
    ip = icp_params()
    one = TL.cloud(np.zeros((3, 3), np.float32))
    res = (type(full_ctx.icp_align(one, one, raw=True)) * 1)()
    ptrs, cnt, neg = (ctypes.c_void_p * 1)(one.ctypes.data), (ctypes.c_int64 * 1)(3), (ctypes.c_int64 * 1)(-3)
    null = (ctypes.c_void_p * 1)(None)
    assert L.fbr_icp_align_batch(h, ptrs, neg, ptrs, cnt, 1, ctypes.byref(ip), 0, res) == INVALID_ARG
    assert L.fbr_icp_align_batch(h, ptrs, cnt, ptrs, neg, 1, ctypes.byref(ip), 0, res) == INVALID_ARG
    assert L.fbr_icp_align_batch(h, null, cnt, ptrs, cnt, 1, ctypes.byref(ip), 0, res) == INVALID_ARG
    assert L.fbr_icp_align_batch(h, ptrs, cnt, ptrs, cnt, -1, ctypes.byref(ip), 0, res) == INVALID_ARG
    assert L.fbr_icp_align_batch(h, ptrs, cnt, ptrs, cnt, 1, ctypes.byref(ip), 0, None) == INVALID_ARG
    assert L.fbr_icp_align_batch(h, ptrs, cnt, ptrs, cnt, 1, None, 0, res) == INVALID_ARG
    # a valid call afterwards returns the right bytes
    want = single_bytes()
    got = full_ctx.perform_loop_closures([PAIRS[13], PAIRS[0]], lp, raw=True)
    assert [raw_bytes(r) for r in got] == [want[13], want[0]]


@pytest.mark.gpu
def test_batch_leaves_map_keyframes_and_resources_alone():
    from feature_base_pointcloud_registration_amd import synth
    import pyoracle as O
    P, poses, corners, surfs, lp = fixture()
    cmap, smap = synth.config_map("C1")
    gt, guess = synth.job(3)
    f = O.Stream(P).features(synth.scan(gt, 16, 1800, seed=3))
    base = api.live_resources()
    ctx = api.Context(P)
    ctx.set_map(cmap, smap)
    TL.add_keyframes(ctx, poses, corners, surfs)
    c0, s0 = ctx.get_map()
    p0, st0 = ctx.register(f["corner"], f["surf"], guess)
    r = ctx.perform_loop_closures(PAIRS[9:], lp, chunk=2)
    assert [d["status"] for d in r] == [FBR_LOOP_CLOSED] * 5
    held = api.live_resources()
    c1, s1 = ctx.get_map()
    p1, st1 = ctx.register(f["corner"], f["surf"], guess)
    assert ctx.keyframes_count() == TL.N_KF and ctx.loop_candidates(lp) == PAIRS
    ctx.close()
    assert c0.tobytes() == c1.tobytes() and s0.tobytes() == s1.tobytes()
    assert p0.tobytes() == p1.tobytes() and st0 == st1
    assert held[0] > base[0] and api.live_resources() == base


@pytest.mark.gpu
def test_batch_results_feed_the_pose_graph():
    P, poses, corners, surfs, lp = fixture()
    with api.Context(P) as ctx:
        TL.add_keyframes(ctx, poses, corners, surfs)
        ctx.pg_reset()
        ctx.pg_add_prior(0, M.pose_of(poses[0]), [1e-2, 1e-2, np.pi ** 2, 1e8, 1e8, 1e8])
        for k in range(1, TL.N_KF):
            ctx.pg_add_between_poses(k - 1, k, M.pose_of(poses[k - 1]), M.pose_of(poses[k]), [1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4])
        n0 = ctx.pg_factor_count()
        res = ctx.perform_loop_closures(ctx.loop_candidates(lp), lp, raw=True)
        added = [ctx.pg_add_loop(r) for r in res]
        assert added == [r.status == FBR_LOOP_CLOSED for r in res] and sum(added) == 9
        assert ctx.pg_factor_count() == n0 + 9
        ctx.pg_optimize()
        ctx.pg_apply()
        assert ctx.keyframes_count() == TL.N_KF
