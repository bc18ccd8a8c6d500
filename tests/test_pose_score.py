"""Pose scoring on the device (fbr_score_poses, fbr_pose_search, Context.relocalize_search) against
the float32 model of tests/score_model.py: every correspondence key, the counts, the sums within
the reordering bound of non-negative double terms, on the inputs where a grid search goes wrong
(tests/knn_model.py) and on rotated poses; batch independence; arguments and state; and the C1
relocalisation from a seed the Gauss-Newton registration cannot use.

The map grid's layout and cell sizes come from environment knobs read at the map build, so those
variants, and the live-resource count, run in child processes (this file run as a script).
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import knn_model as K  # noqa: E402
import score_model as S  # noqa: E402
from feature_base_pointcloud_registration_amd.fbr_types import (POSE_SCORE, default_params, pose_lattice,  # noqa: E402
                                                                 ptr, score_params)

ERR_ARG, ERR_STATE = -1, -7
KNOBS = ("FBR_GRID_SPARSE", "FBR_KNN_CELL", "FBR_KNN_CELL_X")


def lattice_params(leaves=(K.LEAF_C, K.LEAF_S)):
    return default_params(16, 1800, crop_half=K.CROP_HALF, mapping_corner_leaf_size=leaves[0],
                          mapping_surf_leaf_size=leaves[1])


def run_lattice(ctx, cases):
    """Every case set scored at its own guess with and without the crop box: name/crop -> (record, keys)."""
    out = {}
    for c in cases:
        for crop in (1, 0):
            rec, keys = ctx.score_poses(c["corner"], c["surf"], c["guess"][None], score_params(use_crop=crop), keys=True)
            out["%s/%d" % (c["name"], crop)] = (rec[0], keys[0])
    return out


# ------------------------------------------------------------------------------------ the children
def child_lattice(out_path):
    from feature_base_pointcloud_registration_amd import api
    lat = K.cloud(K.lattice_points())
    out = {}
    with api.Context(lattice_params()) as ctx:
        ctx.set_map(lat, lat)
        out["map_c"], out["map_s"] = ctx.get_map()
        info = ctx.map_grid_info()
        out["info"] = np.array([int(info["sparse"]), *info["dims"]], np.int64)
        for name, (rec, keys) in run_lattice(ctx, K.lattice_cases()).items():
            out[name + "/rec"], out[name + "/keys"] = rec, keys
    np.savez(out_path, **out)


def child_resources():
    from feature_base_pointcloud_registration_amd import api
    s = K.structured_case()
    base = api.live_resources()
    ctx = api.Context(default_params(16, 1800))
    alive = api.live_resources()
    ctx.set_map(s["corner_map"], s["surf_map"])
    mapped = api.live_resources()
    poses = S.lattice(s["gt"][None], *S.STRUCT_LATTICE)
    ctx.score_poses(s["corner"], s["surf"], poses[:3])
    ctx.score_poses(s["corner"], s["surf"], poses, keys=True)  # every scratch array grows
    ctx.pose_search(s["corner"], s["surf"], poses[:2], pose_lattice(*S.STRUCT_LATTICE), 5, score_params(pose_chunk=7))
    mid = api.live_resources()
    ctx.close()
    print(json.dumps(dict(base=base, alive=alive, mapped=mapped, mid=mid, end=api.live_resources())))


if __name__ == "__main__":
    if sys.argv[1] == "lattice":
        child_lattice(sys.argv[2])
    else:
        child_resources()
    sys.exit(0)


def run_child(args, env_set=None):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(env_set or {})
    p = subprocess.run([sys.executable, os.path.abspath(__file__), *args], env=env, capture_output=True, text=True,
                       timeout=240, cwd=REPO)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


# ------------------------------------------------------------------------------------ the parent
pytestmark = pytest.mark.gpu

from feature_base_pointcloud_registration_amd import api  # noqa: E402


def sums_close(got, want, n_terms):
    """Two sums of the same non-negative doubles in different orders: within n * 2^-52, relatively."""
    return abs(float(got) - float(want)) <= n_terms * 2.0 ** -52 * abs(float(want))


def assert_record(got, want, keys_got, keys_want, where):
    bad = np.flatnonzero(keys_got != keys_want)
    assert len(bad) == 0, (where, len(bad), bad[:5], keys_got[bad[:5]], keys_want[bad[:5]])
    assert list(got["n"]) == list(want["n"]) and list(got["n_in"]) == list(want["n_in"]), (where, got, want)
    n = int(want["n"].sum())
    for k in range(2):
        assert sums_close(got["sum_d2"][k], want["sum_d2"][k], n), (where, k, got, want)
    # the outlier term is one exact product and one sum, the mean one division
    assert sums_close(got["fitness"], want["fitness"], n + 3), (where, got, want)


@pytest.fixture(scope="module")
def cases():
    return K.lattice_cases()


_CTX, _DENSE = {}, {}


def lattice_ctx(leaves):
    """The context over the lattice map at these mapping leaves, created once."""
    if leaves not in _CTX:
        _CTX[leaves] = api.Context(lattice_params(leaves))
        lat = K.cloud(K.lattice_points())
        _CTX[leaves].set_map(lat, lat)
    return _CTX[leaves]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for ctx in _CTX.values():
        ctx.close()
    _CTX.clear()
    _DENSE.clear()


def dense_results(cases):
    """The dense 1 m-cell context's records and keys, computed once: the children compare with them."""
    if not _DENSE:
        _DENSE.update(run_lattice(lattice_ctx((K.LEAF_C, K.LEAF_S)), cases))
    return _DENSE


@pytest.mark.parametrize("leaves,dims", [((K.LEAF_C, K.LEAF_S), (49, 13, 7)), ((0.1, 0.2), (97, 25, 13))])
def test_lattice_map_key_for_key(cases, leaves, dims):
    """Mapping leaves 0.2 / 0.4 give 1 m x 0.25 m cells, 0.1 / 0.2 give 0.5 m x 0.125 m."""
    ctx = lattice_ctx(leaves)
    info = ctx.map_grid_info()
    assert not info["sparse"] and info["dims"] == dims, info
    mc, ms = ctx.get_map()
    lat = K.lattice_points()
    for m in (mc, ms):  # one point per voxel: the start-up filter kept every point as it is
        assert len(m) == len(lat) and np.array_equal(np.unique(K.xyz_of(m), axis=0), np.unique(lat, axis=0))
    res = dense_results(cases) if leaves == (K.LEAF_C, K.LEAF_S) else run_lattice(ctx, cases)
    n_q = n_none = 0
    for c in cases:
        T = S.affine32(c["guess"])
        for crop in (1, 0):
            want, wkeys = S.score(K.xyz_of(mc), K.xyz_of(ms), K.xyz_of(c["corner"]), K.xyz_of(c["surf"]), T, K.CROP_HALF,
                                  1.0, bool(crop))
            rec, keys = res["%s/%d" % (c["name"], crop)]
            assert_record(rec, want, keys, wkeys, (c["name"], crop))
            n_q += len(keys)
            n_none += int((keys == S.NONE).sum())
    assert n_q > 9000 and 0.02 * n_q < n_none < 0.5 * n_q, (n_q, n_none)
    far = next(c for c in cases if c["name"] == "far")
    q = np.vstack([K.xyz_of(far["corner"]), K.xyz_of(far["surf"])])
    assert (res["far/1"][1][np.abs(q).max(1) > 1e7] == S.NONE).all() and (np.abs(q).max(1) > 1e7).sum() == 3


def test_designed_ties_and_gate_resolve_as_the_model_says(cases):
    """The 12-way ties go to the lowest map index, d2 == g2 is no inlier and one float below is."""
    ctx = lattice_ctx((K.LEAF_C, K.LEAF_S))
    mc, ms = (K.xyz_of(m) for m in ctx.get_map())
    res = dense_results(cases)
    seen = set()
    for c in cases:
        if not c["name"].startswith("ties_gate_crop"):
            continue
        nc = len(c["corner"])
        keys = res[c["name"] + "/1"][1]
        for m, scan, kk in ((mc, K.xyz_of(c["corner"]), keys[:nc]), (ms, K.xyz_of(c["surf"]), keys[nc:])):
            for n, star in enumerate(K.STARS):
                for i in np.flatnonzero((scan == np.float32(star)).all(1)):
                    tied = np.flatnonzero(K.dist2(scan[i], m)[0] == np.float32(0.5))
                    assert len(tied) == 12 and kk[i] == (np.uint64(np.float32(0.5).view(np.uint32)) << np.uint64(32)) | np.uint64(tied[0])
                    seen.add("star%d" % n)
    assert {"star0", "star1", "star2"} <= seen
    # the gate: a query exactly 1 m from its only neighbour in reach has no key; at gate^2 one float
    # above d2 it has one
    m = K.cloud(np.float32([[0, 0, 0], [40, 0, 0], [0, 40, 0], [0, 0, 9]]))
    q = K.cloud(np.float32([[1, 0, 0], [0, 0.75, 0], [0, 0, -0.5]]))
    with api.Context(default_params(16, 1800)) as c2:
        c2.set_map(m, m)
        mm = K.xyz_of(c2.get_map()[1])
        origin = int(np.flatnonzero((mm == 0).all(1))[0])
        for gate, inl in ((1.0, [False, True, True]), (0.75, [False, False, True]), (0.5, [False, False, False]),
                          (float(np.nextafter(np.float32(0.75), np.float32(1))), [False, True, True])):
            rec, keys = c2.score_poses(q[:0], q, np.zeros((1, 6), np.float32), score_params(gate=gate), keys=True)
            want, wkeys = S.score(mm, mm, np.zeros((0, 3), np.float32), K.xyz_of(q), np.eye(4, dtype=np.float32)[:3],
                                  (30, 30, 10), gate)
            assert_record(rec[0], want, keys[0], wkeys, gate)
            assert [bool(k != S.NONE) for k in keys[0]] == inl, (gate, keys)
            assert all(int(k & np.uint64(0xFFFFFFFF)) == origin for k in keys[0] if k != S.NONE)


def test_gate_half_keeps_exactly_the_model_inliers(cases):
    ctx = lattice_ctx((K.LEAF_C, K.LEAF_S))
    mc, ms = (K.xyz_of(m) for m in ctx.get_map())
    res = dense_results(cases)
    n_in = n_out = 0
    for c in cases:
        rec, keys = ctx.score_poses(c["corner"], c["surf"], c["guess"][None], score_params(gate=0.5), keys=True)
        want, wkeys = S.score(mc, ms, K.xyz_of(c["corner"]), K.xyz_of(c["surf"]), S.affine32(c["guess"]), K.CROP_HALF, 0.5)
        inl = wkeys != S.NONE
        full = res[c["name"] + "/1"][1]  # the device's keys at gate 1.0
        assert np.array_equal(keys[0][inl], full[inl]) and (keys[0][~inl] == S.NONE).all(), c["name"]
        assert_record(rec[0], want, keys[0], wkeys, c["name"])
        n_in += int(inl.sum())
        n_out += int((~inl & (full != S.NONE)).sum())
    assert n_in > 1000 and n_out > 100, (n_in, n_out)  # inliers at 1 m that the 0.5 m gate drops


VARIANTS = {  # environment -> (sparse, grid dims) on the 0.2 / 0.4 leaves
    "sparse_1m": ({"FBR_GRID_SPARSE": "1"}, 1, (49, 13, 7)),
    "sparse_0.5m": ({"FBR_GRID_SPARSE": "1", "FBR_KNN_CELL": "0.5", "FBR_KNN_CELL_X": "0.125"}, 1, (97, 25, 13)),
    "cell_0.25_x_1": ({"FBR_KNN_CELL": "0.25", "FBR_KNN_CELL_X": "1"}, 0, (13, 49, 25)),
    "cell_2_x_0.5": ({"FBR_KNN_CELL": "2", "FBR_KNN_CELL_X": "0.5"}, 0, (25, 7, 4)),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_grid_layouts_and_cell_sizes_give_the_dense_bytes(variant, cases, tmp_path):
    env, sparse, dims = VARIANTS[variant]
    out = str(tmp_path / "out.npz")
    run_child(["lattice", out], env)
    r = np.load(out)
    assert (int(r["info"][0]), tuple(int(v) for v in r["info"][1:])) == (sparse, dims), r["info"]
    mc, ms = lattice_ctx((K.LEAF_C, K.LEAF_S)).get_map()
    assert r["map_c"].tobytes() == mc.tobytes() and r["map_s"].tobytes() == ms.tobytes()
    for name, (rec, keys) in dense_results(cases).items():
        assert r[name + "/rec"].tobytes() == rec.tobytes(), name
        assert np.array_equal(r[name + "/keys"], keys), name


# ------------------------------------------------------------------------------------ rotated poses
@pytest.fixture(scope="module")
def struct_ctx():
    s = K.structured_case()
    with api.Context(default_params(16, 1800)) as ctx:
        ctx.set_map(s["corner_map"], s["surf_map"])
        yield ctx


def test_rotated_poses_and_search_order(struct_ctx):
    R = S.structured_reference()
    s = R["case"]
    mc, ms = struct_ctx.get_map()  # the reference took the installed order from the CPU oracle
    assert np.array_equal(K.xyz_of(mc), K.xyz_of(s["corner_map"])) and np.array_equal(K.xyz_of(ms), K.xyz_of(s["surf_map"]))
    rec, keys = struct_ctx.score_poses(s["corner"], s["surf"], R["poses"], keys=True)
    for i in range(len(rec)):
        assert_record(rec[i], R["records"][i], keys[i], R["keys"][i], i)
    seed = s["gt"][None]
    for top_k in (1, 5, 125):
        poses, sc, idx = struct_ctx.pose_search(s["corner"], s["surf"], seed, pose_lattice(*S.STRUCT_LATTICE), top_k)
        assert np.array_equal(idx, R["order"][:top_k]), (top_k, idx)
        assert poses.tobytes() == R["poses"][idx].tobytes()
        assert sc.tobytes() == rec[idx].tobytes()
    assert idx[0] == 62 and np.array_equal(poses[0], s["gt"])


def test_batch_independence(struct_ctx):
    R = S.structured_reference()
    s = R["case"]
    poses = R["poses"][[3, 62, 124, 62, 17, 0, 99]]  # pose 62 twice
    one = struct_ctx.score_poses(s["corner"], s["surf"], poses)
    again = struct_ctx.score_poses(s["corner"], s["surf"], poses)
    assert one.tobytes() == again.tobytes()
    seven = np.concatenate([struct_ctx.score_poses(s["corner"], s["surf"], p[None]) for p in poses])
    assert one.tobytes() == seven.tobytes()
    for chunk in (3, 1, 7, 64):
        assert one.tobytes() == struct_ctx.score_poses(s["corner"], s["surf"], poses, score_params(pose_chunk=chunk)).tobytes()
    assert one[1].tobytes() == one[3].tobytes()
    rec, keys = struct_ctx.score_poses(s["corner"], s["surf"], poses, score_params(pose_chunk=3), keys=True)
    assert rec.tobytes() == one.tobytes() and np.array_equal(keys, R["keys"][[3, 62, 124, 62, 17, 0, 99]])


# ------------------------------------------------------------------------------------ arguments and state
def raw_score(ctx, sp, corner, n_corner, surf, n_surf, poses, n_poses, out):
    return api.lib().fbr_score_poses(ctx._h, None if sp is None else ctypes.byref(sp), corner, n_corner, surf, n_surf,
                                     poses, n_poses, out, None)


def raw_search(ctx, sp, c, nc, s, ns, seeds, n_seeds, lat, top_k, poses, n_out):
    return api.lib().fbr_pose_search(ctx._h, None if sp is None else ctypes.byref(sp), c, nc, s, ns, seeds, n_seeds,
                                     None if lat is None else ctypes.byref(lat), top_k, poses, None, None, n_out)


def test_arguments_and_state(struct_ctx):
    s = S.structured_reference()["case"]
    ctx = struct_ctx
    c, p = np.ascontiguousarray(s["corner"]), np.ascontiguousarray(s["surf"])
    poses = np.ascontiguousarray(S.structured_reference()["poses"][:4])
    out = np.zeros(4, POSE_SCORE)
    sp, lat = score_params(), pose_lattice(*S.STRUCT_LATTICE)
    n_out = ctypes.c_int64(-5)
    top = np.zeros((8, 6), np.float32)
    map0, kf0 = ctx.get_map(), ctx.keyframes_count()
    args = (ptr(c), len(c), ptr(p), len(p))
    # no installed map
    with api.Context(default_params(16, 1800)) as fresh:
        assert raw_score(fresh, sp, *args, ptr(poses), 4, ptr(out)) == ERR_STATE
        assert raw_search(fresh, sp, *args, ptr(poses), 1, lat, 3, ptr(top), ctypes.byref(n_out)) == ERR_STATE
        assert raw_score(fresh, None, *args, ptr(poses), 4, ptr(out)) == ERR_ARG  # arguments come first
    # null and negative arguments
    assert api.lib().fbr_score_poses(None, ctypes.byref(sp), *args, ptr(poses), 4, ptr(out), None) == ERR_ARG
    assert raw_score(ctx, None, *args, ptr(poses), 4, ptr(out)) == ERR_ARG
    assert raw_score(ctx, sp, None, len(c), ptr(p), len(p), ptr(poses), 4, ptr(out)) == ERR_ARG
    assert raw_score(ctx, sp, ptr(c), len(c), None, len(p), ptr(poses), 4, ptr(out)) == ERR_ARG
    assert raw_score(ctx, sp, ptr(c), -1, ptr(p), len(p), ptr(poses), 4, ptr(out)) == ERR_ARG
    assert raw_score(ctx, sp, ptr(c), len(c), ptr(p), -1, ptr(poses), 4, ptr(out)) == ERR_ARG
    assert raw_score(ctx, sp, *args, None, 4, ptr(out)) == ERR_ARG
    assert raw_score(ctx, sp, *args, ptr(poses), 4, None) == ERR_ARG
    assert raw_score(ctx, sp, *args, ptr(poses), -1, ptr(out)) == ERR_ARG
    for bad in (dict(gate=0.0), dict(gate=-0.5), dict(gate=float(np.nextafter(np.float32(1), np.float32(2)))),
                dict(gate=float("nan")), dict(gate=float("inf")), dict(pose_chunk=-1), dict(use_crop=2), dict(use_crop=-1)):
        assert raw_score(ctx, score_params(**bad), *args, ptr(poses), 4, ptr(out)) == ERR_ARG, bad
        assert raw_search(ctx, score_params(**bad), *args, ptr(poses), 1, lat, 3, ptr(top), ctypes.byref(n_out)) == ERR_ARG, bad
    assert raw_search(ctx, sp, *args, ptr(poses), 1, None, 3, ptr(top), ctypes.byref(n_out)) == ERR_ARG
    assert raw_search(ctx, sp, *args, ptr(poses), 1, lat, 3, ptr(top), None) == ERR_ARG
    assert raw_search(ctx, sp, *args, ptr(poses), 1, lat, 3, None, ctypes.byref(n_out)) == ERR_ARG
    assert raw_search(ctx, sp, *args, ptr(poses), 1, lat, -1, ptr(top), ctypes.byref(n_out)) == ERR_ARG
    assert raw_search(ctx, sp, *args, None, 1, lat, 3, ptr(top), ctypes.byref(n_out)) == ERR_ARG
    assert raw_search(ctx, sp, *args, ptr(poses), -1, lat, 3, ptr(top), ctypes.byref(n_out)) == ERR_ARG
    for bad in (pose_lattice((1, 1, 1, 1), (0.01, 0.01, 0.01, 0.01)), pose_lattice((512, 0, 0, 0), (1, 0, 0, 0)),
                pose_lattice((-1, 0, 0, 0), (1, 0, 0, 0)), pose_lattice((1, 0, 0, 0), (-1, 0, 0, 0)),
                pose_lattice((float("nan"), 0, 0, 0), (1, 0, 0, 0)), pose_lattice((float("inf"), 0, 0, 0), (1, 0, 0, 0))):
        big = np.zeros((1024, 6), np.float32)  # 1024 seeds x 1025 offsets pass 2^20
        assert raw_search(ctx, sp, *args, ptr(big), 1024, bad, 3, ptr(top), ctypes.byref(n_out)) == ERR_ARG
    assert n_out.value == -5 and not out.view(np.uint8).any() and not top.any()  # nothing was written
    # n_poses = 0 succeeds and writes nothing; so do no seeds and top_k = 0
    assert raw_score(ctx, sp, *args, None, 0, None) == 0 and raw_score(ctx, sp, *args, ptr(poses), 0, ptr(out)) == 0
    assert not out.view(np.uint8).any()
    assert raw_search(ctx, sp, *args, None, 0, lat, 3, ptr(top), ctypes.byref(n_out)) == 0 and n_out.value == 0
    n_out.value = -5
    assert raw_search(ctx, sp, *args, ptr(poses), 1, lat, 0, None, ctypes.byref(n_out)) == 0 and n_out.value == 0
    assert not top.any()
    # empty clouds
    R = S.structured_reference()
    mc, ms = (K.xyz_of(m) for m in map0)
    e = p[:0]
    for cc, ss in ((e, p), (c, e), (e, e)):
        rec, keys = ctx.score_poses(cc, ss, poses[:2], keys=True)
        for i in range(2):
            want, wkeys = S.score(mc, ms, K.xyz_of(cc), K.xyz_of(ss), S.affine32(poses[i]), S.STRUCT_CROP_HALF)
            assert_record(rec[i], want, keys[i], wkeys, (len(cc), len(ss), i))
    assert list(rec[0]["n"]) == [0, 0] and rec[0]["fitness"] == np.finfo(np.float64).max
    found, sc, idx = ctx.pose_search(e, e, poses[:1], lat, 3)
    assert list(idx) == [0, 1, 2] and (sc["fitness"] == np.finfo(np.float64).max).all()  # all equal: index order
    # top_k larger than the lattice
    found, sc, idx = ctx.pose_search(c, p, s["gt"][None], lat, 1000)
    assert len(idx) == 125 and np.array_equal(idx, R["order"]) and (np.diff(sc["fitness"]) >= 0).all()
    # a single hypothesis: step 0 everywhere
    found, sc, idx = ctx.pose_search(c, p, poses[:3], pose_lattice(), 2)
    assert len(idx) == 2 and found.tobytes() == poses[idx].tobytes()
    # nothing else changed
    map1 = ctx.get_map()
    assert map0[0].tobytes() == map1[0].tobytes() and map0[1].tobytes() == map1[1].tobytes()
    assert ctx.keyframes_count() == kf0 == 0
    assert api.strerror(ERR_ARG) and callable(api.Context.relocalize_search)


def test_scratch_is_released_with_the_context():
    r = json.loads([ln for ln in run_child(["resources"]).splitlines() if ln.startswith("{")][-1])
    assert all(v >= 0 for v in r["base"])
    assert [a - b for a, b in zip(r["alive"], r["base"])][:2] == [51, 7]  # fbr_create allocates none of it
    assert r["mid"][0] - r["mapped"][0] == 5 and r["mid"][1:] == r["mapped"][1:]  # the five scratch arrays
    assert r["end"] == r["base"]


# ------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def c1_ctx():
    import sc_fixtures as SF
    R = SF.reloc()
    with api.Context(default_params(16, 1800, exact_voxel_order=1)) as ctx:
        ctx.set_map(*R["map"])
        yield ctx


@pytest.mark.parametrize("q", [1, 3])
def test_relocalize_from_a_coarse_seed(c1_ctx, q):
    import sc_fixtures as SF
    R = SF.reloc()
    omap = SF._oracle_map()
    Q = R["queries"][q]
    gt, seed = Q["gt"], S.reloc_seed(q)
    # why the feature is needed: the oracle registered from the seed misses the bound
    p0, _ = S.reloc_seed_oracle(q)
    dt0, dr0 = SF.pose_err(p0, gt)
    print("query", q, "oracle from the seed: %.3g m, %.3g rad" % (dt0, dr0))
    assert dt0 > SF.RELOC_BOUND[0] and dr0 > SF.RELOC_BOUND[1]
    # the search's first pose is within one lattice step per axis of the truth
    lat = pose_lattice(*S.RELOC_LATTICE)
    found, sc, idx = c1_ctx.pose_search(Q["corner_ds"], Q["surf_ds"], seed[None], lat, 3)
    d = found[0].astype(np.float64) - gt
    print("   best lattice pose: fitness %.4g, off by %.3g m, %.3g m, %.3g rad" % (sc[0]["fitness"], d[3], d[4], d[2]))
    assert len(idx) == 3 and abs(d[3]) <= 0.5 and abs(d[4]) <= 0.5 and abs(d[2]) <= 0.1
    # registration from the best three ends within the bound, and where the oracle ends from the same pose
    map0 = c1_ctx.get_map()
    hyps, win = c1_ctx.relocalize_search(Q["scan"], seeds=seed[None], top=3, lattice=lat)
    assert len(hyps) == 3 and win >= 0
    start, pose, st, score = hyps[win]
    # (the call extracts and down-samples the features itself) every start is a pose of the lattice
    hypotheses = S.lattice(seed[None], *S.RELOC_LATTICE)
    assert len(hypotheses) == 2873 and all((hypotheses == h[0]).all(1).any() for h in hyps)
    assert not (np.abs(hypotheses.astype(np.float64) - gt).max(1) < 1e-3).any()  # the truth is not on it
    assert st["converged"] and not st["degenerate"]
    assert score["fitness"] == min(h[3]["fitness"] for h in hyps if h[2]["converged"] and not h[2]["degenerate"])
    dt, dr = SF.pose_err(pose, gt)
    print("   winner %d: fitness %.4g, %.4g m, %.3g rad from the truth" % (win, score["fitness"], dt, dr))
    assert dt <= SF.RELOC_BOUND[0] and dr <= SF.RELOC_BOUND[1]
    op, ost, _ = omap.register(Q["feat"]["corner"], Q["feat"]["surf"], start)
    dpos = float(np.abs(pose[3:] - op[3:]).max())
    drot = float(np.abs(np.angle(np.exp(1j * (pose[:3].astype(np.float64) - op[:3])))).max())
    print("   device - oracle: %.3g m, %.3g rad" % (dpos, drot))
    assert dpos <= 1e-4 and drot <= 1e-4
    # three poses' records against the float32 model: the seed, the best lattice pose, the winner
    mc, ms = (K.xyz_of(m) for m in map0)
    three = np.stack([seed, found[0], pose])
    rec, keys = c1_ctx.score_poses(Q["corner_ds"], Q["surf_ds"], three, keys=True)
    for i in range(3):
        want, wkeys = S.score(mc, ms, K.xyz_of(Q["corner_ds"]), K.xyz_of(Q["surf_ds"]), S.affine32(three[i]),
                              list(R["P"].crop_half), pre=K.near)
        assert_record(rec[i], want, keys[i], wkeys, (q, i))
    print("   fitness at the seed %.4g, at the winner %.4g" % (rec[0]["fitness"], rec[2]["fitness"]))
    assert rec[2]["fitness"] < rec[1]["fitness"] < rec[0]["fitness"]
    map1 = c1_ctx.get_map()
    assert map0[0].tobytes() == map1[0].tobytes() and map0[1].tobytes() == map1[1].tobytes()
