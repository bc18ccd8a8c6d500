"""Registration information on the device (fbr_reg_info_poses, fbr_batch_info,
fbr_reg_info_variances) against tests/info_model.py.

Sums (H, g, rss) are held to n_rows 2^-52 sum|terms| of the model's correctly rounded sums: the worst
case of any summation order, the bound tests/test_gn_direct.py uses for the item partials.  The
spectrum and the covariances are held to the Jacobi's backward-error bound (tests/
test_reg_info_model.py) widened by that summation error and propagated (info_model.cov_bound).
Counts are exact.

The map grid's layout is an environment knob read once per process, so the comparison with the
Gauss-Newton kernels' own partials runs in child processes (this file run as a script).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import info_cases as C  # noqa: E402
import info_model as M  # noqa: E402
import knn_model as K  # noqa: E402
from feature_base_pointcloud_registration_amd.fbr_types import (FBR_INFO_BAD_POSE, FBR_INFO_NO_ROWS,  # noqa: E402
                                                                 FBR_INFO_NOT_REGISTERED, KEYPOSE, POINT_XYZI, REG_INFO,
                                                                 default_params, info_params, ptr)

F = np.float32
ERR_ARG, ERR_STATE = -1, -7
KNOBS = ("FBR_GRID_SPARSE", "FBR_KNN_CELL", "FBR_KNN_CELL_X", "FBR_KNN_LPQ", "FBR_GN_TAIL", "FBR_KNN_TILE", "FBR_FIT_CACHE")


# ------------------------------------------------------------------------------------ the child
def child(out_path):
    """The structured case registered with a trace; then reg_info over the residual pass's own
    points at the pose that pass ran at.  The crop box is wide: a registration keeps the box of its
    guess through every iteration, reg_info crops around the pose it is given, and with the 4 m box
    of the other tests the two boxes differ by the 0.12 m the pose has moved, which changes the
    neighbours of the queries at the box's faces."""
    from feature_base_pointcloud_registration_amd import api
    s = K.structured_case()
    guess = np.concatenate([-2 * s["gt"][:3], np.zeros(3, F)]).astype(F)
    with api.Context(default_params(16, 1800, crop_half=C.CORRIDOR_CROP, max_iterations=3)) as ctx:
        ctx.set_map(s["corner_map"], s["surf_map"])
        mc, ms = ctx.get_map()
        pose, st, trace = ctx.register(s["corner"], s["surf"], guess, trace=True)
        g = ctx.diag_gn_last()
        it = st["iterations"]
        before = np.asarray(guess if it == 1 else trace[it - 2], F)
        nc = int(g["n_corner"])
        rec = ctx.reg_info(K.cloud(g["points"][:nc]), K.cloud(g["points"][nc:]), before[None])
        g2 = ctx.diag_gn_last()  # reg_info leaves the diagnostics alone
        assert g2["partial"].tobytes() == g["partial"].tobytes() and g2["points"].tobytes() == g["points"].tobytes()
        info = ctx.map_grid_info()
    np.savez(out_path, rec=rec, partial=g["partial"], points=g["points"], nc=nc, before=before, map_c=mc, map_s=ms,
             sparse=int(info["sparse"]), iterations=it)


if __name__ == "__main__":
    child(sys.argv[1])
    sys.exit(0)


# ------------------------------------------------------------------------------------ the parent
pytestmark = pytest.mark.gpu

from feature_base_pointcloud_registration_amd import api, synth  # noqa: E402
from test_reg_info_model import compare  # noqa: E402


def check(rec, want, mag, tag):
    """A device record against the model's record and the magnitudes of its sums' terms."""
    assert list(rec["n_rows"]) == list(want["n_rows"]) and list(rec["n_query"]) == list(want["n_query"]), \
        (tag, rec["n_rows"], want["n_rows"], rec["n_query"], want["n_query"])
    if want["flags"]:
        compare(rec, want, tag)
        return
    n = int(np.sum(want["n_rows"]))
    bound = n * M.EPS * mag
    Hb = M.full_H(bound)
    eH, eg, er = np.abs(rec["H"] - want["H"]), np.abs(rec["g"] - want["g"]), abs(rec["rss"] - want["rss"])
    print("%s: n_rows %s, max |dH| / bound %.3g, |dg| / bound %.3g, |drss| / bound %.3g" % (
        tag, list(rec["n_rows"]), (eH / np.maximum(Hb, 1e-300)).max(), (eg / np.maximum(bound[21:27], 1e-300)).max(),
        er / max(bound[28], 1e-300)))
    assert (eH <= Hb).all(), (tag, "H", eH.max())
    assert (eg <= bound[21:27]).all(), (tag, "g")
    assert er <= bound[28], (tag, "rss")
    compare(rec, want, tag, h_err=np.linalg.norm(Hb), s2_rel=bound[28] / want["rss"] if want["rss"] > 0 else 0.0)


def model_of(ctx, world, pose, crop):
    mc, ms = ctx.get_map()
    return M.info(K.xyz_of(mc), K.xyz_of(ms), K.xyz_of(world["corner"]), K.xyz_of(world["surf"]), pose, crop)


@pytest.fixture(scope="module")
def tiny_ctx():
    t = C.tiny()
    with api.Context(default_params(16, 1800, crop_half=K.CROP_HALF)) as ctx:
        ctx.set_map(t["corner_map"], t["surf_map"])
        yield ctx, t


# ---- 1. the tiny set ----
def test_tiny_set_equals_the_model(tiny_ctx):
    ctx, t = tiny_ctx
    poses = np.stack([t["gt"], np.zeros(6, F)]).astype(F)
    rec = ctx.reg_info(t["corner"], t["surf"], poses)
    assert list(rec["n_query"][0]) == [60, 300]
    for k, name in enumerate(("true", "guess")):
        want, _, mag = model_of(ctx, t, poses[k], K.CROP_HALF)
        assert want["flags"] == 0 and want["n_rows"].sum() > 100
        check(rec[k], want, mag, "tiny/" + name)


# ---- 2. against the Gauss-Newton kernels themselves ----
@pytest.mark.parametrize("sparse", [0, 1])
def test_reproduces_the_gauss_newton_partials(sparse, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    if sparse:
        env["FBR_GRID_SPARSE"] = "1"
    out = str(tmp_path / "child.npz")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=240,
                       cwd=REPO)
    assert p.returncode == 0, p.stderr[-3000:]
    d = np.load(out)
    assert int(d["sparse"]) == sparse and int(d["iterations"]) >= 2
    rec, nc = d["rec"][0], int(d["nc"])
    acc = d["partial"].sum(0)  # 21 AtA, 6 AtB, the row count
    want, r, mag = M.info(K.xyz_of(d["map_c"]), K.xyz_of(d["map_s"]), d["points"][:nc], d["points"][nc:], d["before"], C.CORRIDOR_CROP)
    n = int(acc[27])
    assert n == int(rec["n_rows"].sum()) == int(want["n_rows"].sum()) >= 50
    bound = n * M.EPS * mag  # n_rows 2^-52 sum|terms|, as for the tiny set
    Hb = np.maximum(M.full_H(bound), 1e-300)
    print("sparse %d: %d rows; Gauss-Newton partials vs model %.3g, reg_info vs model %.3g, vs each other %.3g (units of the bound)" % (
        sparse, n, (np.abs(M.full_H(acc[:21]) - want["H"]) / Hb).max(), (np.abs(rec["H"] - want["H"]) / Hb).max(),
        (np.abs(M.full_H(acc[:21]) - rec["H"]) / Hb).max()))
    assert (np.abs(M.full_H(acc[:21]) - rec["H"]) <= M.full_H(bound)).all()
    assert (np.abs(acc[21:27] - rec["g"]) <= bound[21:27]).all()
    assert (np.abs(M.full_H(acc[:21]) - want["H"]) <= M.full_H(bound)).all()  # and the partials against the model
    assert (np.abs(acc[21:27] - want["g"]) <= bound[21:27]).all()
    check(rec, want, mag, "gn_partials/sparse%d" % sparse)


# ---- 4. independence ----
def test_records_do_not_depend_on_the_call(tiny_ctx):
    ctx, t = tiny_ctx
    far = t["gt"].copy()
    far[3] += 50.0
    poses = np.stack([t["gt"], np.zeros(6, F), far]).astype(F)
    rec = ctx.reg_info(t["corner"], t["surf"], poses)
    assert rec[2]["flags"] == FBR_INFO_NO_ROWS and rec[2]["rank"] == 0 and not rec[2]["H"].any()
    assert list(rec[2]["n_query"]) == [60, 300] and list(rec[2]["n_rows"]) == [0, 0]
    assert np.array_equal(rec[2]["cov_tangent"], 1e4 * np.eye(6))
    assert rec[0]["flags"] == 0 and rec[1]["flags"] == 0
    for k in range(3):
        one = ctx.reg_info(t["corner"], t["surf"], poses[k][None])
        assert one[0].tobytes() == rec[k].tobytes(), k
    assert ctx.reg_info(t["corner"], t["surf"], poses, pose_chunk=1).tobytes() == rec.tobytes()
    assert ctx.reg_info(t["corner"], t["surf"], poses, pose_chunk=2).tobytes() == rec.tobytes()
    assert ctx.reg_info(t["corner"], t["surf"], poses).tobytes() == rec.tobytes()
    assert ctx.reg_info(t["corner"], t["surf"], poses[::-1].copy())[::-1].tobytes() == rec.tobytes()


# ---- 5. the corridor ----
@pytest.mark.parametrize("yaw,axis", [(0.0, 0), (np.pi / 2, 1)])
def test_corridor_does_not_observe_x(yaw, axis):
    w = C.corridor(yaw=yaw)
    with api.Context(default_params(16, 1800, crop_half=C.CORRIDOR_CROP)) as ctx:
        ctx.set_map(w["corner_map"], w["surf_map"])
        rec = ctx.reg_info(w["corner"], w["surf"], w["pose"][None])[0]
        want, _, mag = model_of(ctx, w, w["pose"], C.CORRIDOR_CROP)
    assert rec["rank"] == 5 and rec["flags"] == 0, (rec["eig"], rec["flags"])
    v0 = rec["evec"][0]
    assert abs(v0[3]) > 0.999 and np.abs(v0[4:]).max() < 0.04, v0  # the unobserved direction: map-frame x
    assert int(np.argmax(rec["var_tangent"][3:])) == axis, rec["var_tangent"]
    assert list(rec["n_query"]) == [60, 320], rec["n_query"]  # a few hundred queries in all
    check(rec, want, mag, "corridor/yaw%.2f" % yaw)


def test_corridor_with_an_end_wall_observes_x():
    w = C.corridor(end_wall=True)
    with api.Context(default_params(16, 1800, crop_half=C.CORRIDOR_CROP)) as ctx:
        ctx.set_map(w["corner_map"], w["surf_map"])
        rec = ctx.reg_info(w["corner"], w["surf"], w["pose"][None])[0]
        want, _, mag = model_of(ctx, w, w["pose"], C.CORRIDOR_CROP)
    assert rec["rank"] == 6, rec["eig"]
    check(rec, want, mag, "corridor/end_wall")


# ---- 6. the batch ----
def _batch_inputs():
    gts, guesses, scans = [], [], []
    for j in range(3):
        gt, guess = synth.job(7300 + j)
        s = synth.scan(gt, 16, 1800, seed=7300 + j)
        scans.append(s[:300].copy() if j == 2 else s)  # job 2: too few features to register
        guesses.append(guess)
    return scans, np.asarray(guesses, F)


def test_batch_info_equals_reg_info_of_each_job():
    """A cloud is summed in the canonical order of its points, so the batch's Morton-ordered
    down-samples and Context.voxel_grid's key-ordered ones give the same bytes."""
    P =synth.config_params("C1", max_batch=3, exact_voxel_order=1)
    cmap, smap = synth.config_map("C1")
    scans, guesses = _batch_inputs()
    with api.Context(P) as ctx:
        ctx.set_map(cmap, smap)
        ctx.batch_stage(scans, guesses)
        ctx.batch_launch()
        poses, stats = ctx.batch_results()
        info = ctx.batch_info()
        poses2, stats2 = ctx.batch_results()
        assert poses.tobytes() == poses2.tobytes() and stats.tobytes() == stats2.tobytes()
        assert list(stats["status"]) == [0, 0, 1], stats["status"]
        assert info[2]["flags"] == FBR_INFO_NOT_REGISTERED and info[2]["rank"] == 0 and not info[2]["H"].any()
        assert ctx.batch_info().tobytes() == info.tobytes()
        # job 1 alone
        ctx.batch_stage(scans[1:2], guesses[1:2])
        ctx.batch_launch()
        alone = ctx.batch_info()
        assert alone[0].tobytes() == info[1].tobytes()
        # each registered job against reg_info of its own features at its result pose
        for j in range(2):
            ctx.reset_stream()
            f = ctx.features(scans[j])
            corner = ctx.voxel_grid(f["corner"], P.mapping_corner_leaf_size)
            surf = ctx.voxel_grid(f["surf"], P.mapping_surf_leaf_size)
            assert (len(corner), len(surf)) == (stats["n_corner_ds"][j], stats["n_surf_ds"][j]) == tuple(info[j]["n_query"])
            one = ctx.reg_info(corner, surf, poses[j][None])[0]
            assert list(one["n_rows"]) == list(info[j]["n_rows"]) and one["rank"] == info[j]["rank"], j
            print("job %d: n_rows %s rank %d, max |dH| %.3g of %.3g" % (j, list(one["n_rows"]), one["rank"],
                                                                     np.abs(one["H"] - info[j]["H"]).max(), np.abs(one["H"]).max()))
            assert one.tobytes() == info[j].tobytes(), j


# ---- 8. the pose graph ----
def test_information_variances_let_gps_correct_the_unobserved_axis():
    """Five key poses along the corridor, odometry wrong by 1 m along x at the last one, a GPS fix on
    it at the true position, node 0 held by a tight prior.  With LIO-SAM's constant between-variances
    the chain is stiff along x and the fix is overruled; with the registration's own variances
    (floored at those constants) x is known to be unobserved and the fix moves the node."""
    xs = [-2.0, -1.0, 0.0, 1.0, 2.0]
    const = np.array([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4])
    odo = np.array([[0, 0, 0, x, 0, 0] for x in xs], F)
    odo[-1, 3] += 1.0
    w0 = C.corridor()
    with api.Context(default_params(16, 1800, crop_half=C.CORRIDOR_CROP)) as ctx:
        ctx.set_map(w0["corner_map"], w0["surf_map"])
        var = []
        for x in xs[1:]:  # the registration of node k's scan, at its true pose
            w = C.corridor(centre=(x, 0.0, 0.0))
            rec = ctx.reg_info(w["corner"], w["surf"], w["pose"][None])[0]
            assert rec["rank"] == 5
            var.append(api.reg_info_variances(rec, const))
            assert var[-1][3] > 1e3 and (var[-1][[0, 1, 2, 4, 5]] <= 1e-3).all(), var[-1]
        kp = np.zeros(5, KEYPOSE)
        kp["x"], kp["time"] = odo[:, 3], np.arange(5.0)
        for k in range(5):
            ctx.keyframes_add(kp[k], np.zeros(3, POINT_XYZI), np.zeros(3, POINT_XYZI))
        moved = {}
        for name, vs in (("const", [const] * 4), ("info", var)):
            ctx.pg_reset()
            ctx.pg_add_prior(0, odo[0], np.full(6, 1e-8))
            for k in range(4):
                ctx.pg_add_between_poses(k, k + 1, odo[k], odo[k + 1], vs[k])
            ctx.pg_add_gps(4, np.array([xs[-1], 0.0, 0.0]), np.full(3, 0.01))
            eul, r = ctx.pg_optimize()
            moved[name] = np.abs(eul[4, 3:] - odo[4, 3:].astype(np.float64))
            print(name, "last node moved by", moved[name], "status", r["status"])
    assert moved["info"][0] > moved["const"][0], moved
    assert moved["info"][1] <= moved["const"][1], moved  # (y is never pulled: the device moved it by exactly 0 in both runs)


# ---- 9. arguments and state ----
def test_arguments_and_state():
    L = api.lib()
    assert L.fbr_abi_version() == 4
    t = C.tiny()
    base = api.live_resources()
    ctx = api.Context(default_params(16, 1800, crop_half=K.CROP_HALF, max_batch=2))
    ip = info_params()
    out = np.zeros(4, REG_INFO)
    pose = np.ascontiguousarray(t["gt"][None], F)
    c, s = t["corner"], t["surf"]
    call = lambda h, p, cc, nc, ss, ns, po, npo, o: L.fbr_reg_info_poses(h, p, cc, nc, ss, ns, po, npo, o)  # noqa: E731
    ipp = ctypes.byref(ip)
    assert call(ctx._h, ipp, ptr(c), len(c), ptr(s), len(s), ptr(pose), 1, ptr(out)) == ERR_STATE  # no map
    assert L.fbr_batch_info(ctx._h, ipp, ptr(out)) == ERR_STATE  # no launch
    ctx.set_map(t["corner_map"], t["surf_map"])
    assert call(None, ipp, ptr(c), len(c), ptr(s), len(s), ptr(pose), 1, ptr(out)) == ERR_ARG
    assert call(ctx._h, None, ptr(c), len(c), ptr(s), len(s), ptr(pose), 1, ptr(out)) == ERR_ARG
    assert call(ctx._h, ipp, None, len(c), ptr(s), len(s), ptr(pose), 1, ptr(out)) == ERR_ARG
    assert call(ctx._h, ipp, ptr(c), -1, ptr(s), len(s), ptr(pose), 1, ptr(out)) == ERR_ARG
    assert call(ctx._h, ipp, ptr(c), len(c), ptr(s), -1, ptr(pose), 1, ptr(out)) == ERR_ARG
    assert call(ctx._h, ipp, ptr(c), len(c), ptr(s), len(s), None, 1, ptr(out)) == ERR_ARG
    assert call(ctx._h, ipp, ptr(c), len(c), ptr(s), len(s), ptr(pose), 1, None) == ERR_ARG
    assert call(ctx._h, ipp, ptr(c), len(c), ptr(s), len(s), ptr(pose), -1, ptr(out)) == ERR_ARG
    assert call(ctx._h, ipp, ptr(c), len(c), ptr(s), len(s), None, 0, None) == 0  # n_poses = 0
    for bad in (dict(eig_floor=0.0), dict(unobserved_variance=-1.0), dict(sigma2=-1.0), dict(pose_chunk=-1), dict(eig_floor=np.nan)):
        b = info_params(**bad)
        assert call(ctx._h, ctypes.byref(b), ptr(c), len(c), ptr(s), len(s), ptr(pose), 1, ptr(out)) == ERR_ARG, bad
    assert L.fbr_batch_info(ctx._h, None, ptr(out)) == ERR_ARG and L.fbr_batch_info(ctx._h, ipp, None) == ERR_ARG
    assert L.fbr_batch_info(ctx._h, ipp, ptr(out)) == ERR_STATE  # a map, but no launch yet
    # a non-finite pose is a flagged record, not an error; empty clouds are a record without rows
    bad = np.stack([t["gt"], t["gt"]]).astype(F)
    bad[0, 1], bad[1, 4] = np.nan, np.inf
    r = ctx.reg_info(c, s, bad)
    assert list(r["flags"]) == [FBR_INFO_BAD_POSE] * 2 and not r["H"].any() and (r["rank"] == 0).all()
    r = ctx.reg_info(c[:0], s[:0], pose)
    assert r[0]["flags"] == FBR_INFO_NO_ROWS and list(r[0]["n_query"]) == [0, 0]
    # a registration returns the same bytes before and after reg_info
    g = np.zeros(6, F)
    p1, s1 = ctx.register(c, s, g)
    ctx.reg_info(c, s, pose)
    p2, s2 = ctx.register(c, s, g)
    assert p1.tobytes() == p2.tobytes() and s1 == s2
    # a batch launch, then a single-scan call drops it
    gt, guess = synth.job(1)
    scan = synth.scan(gt, 16, 1800, seed=1)
    ctx.batch_stage([scan], [guess])
    assert L.fbr_batch_info(ctx._h, ipp, ptr(out)) == ERR_STATE  # staged, not launched
    ctx.batch_launch()
    assert L.fbr_batch_info(ctx._h, ipp, ptr(out)) == 0
    ctx.register(c, s, g)
    assert L.fbr_batch_info(ctx._h, ipp, ptr(out)) == ERR_STATE
    ctx.close()
    assert api.live_resources() == base


# ---- 7. the keyframe local map ----
def test_keyframe_local_map_is_not_cropped():
    """Two keyframes (kf_cases.key_poses) hold the corridor's map, each its half in its own frame; after
    extract_surrounding_keyframes the registration map is their local map, which registration does not
    crop.  The context's box is 1 m: a cropped pass would keep a fraction of the rows."""
    import kf_cases
    from feature_base_pointcloud_registration_amd.fbr_types import keyframe_params
    w = C.corridor()
    poses = kf_cases.key_poses([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0)], times=[0.0, 1.0])
    with api.Context(default_params(16, 1800, crop_half=(1.0, 1.0, 1.0))) as ctx:
        for k in range(2):
            c, s = w["corner_map"][k::2].copy(), w["surf_map"][k::2].copy()
            c["x"] -= poses["x"][k]  # lidar frame of key k (no rotation): exact on the 0.25 m lattice
            s["x"] -= poses["x"][k]
            ctx.keyframes_add(poses[k], c, s)
        sizes = ctx.extract_surrounding_keyframes(1.5, keyframe_params(search_radius=50.0, recent_window=10.0))
        assert sizes[2] >= 2, sizes
        rec = ctx.reg_info(w["corner"], w["surf"], w["pose"][None])[0]
        want, _, mag = model_of(ctx, w, w["pose"], None)
        boxed, _, _ = model_of(ctx, w, w["pose"], (1.0, 1.0, 1.0))
    print("keyframe map: n_rows %s, cropped model %s" % (list(rec["n_rows"]), list(boxed["n_rows"])))
    assert want["n_rows"].sum() > 300 and boxed["n_rows"].sum() < want["n_rows"].sum() // 2
    assert list(rec["n_rows"]) == list(want["n_rows"])
    check(rec, want, mag, "keyframe_map")


# ---- 3. search edges ----
def test_search_edges_keep_the_models_rows():
    """knn_model.lattice_cases(): designed ties (the kept five decided by map index), the d2[4] < 1
    gate from both sides, the crop-box faces, the hole of absent chunks, the map's extent, a query
    beyond 1e7.  n_rows per kind must equal the model's.  tests/test_reg_info_model.py shows on the CPU
    that the model's accepted set is unambiguous on these inputs once the 29 queries of
    info_cases.LATTICE_DROPPED are left out (named there, by case set and index: corner queries whose
    five lattice neighbours give covariance eigenvalues in the exact ratio 3, and one surf query with a
    neighbour 0.2 m from its plane); no case set is dropped."""
    lat, mc, ms = C.lattice_map()
    P = default_params(16, 1800, crop_half=K.CROP_HALF, mapping_corner_leaf_size=K.LEAF_C, mapping_surf_leaf_size=K.LEAF_S)
    names = []
    with api.Context(P) as ctx:
        ctx.set_map(lat, lat)
        gc, gs = ctx.get_map()
        assert np.array_equal(K.xyz_of(gc), mc) and np.array_equal(K.xyz_of(gs), ms)  # the map the CPU check judged
        for c in K.lattice_cases():
            corner, surf = C.lattice_clouds(c)
            rec = ctx.reg_info(corner, surf, c["guess"][None])[0]
            want, _, mag = M.info(mc, ms, K.xyz_of(corner), K.xyz_of(surf), c["guess"], K.CROP_HALF)
            print("%s: n_rows %s of %s queries" % (c["name"], list(rec["n_rows"]), list(rec["n_query"])))
            assert list(rec["n_rows"]) == list(want["n_rows"]), (c["name"], rec["n_rows"], want["n_rows"])
            check(rec, want, mag, "lattice/" + c["name"])
            names.append(c["name"])
    assert len(names) == 15 and {n.rsplit("_", 1)[0] for n in names} >= {"grid", "ties_gate_crop", "holes", "extent_pos", "extent_neg",
                                                                         "shifted_box"}
