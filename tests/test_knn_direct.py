"""The Gauss-Newton 5-NN search per query against the float32 brute force of tests/knn_model.py.

Every other kNN test compares poses at the end of a registration; here every query's five map
indices, read back from the device (fbr_diag_knn_last), must equal brute_knn5's in order, on the
inputs where a grid search goes wrong (tests/knn_model.py: cell faces, exact ties, the d2 < 1 gate,
the crop planes, the grid's extent, absent chunks) and on a structured world and a realistic scan
whose later passes run warm-started.  The ground truth is built from ctx.get_map() (map-index order)
and the query positions the pass itself computed.

The kernel variants are chosen by environment knobs read once per process, so each variant runs in
one child process (this file run as a script), which writes what it read back to an .npz; the
parent compares, and asserts from the launch descriptor that the variant it meant to test ran.
"""
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
from feature_base_pointcloud_registration_amd.fbr_types import default_params  # noqa: E402

FBR_ERR_STATE = -7
DESC = ("iterations", "r", "rx", "flat", "sparse", "lpq", "fused", "tiles")


# ------------------------------------------------------------------------------------ the child
def _params(max_iterations, leaf=None, cfg=None):
    if cfg is not None:
        from feature_base_pointcloud_registration_amd import synth
        return synth.config_params(cfg, max_iterations=max_iterations)
    kw = {} if leaf is None else dict(mapping_corner_leaf_size=leaf, mapping_surf_leaf_size=leaf)
    return default_params(16, 1800, crop_half=K.CROP_HALF, max_iterations=max_iterations, **kw)


def child(in_path, out_path):
    from feature_base_pointcloud_registration_amd import api
    d = np.load(in_path)
    out = {}

    def run(ctx, name, corner, surf, guess):
        pose, st, trace = ctx.register(corner, surf, guess, trace=True)
        k = ctx.diag_knn_last()
        assert (k["n_corner"], k["n_surf"]) == (st["n_corner_ds"], st["n_surf_ds"]), (name, k["n_corner"], st)
        assert k["desc"]["iterations"] == st["iterations"], (name, k["desc"], st)
        out[name + "/q"], out[name + "/nbr"] = k["queries"], k["nbr"]
        out[name + "/nc"] = np.int32(k["n_corner"])
        out[name + "/desc"] = np.array([k["desc"][f] for f in DESC], np.int32)
        out[name + "/trace"] = trace
        out[name + "/status"] = np.int32(st["status"])
        return st, trace

    def prev_pose(guess, st, trace):  # the pose the last pass ran at
        return np.asarray(guess if st["iterations"] < 2 else trace[st["iterations"] - 2], np.float32)

    names = [str(n) for n in d["case_names"]]
    with api.Context(_params(1)) as ctx:
        try:
            ctx.diag_knn_last()
            out["state_error"] = np.int32(0)
        except api.FbrError as e:
            out["state_error"] = np.int32(e.status)
        ctx.set_map(d["lattice"], d["lattice"])
        out["lattice/map_c"], out["lattice/map_s"] = ctx.get_map()
        for n in names:
            run(ctx, "case/" + n, d["case/%s/corner" % n], d["case/%s/surf" % n], d["case/%s/guess" % n])
    for tag, leaf, cfg in (("struct", None, None), ("cluster", float(d["cluster/leaf"]), None), ("c1", None, "C1")):
        with api.Context(_params(3, leaf, cfg)) as ctx:
            ctx.set_map(d[tag + "/map_c"], d[tag + "/map_s"])
            out[tag + "/map_c"], out[tag + "/map_s"] = ctx.get_map()
            st, trace = run(ctx, tag + "/warm", d[tag + "/corner"], d[tag + "/surf"], d[tag + "/guess"])
            prev = prev_pose(d[tag + "/guess"], st, trace)
        # the same queries through the iteration-0 kernel: a fresh context, one iteration from the
        # pose the warm-started last pass ran at
        with api.Context(_params(1, leaf, cfg)) as ctx:
            ctx.set_map(d[tag + "/map_c"], d[tag + "/map_s"])
            run(ctx, tag + "/cold", d[tag + "/corner"], d[tag + "/surf"], prev)
            out[tag + "/prev"] = prev
    ts = api.knn_tile_stats()
    out["tile_stats"] = np.array(ts if ts is not None else [0] * 8, np.int64)
    np.savez(out_path, **out)


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2])
    sys.exit(0)


# ------------------------------------------------------------------------------------ the parent
pytestmark = pytest.mark.gpu

# name -> (environment, descriptor of the iteration-0 pass, of a warm-started pass) on the 0.4 m-leaf
# maps (1 m y/z cells, 0.25 m x cells unless the variant says otherwise).  None: do not care.
_D = dict(r=1, rx=4, flat=0, sparse=0, lpq=8, fused=0, tiles=0)
VARIANTS = {
    "default_wide": ({}, _D, _D),
    "lpq1": ({"FBR_KNN_LPQ": "1"}, dict(_D, lpq=1), dict(_D, lpq=1, flat=1)),
    "lpq1_per_row": ({"FBR_KNN_LPQ": "1", "FBR_KNN_FLAT": "0"}, dict(_D, lpq=1), dict(_D, lpq=1)),
    "cell_0.5": ({"FBR_KNN_CELL": "0.5"}, dict(_D, r=2), dict(_D, r=2)),
    "cell_0.25": ({"FBR_KNN_CELL": "0.25"}, dict(_D, r=4), dict(_D, r=4)),
    "cell_x_1": ({"FBR_KNN_CELL_X": "1"}, dict(_D, rx=1), dict(_D, rx=1)),
    "cell_x_0.125": ({"FBR_KNN_CELL_X": "0.125"}, dict(_D, rx=8), dict(_D, rx=8)),
    "sparse_1m": ({"FBR_GRID_SPARSE": "1"}, dict(_D, sparse=1), dict(_D, sparse=1)),
    "sparse_0.5m": ({"FBR_GRID_SPARSE": "1", "FBR_KNN_CELL": "0.5"}, dict(_D, r=2, sparse=1), dict(_D, r=2, sparse=1)),
    "sparse_lpq1": ({"FBR_GRID_SPARSE": "1", "FBR_KNN_LPQ": "1"}, dict(_D, sparse=1, lpq=1),
                    dict(_D, sparse=1, lpq=1, flat=1)),
    "lpq1_cell_0.5": ({"FBR_KNN_LPQ": "1", "FBR_KNN_CELL": "0.5"}, dict(_D, r=2, lpq=1), dict(_D, r=2, lpq=1)),
    "fused_tail": ({"FBR_GN_TAIL": "1"}, dict(_D, lpq=1, fused=1), dict(_D, lpq=1, fused=1)),
    "tiles": ({"FBR_KNN_TILE": "1", "FBR_KNN_TILE_STATS": "1", "FBR_KNN_CELL": "0.5", "FBR_KNN_CELL_X": "0.125"},
              dict(_D, r=2, rx=8), dict(_D, r=2, rx=8, lpq=1, tiles=1)),
}
KNOBS = ("FBR_KNN_LPQ", "FBR_KNN_FLAT", "FBR_KNN_CELL", "FBR_KNN_CELL_X", "FBR_GRID_SPARSE", "FBR_GN_TAIL", "FBR_KNN_TILE",
         "FBR_KNN_TILE_STATS", "FBR_GN_LAG", "FBR_FIT_CACHE")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """Everything the children register, written once; the C1 features come from the oracle."""
    import pyoracle as O
    from feature_base_pointcloud_registration_amd import synth
    cases = K.lattice_cases()
    d = {"lattice": K.cloud(K.lattice_points()), "case_names": np.array([c["name"] for c in cases])}
    for c in cases:
        for f in ("corner", "surf", "guess"):
            d["case/%s/%s" % (c["name"], f)] = c[f]
    s, cl = K.structured_case(), K.dense_cluster_case()
    P = synth.config_params("C1")
    gt, guess = synth.job(1)
    feat = O.Stream(P).features(synth.scan(gt, 16, 1800, seed=1))
    cmap, smap = synth.config_map("C1")
    c1 = dict(corner_map=cmap, surf_map=smap, corner=feat["corner"], surf=feat["surf"], guess=np.asarray(guess, np.float32))
    for tag, j in (("struct", s), ("cluster", cl), ("c1", c1)):
        d[tag + "/map_c"], d[tag + "/map_s"] = j["corner_map"], j["surf_map"]
        d[tag + "/corner"], d[tag + "/surf"], d[tag + "/guess"] = j["corner"], j["surf"], j["guess"]
    d["cluster/leaf"] = np.float32(cl["leaf"])
    path = str(tmp_path_factory.mktemp("knn_direct") / "inputs.npz")
    np.savez(path, **d)
    return dict(path=path, cases=cases, struct=s, cluster=cl, c1=c1, c1_params=P)


_BRUTE = {}


def brute(map_xyz, q, box, near=False):
    """brute_knn5, computed once per (map, queries, box): the variants share the reference."""
    key = (map_xyz.tobytes(), q.tobytes(), box[0].tobytes(), box[1].tobytes())
    if key not in _BRUTE:
        _BRUTE[key] = (K.brute_knn5_near if near else K.brute_knn5)(map_xyz, q, *box)
    return _BRUTE[key]


def check_run(r, name, maps, box, near=False):
    """Every query of run `name` against the brute force on its own map (corner queries first)."""
    q, nbr, nc = r[name + "/q"], r[name + "/nbr"], int(r[name + "/nc"])
    for kind, sl, m in (("corner", slice(0, nc), maps[0]), ("surf", slice(nc, None), maps[1])):
        want = brute(K.xyz_of(m), q[sl], box, near)
        bad = np.flatnonzero((nbr[sl] != want).any(1))
        assert len(bad) == 0, (name, kind, len(bad), q[sl][bad[:4]], nbr[sl][bad[:4]], want[bad[:4]])
    return q, nbr, nc


def assert_desc(r, name, want, iterations=None):
    got = dict(zip(DESC, (int(v) for v in r[name + "/desc"])))
    if iterations is not None:
        assert got["iterations"] == iterations, (name, got)
    assert {k: got[k] for k in want} == want, (name, got)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_query_has_the_brute_force_neighbours(variant, inputs, tmp_path):
    env_set, cold, warm = VARIANTS[variant]
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(env_set)
    out = str(tmp_path / "out.npz")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), inputs["path"], out], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    r = np.load(out)
    assert int(r["state_error"]) == FBR_ERR_STATE  # no registration yet on that context

    # ---- the lattice case sets: one iteration, the iteration-0 kernel ----
    lat = K.lattice_points()
    mc, ms = r["lattice/map_c"], r["lattice/map_s"]
    for m in (mc, ms):  # one point per voxel: the start-up filter kept every point as it is
        assert len(m) == len(lat) and np.array_equal(np.unique(K.xyz_of(m), axis=0), np.unique(lat, axis=0))
    n_q = n_rej = 0
    for c in inputs["cases"]:
        name = "case/" + c["name"]
        assert_desc(r, name, cold, iterations=1)
        q, nbr, nc = check_run(r, name, (mc, ms), K.crop_box(c["guess"]))
        # the queries are the scan's points bit for bit (fl(p + t); the scan-side filter kept each)
        for sl, scan in ((slice(0, nc), c["corner"]), (slice(nc, None), c["surf"])):
            want = K.xyz_of(scan) + c["guess"][3:]
            assert len(q[sl]) == len(want), (name, len(q[sl]), len(want))
            assert np.array_equal(np.unique(q[sl], axis=0), np.unique(want, axis=0)), name
        n_q += len(q)
        n_rej += int((nbr[:, 0] < 0).sum())
    # every designed query reached the search in one of its family's sets
    for fam in ("grid", "ties_gate_crop", "holes", "extent_pos", "extent_neg", "shifted_box"):
        sets = [c for c in inputs["cases"] if c["name"].rsplit("_", 1)[0] == fam]
        allq = np.vstack([r["case/%s/q" % c["name"]] for c in sets])
        keys = {row.tobytes() for row in allq}
        missing = [dq for dq in sets[0]["designed"] if dq.tobytes() not in keys]
        assert not missing, (fam, missing[:5])
    assert n_q > 4000 and 0.05 * n_q < n_rej < 0.8 * n_q
    far = r["case/far/nbr"][np.abs(r["case/far/q"]).max(1) > 1e7]
    assert len(far) == 3 and (far == -1).all()

    # ---- structure, the dense cluster and the C1 scan: three iterations, warm-started passes ----
    P1 = inputs["c1_params"]
    for tag, half, near in (("struct", K.CROP_HALF, False), ("cluster", K.CROP_HALF, False), ("c1", list(P1.crop_half), True)):
        j = inputs[tag]
        maps = (r[tag + "/map_c"], r[tag + "/map_s"])
        wdesc = dict(zip(DESC, (int(v) for v in r[tag + "/warm/desc"])))
        assert int(r[tag + "/warm/status"]) == 0 and wdesc["iterations"] >= (2 if tag == "cluster" else 3), (tag, wdesc)
        want_w, want_c = dict(warm), dict(cold)
        if tag == "cluster":  # leaves below 0.3 m: 0.5 m / 0.125 m cells unless the variant sets them
            for w in (want_w, want_c):
                w["r"] = w["r"] if "FBR_KNN_CELL" in env_set else 2
                w["rx"] = w["rx"] if "FBR_KNN_CELL_X" in env_set else 8
                w["flat"] = w["flat"] if w["r"] == 1 else 0  # the flat row queue is the 1 m cells'
        assert_desc(r, tag + "/warm", want_w)
        assert_desc(r, tag + "/cold", want_c, iterations=1)
        qw, nw, nc = check_run(r, tag + "/warm", maps, K.crop_box(j["guess"], half), near)
        prev = r[tag + "/prev"]
        qc, ncold, nc2 = check_run(r, tag + "/cold", maps, K.crop_box(prev, half), near)
        # the warm-started kernel against the cold one on identical queries (the boxes differ by the
        # guesses' offset: compare where the brute force says the box makes no difference)
        assert nc == nc2 and np.array_equal(qw.view(np.uint32), qc.view(np.uint32)), tag
        same = np.ones(len(qw), bool)
        for sl, m in ((slice(0, nc), maps[0]), (slice(nc, None), maps[1])):
            same[sl] = (brute(K.xyz_of(m), qw[sl], K.crop_box(j["guess"], half), near) ==
                        brute(K.xyz_of(m), qc[sl], K.crop_box(prev, half), near)).all(1)
        assert same.mean() > 0.9 and np.array_equal(nw[same], ncold[same]), tag
        assert (nw[:, 0] >= 0).mean() > 0.5, tag
    # ---- the returned positions are the traced pose's: T p within the float32 error of three
    # products, three sums and T's rounded entries, 16 * 2^-24 * (|px| + |py| + |pz| + |t_k|); a
    # stale pose is off by the step size (centimetres) ----
    s = inputs["struct"]
    it = int(r["struct/warm/desc"][0])
    prev = r["struct/prev"]
    assert np.array_equal(prev, r["struct/warm/trace"][it - 2]) and np.abs(prev - s["guess"]).max() > 0.01
    T = K.pose_matrix64(prev)
    p = np.vstack([K.xyz_of(s["corner"]), K.xyz_of(s["surf"])]).astype(np.float64)
    ref = p @ T[:, :3].T + T[:, 3]
    bound = 16 * 2.0 ** -24 * (np.abs(p).sum(1)[:, None] + np.abs(T[:, 3])[None, :])
    q = r["struct/warm/q"].astype(np.float64)
    assert len(q) == len(ref)
    d2 = ((q[:, None, :] - ref[None, :, :]) ** 2).sum(2)
    match = d2.argmin(1)
    assert len(np.unique(match)) == len(q)  # a bijection onto the scan's points
    assert (np.abs(q - ref[match]) <= bound[match]).all(), np.abs(q - ref[match]).max()

    if variant == "tiles":
        ts = r["tile_stats"]
        queries, binned, tiles, over = int(ts[0]), int(ts[1]), int(ts[2]), int(ts[5])
        assert queries > 0 and binned > 0 and tiles > 0 and over > 0, ts
    if variant == "default_wide":
        assert len(VARIANTS) >= 11
