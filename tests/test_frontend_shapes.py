"""The scan front end (k_project, k_rowcount, k_compact, k_features, k_voxel_ring*) against the
oracle over the sensor shapes at which the kernels pick another template instance, tile geometry
or loop shape.  CASES names the branch each (N_SCAN, Horizon_SCAN) is there for; the CPU tests
check, from the oracle and from the host's own selection formulas restated here, that every case
has the shape it is meant to have.

Bars are test_gpu_parity's: projection, labels and corner clouds bit-exact; surf clouds within
SURF_ULPS in the default order and bytes equal with exact_voxel_order = 1.  Environment knobs are
read once per process, so the other instances run in child processes, one at a time.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import proj_model as M
import pyoracle as O
from conftest import REPO
from feature_base_pointcloud_registration_amd import api, synth
from feature_base_pointcloud_registration_amd.fbr_types import DESKEW_TABLE, default_params
from test_compact_model import compact_nchunk, compact_tile
from test_gpu_parity import assert_features_equal, assert_projection_equal, bits

HERE = os.path.dirname(os.path.abspath(__file__))

# (H, W): what the shape reaches
CASES = {
    (1, 1800): "H - 1 = 0 in k_features' grid decode; k_compact tile 1 x 256, the CG > 64 rank combine",
    (2, 300): "k_compact tile 2 x 256: one full and one ragged chunk",
    (4, 900): "k_compact tile 4 x 128",
    (6, 4000): "Livox: W % 64 = 32; k_features<12, 8, *>; ring filter KPT 8 / k_voxel_ring_q<16>",
    (16, 512): "ring filter KPT 2",
    (32, 1024): "ring filter KPT 2, its upper border",
    (16, 1025): "ring filter KPT 4, its lower border",
    (40, 1800): "row blocks 16 + 16 + 8",
    (65, 200): "row blocks 4 x 16 + 1; W < 256",
    (16, 1877): "k_features<5, 4, 1>'s last W (one wave per ring)",
    (16, 1878): "k_features<6, 4, 1>'s first W (one wave per ring)",
    (16, 2049): "ring filter KPT 8 / k_voxel_ring_q<16>, the lower border",
    (16, 2261): "k_features<6, 4, *>'s last W",
    (16, 2262): "k_features<12, 8, *>'s first W",
    (16, 4096): "kMaxW",
    (256, 1024): "k_project's LDS tile of 32 columns",
}
SHAPES = list(CASES)
INSTANCE_SHAPES = [(16, 1877), (16, 1878), (16, 2261), (16, 2262), (6, 4000), (16, 4096)]
RING_FILTER_SHAPES = [(32, 1024), (40, 1800), (6, 4000)]  # one per W class: <= 1024, <= 2048, above
BATCH_SHAPES = [(1, 1800), (6, 4000), (40, 1800), (16, 2262)]
COMPACT_SHAPES = [(4, 900), (16, 1800), (40, 1800), (64, 1800)]
BATCH_B = 9  # a full job group of 8 and a partial one
BATCH_CUTS = [0, 1, 7, 15, 100, None, 1000, 33, 5000]  # points cut from each job's scan; None: empty


def ids(shapes):
    return ["%dx%d" % s for s in shapes]


# ------------------------------------------------------------------------------- the selections
def feature_instance(W, nwv):
    """launch_features (k_features.hip): the template instance <WMAX, KWORDS, waves> for a launch at
    nwv waves per ring, from fbr_feat_layout.h's caps_of: segcap = W / 6 + 8, kseg the next power of
    two >= segcap - 1."""
    segcap, kseg = W // 6 + 8, 1
    while kseg < segcap - 1:
        kseg <<= 1
    if nwv == 1 and segcap <= 5 * 64 and kseg <= 4 * 128:
        return (5, 4, 1)
    if segcap <= 6 * 64 and kseg <= 4 * 128:
        return (6, 4, nwv)
    return (12, 8, 4 if nwv > 1 else 1)


def ring_filter_kpt(W):
    """launch_voxel_ring: points per thread of the 512-thread kernel's instance."""
    kpt = (W + 511) // 512
    return 2 if kpt <= 2 else 4 if kpt <= 4 else 8


def ring_filter_q(W):
    """launch_voxel_ring: the four-wave kernel's instance."""
    return 8 if W <= 4 * 64 * 8 else 16


def row_blocks(H, cells=512):
    hb, _ = compact_tile(H, cells)
    return [min(hb, H - r) for r in range(0, H, hb)]


# ------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def case_scans(H, W):
    """Two scans of the shape, a few metres apart.  A one-ring sensor takes a wall-level ring of a
    16-ring scan (the generator's own single ring looks at the ground: no corner)."""
    out = []
    for seed in (5, 15):
        gt, _ = synth.job(seed)
        if H == 1:
            pts = synth.scan(gt, 16, W, seed=seed)
            pts = pts[pts["ring"] == 9].copy()
            pts["ring"] = 0
        else:
            pts = synth.scan(gt, H, W, seed=seed)
        out.append(pts)
    return out


@functools.lru_cache(maxsize=None)
def oracle_stream(H, W):
    """[(projection, features)] of case_scans(H, W) as a stream: the second scan starts from the
    first one's FeatureExtraction state."""
    P = default_params(H, W)
    st = O.Stream(P)
    return [(O.project(P, pts), st.features(pts)) for pts in case_scans(H, W)]


@functools.lru_cache(maxsize=None)
def case_table():
    """An IMU deskew table whose window covers the scans' point times."""
    q = synth.imu_queue(19.95, 20.16, gyro=(0.08, -0.05, 0.9), seed=3)
    t, _ = api.imu_deskew_info(q, 20.0, 20.1)
    assert t["imu_available"] == 1
    return t


@functools.lru_cache(maxsize=None)
def small_map():
    return synth.prior_map(25.0, 3.0, 3.0)


@functools.lru_cache(maxsize=None)
def batch_jobs(H, W):
    """BATCH_B (scan, guess) jobs with ragged point counts and one empty scan."""
    jobs = []
    for j, cut in enumerate(BATCH_CUTS):
        gt, guess = synth.job(40 + j)
        if H == 1:
            pts = synth.scan(gt, 16, W, seed=40 + j)
            pts = pts[pts["ring"] == 9].copy()
            pts["ring"] = 0
        else:
            pts = synth.scan(gt, H, W, seed=40 + j)
        pts = pts[:0] if cut is None else pts[:max(len(pts) - cut, 1)]
        jobs.append((np.ascontiguousarray(pts), guess))
    return jobs


# ------------------------------------------------------------------------------- conditions (CPU)
def test_cases_select_the_instances_they_name():
    segcap = lambda W: W // 6 + 8  # noqa: E731
    assert (segcap(1877), segcap(1878), segcap(2261), segcap(2262)) == (320, 321, 384, 385)
    assert feature_instance(1877, 1) == (5, 4, 1) and feature_instance(1878, 1) == (6, 4, 1)
    assert feature_instance(1877, 4) == (6, 4, 4) and feature_instance(1877, 2) == (6, 4, 2)
    assert feature_instance(2261, 4) == (6, 4, 4) and feature_instance(2262, 4) == (12, 8, 4)
    assert feature_instance(2261, 1) == (6, 4, 1) and feature_instance(2262, 1) == (12, 8, 1)
    assert feature_instance(2261, 2) == (6, 4, 2) and feature_instance(2262, 2) == (12, 8, 4)
    for W in (4000, 4096):
        assert feature_instance(W, 4) == (12, 8, 4) and feature_instance(W, 1) == (12, 8, 1)
    for H, W in SHAPES:  # every other shape of the matrix takes the six-word instance by default
        if W < 2262:
            assert feature_instance(W, 4) == (6, 4, 4)
    assert [ring_filter_kpt(W) for W in (512, 1024, 1025, 2048, 2049, 4000, 4096)] == [2, 2, 4, 4, 8, 8, 8]
    assert [ring_filter_q(W) for W in (1024, 2048, 2049, 4000)] == [8, 8, 16, 16]
    assert [ring_filter_kpt(W) for _, W in RING_FILTER_SHAPES] == [2, 4, 8]
    assert compact_tile(1, 512) == (1, 256) and compact_nchunk(256, 1800) == 8 and 1800 % 256 != 0
    assert compact_tile(2, 512) == (2, 256) and compact_nchunk(256, 300) == 2
    assert compact_tile(4, 512) == (4, 128)
    assert row_blocks(40) == [16, 16, 8] and row_blocks(65) == [16, 16, 16, 16, 1]
    assert 4000 % 64 == 32
    assert M.project_tile_cols(256) == 32 and all(M.project_tile_cols(H) == 64 for H, _ in SHAPES if H <= 128)
    # FBR_COMPACT_CELLS: tiles above 512 cells (the i = tid + 512 loops), CG > 64, ragged row blocks
    tiles = {(H, c): compact_tile(H, c) for H, _ in COMPACT_SHAPES for c in (1024, 2048)}
    assert tiles[(4, 1024)] == (4, 256) and tiles[(4, 2048)] == (4, 256)
    assert tiles[(16, 1024)] == (16, 64) and tiles[(16, 2048)] == (16, 128)
    assert tiles[(40, 1024)] == (32, 32) and tiles[(40, 2048)] == (40, 32)
    assert tiles[(64, 1024)] == (32, 32) and tiles[(64, 2048)] == (64, 32)
    assert row_blocks(40, 1024) == [32, 8]
    assert all(hb * cg > 512 for hb, cg in tiles.values())


@pytest.mark.parametrize("H,W", SHAPES, ids=ids(SHAPES))
def test_cases_are_not_degenerate(H, W):
    """Every case's oracle result has corners, picked surf points and a surf cloud, and no empty
    ring, in both scans of the stream."""
    scans = case_scans(H, W)
    for pts, (pr, f) in zip(scans, oracle_stream(H, W)):
        assert len(pts) <= H * W
        assert (f["label"] == 1).sum() > 0 and (f["label"] == -1).sum() > 0 and len(f["surf"]) > 0
        assert len(f["corner"]) > 0
        cnt = pr["end_ring"] - pr["start_ring"] + 10  # :650, :668
        assert cnt.sum() == len(pr["col_ind"]) == f["n_points"]
        assert (cnt > 0).all()
    assert not np.array_equal(scans[0]["x"][:100], scans[1]["x"][:100])


@pytest.mark.parametrize("H,W", BATCH_SHAPES, ids=ids(BATCH_SHAPES))
def test_batch_jobs_are_ragged_with_one_empty_scan(H, W):
    jobs = batch_jobs(H, W)
    lens = [len(p) for p, _ in jobs]
    assert len(jobs) == BATCH_B and lens.count(0) == 1 and len(set(lens)) >= BATCH_B - 1
    assert len({n % 16 for n in lens}) >= 5 and max(lens) <= H * W
    P = default_params(H, W)
    some = O.Stream(P).features(jobs[0][0])
    assert (some["label"] == 1).sum() > 0 and (some["label"] == -1).sum() > 0


# ------------------------------------------------------------------------------- stream (GPU)
INSTANCE_CODE = {5: 1, 6: 2, 12: 3}  # bits 30..31 of a ring's path word (FeatArgs::paths): the instance's WMAX


def stream_results(H, W, **params):
    """[(projection, features)] of case_scans(H, W) through one context, and the set of k_features
    instances its rings ran in (codes of the path record, fbr_diag_feature_paths)."""
    out = []
    with api.Context(default_params(H, W, **params)) as ctx:
        ctx.feature_paths()  # arm the record
        for pts in case_scans(H, W):
            pr = ctx.project(pts)
            out.append((pr, ctx.extract_features(len(pr["col_ind"]))))
        words = ctx.feature_paths()
    return out, {int(w) >> 30 for w in words.ravel() if w}


def result_bytes(res):
    out = b""
    for pr, f in res:
        out += b"".join(bits(pr[k]).tobytes() for k in ["start_ring", "end_ring", "col_ind", "range", "cloud"])
        out += f["label"].tobytes() + f["corner"].tobytes() + f["surf"].tobytes()
    return out


def stream_bytes(H, W):
    """Children: the result bytes, then one byte per instance code that ran."""
    res, codes = stream_results(H, W)
    return result_bytes(res) + bytes(sorted(codes))


def assert_stream_matches_oracle(H, W, res):
    for (po, fo), (pg, fg) in zip(oracle_stream(H, W), res):
        assert_projection_equal(po, pg)
        assert_features_equal(fo, fg)


def in_child(expr, env):
    """stdout bytes of `sys.stdout.buffer.write(<expr>)` with this module imported as T, in a child
    process with extra environment knobs."""
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import test_frontend_shapes as T; "
            "sys.stdout.buffer.write(%s)" % (REPO, os.path.join(REPO, "oracle"), HERE, expr))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=120, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SHAPES, ids=ids(SHAPES))
def test_stream_matches_oracle(H, W):
    res, codes = stream_results(H, W)
    assert codes == {INSTANCE_CODE[feature_instance(W, 4)[0]]}  # the instance CASES names, on every ring
    assert_stream_matches_oracle(H, W, res)
    # PCL's in-voxel point order: the surf cloud's bytes too
    for (po, fo), (pg, fg) in zip(oracle_stream(H, W), stream_results(H, W, exact_voxel_order=1)[0]):
        assert_projection_equal(po, pg)
        assert np.array_equal(fo["label"], fg["label"])
        assert np.array_equal(bits(fo["corner"]), bits(fg["corner"]))
        assert np.array_equal(bits(fo["surf"]), bits(fg["surf"]))


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 2])
@pytest.mark.parametrize("H,W", INSTANCE_SHAPES, ids=ids(INSTANCE_SHAPES))
def test_feature_instances_give_the_same_bytes(H, W, waves):
    """k_features at one and two waves per ring (FBR_FEAT_WAVES, child process) runs the instance
    launch_features is meant to pick and returns this process's bytes (four waves per ring), which
    match the oracle."""
    here, _ = stream_results(H, W)
    assert_stream_matches_oracle(H, W, here)
    got = in_child("T.stream_bytes(%d, %d)" % (H, W), {"FBR_FEAT_WAVES": str(waves)})
    assert got[-1:] == bytes([INSTANCE_CODE[feature_instance(W, waves)[0]]])
    assert got[:-1] == result_bytes(here)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [0, 2])
@pytest.mark.parametrize("H,W", RING_FILTER_SHAPES, ids=ids(RING_FILTER_SHAPES))
def test_ring_filter_kernels_match_oracle(H, W, kernel):
    """The 512-thread per-ring surf filter (0) and the four-wave one (2), each forced."""
    st = oracle_stream(H, W)
    with api.Context(default_params(H, W)) as ctx:
        ctx.diag_ring_filter(kernel)
        for pts, (po, fo) in zip(case_scans(H, W), st):
            assert_features_equal(fo, ctx.features(pts))


# ------------------------------------------------------------------------------- batch (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("H,W", BATCH_SHAPES, ids=ids(BATCH_SHAPES))
def test_batch_labels_and_counts_match_oracle(H, W):
    """16-B packed scan records, k_compact<false, true[, true]> and the deal of tiles to XCDs: nine
    staged jobs (a full group of eight and a partial one), ragged and one empty."""
    jobs = batch_jobs(H, W)
    scans, guesses = [j[0] for j in jobs], np.stack([j[1] for j in jobs])
    P = default_params(H, W, max_batch=BATCH_B)
    cmap, smap = small_map()
    with api.Context(P) as ctx:
        ctx.set_map(cmap, smap)
        ctx.batch_stage(scans, guesses)
        ctx.batch_set_full_masks(True)
        ctx.batch_launch()
        ctx.batch_wait()
        _, stats = ctx.batch_results()
        labels = [ctx.batch_labels(j) for j in range(BATCH_B)]
    for j, pts in enumerate(scans):
        f = O.Stream(P).features(pts)
        assert stats["n_points"][j] == f["n_points"], j
        assert len(labels[j]) == f["n_points"] and np.array_equal(labels[j], f["label"]), j
        assert (stats["n_corner"][j], stats["n_surf"][j]) == (len(f["corner"]), len(f["surf"])), j


# ------------------------------------------------------------------------------- compaction tiles (GPU)
def projection_bytes(H, W):
    """fbr_project of the case's first scan without and with a deskew table."""
    pts = case_scans(H, W)[0]
    out = b""
    with api.Context(default_params(H, W)) as ctx:
        for tab in (None, [case_table()]):
            ctx.set_deskew(tab)
            pr = ctx.project(pts)
            out += b"".join(bits(pr[k]).tobytes() for k in ["start_ring", "end_ring", "col_ind", "range", "cloud"])
    return out


def oracle_projection_bytes(H, W):
    P = default_params(H, W)
    pts = case_scans(H, W)[0]
    out = b""
    for tab in (None, case_table()):
        pr = O.project(P, pts, deskew=tab)
        out += b"".join(bits(pr[k]).tobytes() for k in ["start_ring", "end_ring", "col_ind", "range", "cloud"])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cells", [1024, 2048])
@pytest.mark.parametrize("H,W", COMPACT_SHAPES, ids=ids(COMPACT_SHAPES))
def test_compaction_tile_sizes_give_the_same_bytes(H, W, cells):
    """k_compact with tiles of 1024 and 2048 cells (FBR_COMPACT_CELLS, child process), plain and
    deskewing (the deskew instance has its own LDS layout): the default's bytes and the oracle's."""
    ref = oracle_projection_bytes(H, W)
    assert projection_bytes(H, W) == ref
    assert in_child("T.projection_bytes(%d, %d)" % (H, W), {"FBR_COMPACT_CELLS": str(cells)}) == ref


def test_deskew_table_moves_the_compaction_cases():
    """The deskewed half of the compaction cases differs from the plain half (CPU: the oracle)."""
    for H, W in COMPACT_SHAPES:
        b = oracle_projection_bytes(H, W)
        assert b[:len(b) // 2] != b[len(b) // 2:]
    assert np.array(case_table(), DESKEW_TABLE)["imu_pointer_cur"] > 10
