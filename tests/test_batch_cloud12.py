"""The batch front end's 12-B cloud records (k_compact -> k_voxel_ring_q / k_features).

A batch launch staged from 16-B scan records keeps its projected cloud as (x, y, z) records when
the four-wave per-ring filter reads it; fbr_diag_batch_cloud forces the float4 cloud, which is what
every launch computed before the narrow format existed.  Every case runs one staged batch both ways
in one context and asserts the poses and every fbr_reg_stats field byte-equal (n_corner, n_surf,
n_corner_ds and n_surf_ds among them), and with whole feature masks the labels of two jobs.  The
float4 run is the reference; the record size each launch took is read back, so neither side of a
comparison is the other format by accident.
"""
import numpy as np
import pytest

import pyoracle as O
from feature_base_pointcloud_registration_amd import api, synth
from feature_base_pointcloud_registration_amd.fbr_types import DESKEW_TABLE, FBR_DESKEW_READY, default_params

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1


def launch(ctx):
    ctx.batch_launch()
    ctx.batch_wait()
    return ctx.batch_results()


def both_formats(P, cmap_smap, scans, guesses, expect_narrow=12, label_jobs=(0, 1)):
    """The staged batch with the float4 cloud forced and on the default, window masks and whole
    masks.  Returns the reference (float4) poses / stats and the whole-mask labels of label_jobs."""
    with api.Context(P) as ctx:
        ctx.set_map(*cmap_smap)
        assert ctx.diag_batch_cloud() == 0  # no launch yet
        ctx.batch_stage(scans, guesses)
        res = {}
        for full in (False, True):
            ctx.batch_set_full_masks(full)
            for wide in (1, 0):
                ctx.diag_batch_cloud(wide)
                p, s = launch(ctx)
                fmt = ctx.diag_batch_cloud()
                assert fmt == (16 if wide else expect_narrow), (full, wide, fmt)
                lab = [ctx.batch_labels(j).copy() for j in label_jobs] if full else None
                res[full, wide] = (p.copy(), s.copy(), lab)
    p_ref, s_ref, _ = res[False, 1]
    for key, (p, s, lab) in res.items():
        assert p.tobytes() == p_ref.tobytes(), key
        for f in s.dtype.names:
            assert np.array_equal(s[f], s_ref[f]), (key, f)
        assert s.tobytes() == s_ref.tobytes(), key
    for a, b in zip(res[True, 1][2], res[True, 0][2]):
        assert len(a) > 0 and np.array_equal(a, b)
    return p_ref, s_ref, res[True, 1][2]


def jobs_of(cfg, n, base_seed):
    jobs = synth.make_jobs(cfg, n, base_seed=base_seed)
    return [j[0] for j in jobs], np.stack([j[1] for j in jobs])


@pytest.fixture(scope="module")
def c1_map():
    return synth.config_map("C1")


@pytest.fixture(scope="module")
def c1_jobs():
    return jobs_of("C1", 24, 5200)


def test_c1_rings_just_above_the_four_wave_threshold(c1_map, c1_jobs):
    """C1, B = 24: 384 rings (the four-wave filter starts above 256), ring lengths no multiple of 64."""
    scans, guesses = c1_jobs
    P = synth.config_params("C1", max_batch=24)
    _, s, labels = both_formats(P, c1_map, scans, guesses)
    assert (s["status"] == 0).all()
    assert (s["n_corner"] > 0).all() and (s["n_surf"] > 0).all() and (s["n_surf_ds"] > 0).all()
    assert all((l == 1).any() and (l == -1).any() for l in labels)


def test_c1_empty_and_thin_rings(c1_map, c1_jobs):
    """One ring of jobs 0 and 1 loses all its raw points and another all but 8: an empty ring
    (end <= start in k_voxel_ring_q), one of fewer than 12 points, and every later row offset of
    the job moves.  The oracle confirms beforehand that both jobs keep enough features to register."""
    scans, guesses = c1_jobs
    scans = list(scans)
    P = synth.config_params("C1", max_batch=24)
    for j, (r_empty, r_thin) in enumerate([(3, 9), (0, 15)]):
        pts = scans[j]
        keep = pts["ring"] != r_empty
        thin = np.flatnonzero(pts["ring"] == r_thin)
        assert (~keep).sum() > 100 and len(thin) > 100
        keep[thin[8:]] = False
        scans[j] = pts[keep].copy()
        f = O.Stream(P).features(scans[j])
        assert len(f["corner"]) > 4 * P.edge_feature_min_valid_num
        assert len(f["surf"]) > 4 * P.surf_feature_min_valid_num
    _, s, _ = both_formats(P, c1_map, scans, guesses)
    assert (s["status"][:2] == 0).all()
    assert (s["n_corner_ds"][:2] > P.edge_feature_min_valid_num).all()
    assert (s["n_surf_ds"][:2] > P.surf_feature_min_valid_num).all()


def test_c2_headline_instances():
    """C2, B = 8: k_voxel_ring_q<8> and k_features<5, 4, 1>, the kernels of the headline batch."""
    scans, guesses = jobs_of("C2", 8, 5300)
    P = synth.config_params("C2", max_batch=8)
    _, s, _ = both_formats(P, synth.config_map("C2"), scans, guesses)
    assert (s["status"] == 0).all()


def test_c1_leaf_overflow_copies_the_candidates(c1_map, c1_jobs):
    """odometry_surf_leaf_size = 0.001 m: a ring's voxel grid has more than 2^31 - 1 cells, PCL's
    "leaf size too small" case, where the filter's output is its input (w = 0).  The condition is
    checked on the host from each ring's bounds: the candidates are the ring's points less its
    corners and their neighbours, so a grid of 64 x 2^31 cells over all the ring's points leaves
    every extent of the candidates' box room to be a quarter of the ring's.  Most rings must meet
    it (a ring that sweeps level ground is one cell high and may not), and the surf count shows the
    copy: most of a scan's points come out."""
    scans, guesses = c1_jobs
    leaf = 0.001
    P = synth.config_params("C1", max_batch=24, odometry_surf_leaf_size=leaf)
    for pts in scans[:4]:
        fires = 0
        for r in range(P.n_scan):
            q = pts[pts["ring"] == r]
            cells = 1 if len(q) else 0
            for k in "xyz":
                cells *= int((float(q[k].max()) - float(q[k].min())) / leaf) + 1 if len(q) else 0
            fires += cells > 64 * INT32_MAX
        assert fires > P.n_scan // 2, fires
    _, s, _ = both_formats(P, c1_map, scans, guesses)
    assert (s["n_surf"] > 0.5 * s["n_points"]).all()


def test_wide_rings_take_the_sixteen_step_instance(c1_map):
    """Rings of 2,049 to 4,096 columns run k_voxel_ring_q<16>.  No synth.CONFIGS entry has such
    rings, so the scans are ray-cast at 16 x 4096; 17 of them make 272 rings, above the threshold."""
    H, W, B = 16, 4096, 17
    scans, guesses = [], []
    for j in range(B):
        gt, guess = synth.job(5400 + j)
        scans.append(synth.scan(gt, H, W, seed=5400 + j))
        guesses.append(guess)
    assert max(np.bincount(s["ring"]).max() for s in scans) > 2048
    P = default_params(H, W, max_batch=B)
    _, s, _ = both_formats(P, c1_map, scans, np.stack(guesses))
    assert (s["n_surf"] > 0).all()


def test_launches_that_keep_float4(c1_map, c1_jobs):
    """A batch with deskew tables (staged as 24-B scans), an exact_voxel_order context and a context
    forced to the 512-thread filter keep the float4 cloud whatever the switch says, and compute the
    same on either setting."""
    scans, guesses = c1_jobs

    def run(P, tables=None, ring_filter=None):
        with api.Context(P) as ctx:
            ctx.set_map(*c1_map)
            if ring_filter is not None:
                ctx.diag_ring_filter(ring_filter)
            if tables is not None:
                ctx.set_deskew(tables)
            ctx.batch_stage(scans, guesses)
            out = []
            for wide in (1, 0):
                ctx.diag_batch_cloud(wide)
                p, s = launch(ctx)
                assert ctx.diag_batch_cloud() == 16
                out.append((p.copy(), s.copy()))
        assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
        return out[0]

    q = synth.imu_queue(41.0 - 0.05, 41.0 + 0.16, rate=200.0, gyro=(0.02, 0.03, 0.6), seed=0)
    table, _ = api.imu_deskew_info(q, 41.0, 41.1)
    assert table["status"] == FBR_DESKEW_READY and table["imu_available"] == 1
    tabs = np.zeros(len(scans), DESKEW_TABLE)
    tabs[0] = table
    run(synth.config_params("C1", max_batch=24), tables=tabs)
    run(synth.config_params("C1", max_batch=24, exact_voxel_order=1))
    run(synth.config_params("C1", max_batch=24), ring_filter=0)
