"""Size classes of the batch mapping DS (downsampleCurrentScan, `voxel_scan`): the surf set keeps
the 1024 x 18 in-place instance of k_voxel_grid_ip and the corner set gets a launch of its own with
a 256 x 16 instance (LDS capacity Lc = 4096 points, four workgroups per CU).  The sort is stable for
any workgroup size and chunk length and the emit sums a voxel's points in sorted order, so every
instance must give the bytes of the global-scratch kernel (FBR_VG_INPLACE=0)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pyoracle as O
from conftest import REPO
from feature_base_pointcloud_registration_amd import api, synth
from feature_base_pointcloud_registration_amd.fbr_types import POINT_XYZI, REG_STATS, REG_STATS_FIELDS

pytestmark = pytest.mark.gpu

SMALL_T, SMALL_KPL = 256, 16
LC = SMALL_T * SMALL_KPL          # LDS capacity of the corner instance
LS = 1024 * 18                    # ... of the surf instance
TMP = os.environ.get("TMPDIR", "/tmp")


def _child(code, env):
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, env=dict(os.environ, **env), timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


# ------------------------------------------------------------------ batch poses and statistics
_BATCH_CODE = (
    "import sys, numpy as np; sys.path.insert(0, %r); from feature_base_pointcloud_registration_amd import api, synth\n"
    "d = np.load(%r); scans = [d['arr_%%d' %% k] for k in range(%d)]; m = synth.config_map(%r)\n"
    "for ex in (0, 1):\n"
    "    with api.Context(synth.config_params(%r, max_batch=%d, exact_voxel_order=ex)) as c:\n"
    "        c.set_map(*m); p, s = c.process_batch(scans, d['guesses'])\n"
    "    sys.stdout.buffer.write(p.tobytes() + s.tobytes())\n")


@pytest.mark.parametrize("cfg,n", [("C2", 6), ("C3", 2)])
def test_batch_poses_and_stats_match_global_scratch_kernel(cfg, n):
    """A batch of n jobs (one sub-batch: a two-set launch of 2 n segments, above the split kernel's
    limit) in the default mode and with exact_voxel_order = 1: poses and every statistics field
    byte for byte against a child process on the global-scratch kernel."""
    jobs = synth.make_jobs(cfg, n, base_seed=5200)
    scans, guesses = [j[0] for j in jobs], np.stack([j[1] for j in jobs]).astype(np.float32)
    path = os.path.join(TMP, "fbr_vg_classes_%s.npz" % cfg)
    np.savez(path, *scans, guesses=guesses)
    ref = _child(_BATCH_CODE % (REPO, path, n, cfg, cfg, n), {"FBR_VG_INPLACE": "0"})
    rec = n * 24 + n * REG_STATS.itemsize
    assert len(ref) == 2 * rec
    m = synth.config_map(cfg)
    for ex in (0, 1):
        with api.Context(synth.config_params(cfg, max_batch=n, exact_voxel_order=ex)) as c:
            c.set_map(*m)
            p, s = c.process_batch(scans, guesses)
        assert (s["status"] == 0).all()
        # the corner clouds sort in the small instance's LDS, the C2 surf clouds in the large one's
        assert 0 < s["n_corner"].min() and s["n_corner"].max() <= LC, s["n_corner"]
        if cfg == "C2":
            assert LC < s["n_surf"].min() and s["n_surf"].max() <= LS, s["n_surf"]
        r = ref[ex * rec:(ex + 1) * rec]
        assert p.tobytes() == r[:n * 24], (cfg, ex)
        assert s.tobytes() == r[n * 24:], (cfg, ex)


# ------------------------------------------------------------------------------- cloud sizes
CORNER_SIZES = (0, 1, 63, 64, 65, LC - 64 * (SMALL_T // 64), LC - 1, LC, LC + 1)
SURF_SIZES = (LS - 1024, LS, LS + 1)  # every step used on some waves, full chunks, fallback

_SIZES_CODE = (
    "import sys, numpy as np; sys.path.insert(0, %r); from feature_base_pointcloud_registration_amd import api, synth\n"
    "from feature_base_pointcloud_registration_amd.fbr_types import REG_STATS_FIELDS\n"
    "d = np.load(%r); m = synth.config_map('C2')\n"
    "for ex in (0, 1):\n"
    "    with api.Context(synth.config_params('C2', exact_voxel_order=ex)) as c:\n"
    "        c.set_map(*m)\n"
    "        for k in range(%d):\n"
    "            p, s = c.register(d['corner_%%d' %% k], d['surf_%%d' %% k], d['guess'])\n"
    "            sys.stdout.buffer.write(p.astype(np.float32).tobytes() + np.array([s[f] for f in REG_STATS_FIELDS], np.float64).tobytes())\n")


def _resized(base, n, rng):
    """n points with the structure of the feature cloud `base`: its points repeated, each copy
    moved by up to 3 cm."""
    out = np.zeros(n, POINT_XYZI)
    if n:
        src = base[np.arange(n) % len(base)]
        for f in ("x", "y", "z"):
            out[f] = src[f] + rng.uniform(-0.03, 0.03, n).astype(np.float32)
        out["intensity"] = src["intensity"]
    return out


def test_cloud_sizes_around_both_lds_capacities():
    """Host clouds through fbr_register on a C2-shaped context.  With FBR_VG_SPLIT=1 (the
    few-segment split kernel off) its mapping DS is the two-set launch: corner set of capacity
    kCornerPerRing * 64 = 7,680 -> the 256 x 16 instance, surf set -> 1024 x 18.  Corner sizes
    around the step, chunk and LDS-capacity boundaries of the small instance (above Lc: its
    global-scratch branch), surf sizes around the large instance's.  Poses and statistics byte for
    byte against the global-scratch kernel, default and exact order; voxel counts against the
    oracle's VoxelGrid."""
    P = synth.config_params("C2")
    gt, guess = synth.job(5300)
    f = O.Stream(P).features(synth.scan(gt, 64, 1800, seed=5300))
    rng = np.random.default_rng(53)
    cases = [(_resized(f["corner"], nc, rng), _resized(f["surf"], SURF_SIZES[k % 3], rng))
             for k, nc in enumerate(CORNER_SIZES)]
    path = os.path.join(TMP, "fbr_vg_classes_sizes.npz")
    arrs = {"guess": np.asarray(guess, np.float32)}
    for k, (c, s) in enumerate(cases):
        arrs["corner_%d" % k], arrs["surf_%d" % k] = c, s
    np.savez(path, **arrs)
    code = _SIZES_CODE % (REPO, path, len(cases))
    got = _child(code, {"FBR_VG_SPLIT": "1"})
    ref = _child(code, {"FBR_VG_SPLIT": "1", "FBR_VG_INPLACE": "0"})
    rec = 24 + 8 * len(REG_STATS_FIELDS)
    assert len(got) == len(ref) == 2 * len(cases) * rec
    for ex in (0, 1):
        for k, (c, s) in enumerate(cases):
            o = (ex * len(cases) + k) * rec
            assert got[o:o + rec] == ref[o:o + rec], (ex, len(c), len(s))
            st = dict(zip(REG_STATS_FIELDS, np.frombuffer(got[o + 24:o + rec], np.float64)))
            assert (st["n_corner"], st["n_surf"]) == (len(c), len(s))
            assert st["n_corner_ds"] == (len(O.voxel_grid(c, P.mapping_corner_leaf_size)) if len(c) else 0), (ex, len(c))
            assert st["n_surf_ds"] == len(O.voxel_grid(s, P.mapping_surf_leaf_size)), (ex, len(s))


# ----------------------------------------------------------------------- radix-sort selftest
def _small_radix_cases():
    """Every chunk fill of the 256 x 16 in-place sort: n = 256 k fills k steps of every wave, the
    sizes below and above it leave the last step ragged or spill one point into the next."""
    rng = np.random.default_rng(17)
    nw = SMALL_T // 64
    sizes = sorted({1, 2, 63, 64, 65, 127, LC - 65, LC - 1, LC}
                   | {64 * nw * k for k in range(1, SMALL_KPL + 1)}
                   | {64 * nw * k - 37 for k in range(1, SMALL_KPL + 1)}
                   | {64 * nw * k + 1 for k in range(1, SMALL_KPL)})
    for n in sizes:
        yield n, 24, rng.integers(0, 1 << 24, n)                                    # random
        yield n, 24, np.sort(rng.integers(0, 1 << 24, n))                           # sorted
        yield n, 9, np.full(n, 300)                                                 # constant
        yield n, 18, np.repeat(rng.integers(0, 1 << 18, (n + 99) // 100), 100)[:n]  # runs of 100 equal keys


def test_small_instance_radix_sort_is_a_stable_sort():
    """fbr_selftest_radix_sort variant 6 (vg_radix_sort_inplace<256, 16>, with the early exit at
    the first empty step) against a host stable sort on random, sorted, constant and run-heavy
    keys."""
    for n, nbits, keys in _small_radix_cases():
        keys = np.asarray(keys, np.uint64).astype(np.uint32) & np.uint32((1 << nbits) - 1)
        sk, perm = api.selftest_radix_sort(keys, nbits, 6)
        ref = np.argsort(keys, kind="stable")
        assert np.array_equal(perm, ref), (n, nbits, int(np.nonzero(perm != ref)[0][0]))
        assert np.array_equal(sk, keys[ref]), (n, nbits)
