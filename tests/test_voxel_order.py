"""PCL VoxelGrid's point order inside a voxel = libstdc++ std::sort's order of the index vector
(voxel_grid.cpp; featureExtraction.h:288-292, mapOptmization.h:251-257, 981-993).

The device reproduces it as "introsort partition phase, then a stable sort by key"
(csrc/fbr_introsort.h).  The CPU test pins that decomposition -- the level-by-level partition
phase with the closed-form __unguarded_partition -- against the host's real std::sort (oracle
probe); the GPU test runs the device emulation (global and LDS variants) against it."""
import numpy as np
import pytest

import pyoracle as O
from feature_base_pointcloud_registration_amd import api


def lg(n):
    return n.bit_length() - 1

def median_to_first(k, v, result, a, b, c):
    def sw(i, j):
        k[i], k[j] = k[j], k[i]; v[i], v[j] = v[j], v[i]
    if k[a] < k[b]:
        if k[b] < k[c]: sw(result, b)
        elif k[a] < k[c]: sw(result, c)
        else: sw(result, a)
    elif k[a] < k[c]: sw(result, a)
    elif k[b] < k[c]: sw(result, c)
    else: sw(result, b)

def heap_sort(k, v, first, last):
    # std::partial_sort(first, last, last) == make_heap + sort_heap, restated (stl_heap.h)
    kk = list(k[first:last]); vv = list(v[first:last]); n = len(kk)
    def adjust(hole, length, val):
        top = hole; second = hole
        while second < (length - 1) // 2:
            second = 2 * (second + 1)
            if kk[second][0] < kk[second - 1][0]: second -= 1
            kk[hole] = kk[second]; hole = second
        if (length & 1) == 0 and second == (length - 2) // 2:
            second = 2 * (second + 1); kk[hole] = kk[second - 1]; hole = second - 1
        parent = (hole - 1) // 2
        while hole > top and kk[parent][0] < val[0]:
            kk[hole] = kk[parent]; hole = parent; parent = (hole - 1) // 2
        kk[hole] = val
    kk = [(kk[i], vv[i]) for i in range(n)]
    if n >= 2:
        parent = (n - 2) // 2
        while True:
            adjust(parent, n, kk[parent])
            if parent == 0: break
            parent -= 1
    last_ = n
    while last_ > 1:
        last_ -= 1
        val = kk[last_]; kk[last_] = kk[0]
        adjust(0, last_, val)
    for i in range(n):
        k[first + i], v[first + i] = kk[i]

def partition(k, v, lo, hi, p):
    # __unguarded_partition(lo, hi, pivot value p) in closed form
    idx = np.arange(lo, hi)
    ks = np.array(k[lo:hi])
    posL = idx[~(ks < p)]
    posR = idx[~(p < ks)][::-1]
    m = min(len(posL), len(posR))
    K = int(np.sum(posL[:m] < posR[:m]))
    assert np.all(posL[:K] < posR[:K])
    for j in range(K):
        x, y = posL[j], posR[j]
        k[x], k[y] = k[y], k[x]; v[x], v[y] = v[y], v[x]
    cut = posL[K] if K < len(posL) else 1 << 60
    if K > 0: cut = min(cut, posR[K - 1])
    return min(cut, hi)

def emulate(keys):
    """The decomposition the device implements, restated serially."""
    n = len(keys)
    k = [int(x) for x in keys]; v = list(range(n))
    frames = [(0, n, 2 * lg(n))] if n > 16 else []
    while frames:  # one level
        nxt = []
        for first, last, depth in frames:
            if depth == 0:
                heap_sort(k, v, first, last); continue
            depth -= 1
            mid = first + (last - first) // 2
            median_to_first(k, v, first, first + 1, mid, last - 1)
            cut = partition(k, v, first + 1, last, k[first])
            for f in ((first, cut, depth), (cut, last, depth)):
                if f[1] - f[0] > 16: nxt.append(f)
        frames = nxt
    order = sorted(range(n), key=lambda i: (k[i], i))  # stable sort by key of the partitioned array
    return np.array([v[i] for i in order])



def key_cases(rng, count, nmax):
    for t in range(count):
        n = int(rng.integers(1, nmax))
        kind = t % 6
        if kind == 0:
            keys = rng.integers(0, max(1, n // 6), n)  # voxel-like: ~6 points per key
        elif kind == 1:
            keys = np.repeat(rng.integers(0, 50, n // 7 + 1), 7)[:n]  # runs of equal keys
        elif kind == 2:
            keys = np.sort(rng.integers(0, 100, n))  # sorted with ties
        elif kind == 3:
            keys = rng.integers(0, 3, n)  # massive ties
        elif kind == 4:  # organ pipe: exhausts introsort's depth limit (heap-sorted frames)
            n = min(n, 3000)
            keys = np.concatenate([np.arange(n // 2), np.arange(n - n // 2)[::-1]])
        else:
            keys = rng.integers(0, 1 << 30, n)  # distinct-ish
        yield keys.astype(np.uint32)


def test_partition_phase_then_stable_sort_is_std_sort():
    rng = np.random.default_rng(1)
    for keys in key_cases(rng, 48, 1500):
        assert np.array_equal(O.sort_voxel_pairs(keys), emulate(keys)), len(keys)
    for keys in ring_key_cases(4):
        assert np.array_equal(O.sort_voxel_pairs(keys), emulate(keys)), len(keys)


def ring_key_cases(rings=12):
    """The per-ring surf VoxelGrid's real key sequences (a C2 scan's rings: the candidates of the
    non-empty segments, PCL keys at odometrySurfLeafSize): close to median-of-3's bad case, ~16
    partition levels and depth-exhausted frames (tools/ring_partition_depth.py)."""
    from feature_base_pointcloud_registration_amd import synth
    P = synth.config_params("C2")
    pts = synth.make_jobs("C2", 1, base_seed=1000)[0][0]
    pr, f = O.project(P, pts), O.Stream(P).features(pts)
    inv = np.float32(1.0) / np.float32(P.odometry_surf_leaf_size)
    out = []
    for r in range(0, 64, 64 // rings):
        s, e = pr["start_ring"][r], pr["end_ring"][r]
        idx = []
        for j in range(6):
            sp, ep = (s * (6 - j) + e * j) // 6, (s * (5 - j) + e * (j + 1)) // 6 - 1
            if sp < ep:
                idx += [k for k in range(sp, ep + 1) if f["label"][k] <= 0]
        c = pr["cloud"][idx]
        x = np.stack([c["x"], c["y"], c["z"]], 1).astype(np.float32)
        mnb = np.floor(x.min(0) * inv).astype(np.int64)
        dx = np.floor(x.max(0) * inv).astype(np.int64) - mnb + 1
        ijk = np.floor(x * inv).astype(np.int64) - mnb
        out.append((ijk[:, 0] + ijk[:, 1] * dx[0] + ijk[:, 2] * dx[0] * dx[1]).astype(np.uint32))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("lds", [0, 1, 2, 3])
def test_device_voxel_order_is_std_sort(lds):
    rng = np.random.default_rng(2 + lds)
    for keys in key_cases(rng, 120, {0: 60000, 1: 8000, 2: 18432, 3: 4096}[lds]):
        assert np.array_equal(api.selftest_voxel_order(keys, lds=lds), O.sort_voxel_pairs(keys)), len(keys)
    for n in {0: (17, 2049, 18432, 18433), 1: (17, 2049, 8192), 2: (17, 2049, 8192, 18431, 18432),
              3: (17, 129, 2049, 4096)}[lds]:
        keys = rng.integers(0, max(1, n // 6), n).astype(np.uint32)
        assert np.array_equal(api.selftest_voxel_order(keys, lds=lds), O.sort_voxel_pairs(keys)), n
    for keys in ring_key_cases():
        assert np.array_equal(api.selftest_voxel_order(keys, lds=lds), O.sort_voxel_pairs(keys)), len(keys)


def _radix_cases(cap, nw):
    """Key arrays for a wave-chunk radix sort with nw waves and capacity cap: every chunk fill up to
    full chunks (steps of 64 per wave), ragged sizes, and key patterns with long equal-digit runs
    (sorted / spatially ordered / constant / few distinct) next to random ones."""
    rng = np.random.default_rng(11)
    sizes = sorted({1, 2, 63, 64, 65, 127, 640, cap // 2 + 3, cap - 65, cap - 1, cap}
                   | {min(cap, nw * 64 * k) for k in (1, 2, 5, 9, 13, 17, 18) if nw * 64 * k <= cap})
    for n in sizes:
        yield n, 24, rng.integers(0, 1 << 24, n)
        yield n, 24, np.sort(rng.integers(0, 1 << 24, n))                     # long runs in the upper digits
        yield n, 18, np.repeat(rng.integers(0, 1 << 18, (n + 99) // 100), 100)[:n]  # runs of 100 equal keys
        yield n, 9, np.full(n, 300)                                           # one key
        yield n, 30, (np.arange(n) * 2654435761) % (1 << 30)                  # distinct, scattered
        x, y, z = rng.integers(0, 1024, (3, n))
        o = np.lexsort((x, y, z))                                             # spatially ordered Morton keys
        yield n, 30, np.array([_morton(a, b, c) for a, b, c in zip(x[o], y[o], z[o])], np.int64)


def _morton(x, y, z):
    k = 0
    for b in range(10):
        k |= ((int(x) >> b) & 1) << (3 * b) | ((int(y) >> b) & 1) << (3 * b + 1) | ((int(z) >> b) & 1) << (3 * b + 2)
    return k


@pytest.mark.gpu
@pytest.mark.parametrize("variant,cap,nw", [(0, 4096, 8), (1, 4096, 4), (2, 40000, 16), (3, 18432, 16), (4, 18432, 16),
                                            (5, 18432, 16)],
                         ids=["ring-lds-512", "segment-lds-256", "global-1024", "inplace-atomic", "inplace-leader",
                              "inplace-leader-r03"])
def test_voxel_radix_sorts_are_stable_sorts(variant, cap, nw):
    """Every wave-chunk radix sort configuration of fbr_vg_sort.h (fbr_selftest_radix_sort) against a
    host stable sort, on every chunk fill including full ones and on long equal-digit runs.  Variant
    4 is round 3's ballot-leader digit count in the in-place sort, 5 the exact form round 3 reverted
    (the leader count plus a wave-uniform early exit in both loops)."""
    from feature_base_pointcloud_registration_amd import api
    for n, nbits, keys in _radix_cases(cap, nw):
        keys = np.asarray(keys, np.uint64).astype(np.uint32) & np.uint32((1 << nbits) - 1 if nbits < 32 else 0xFFFFFFFF)
        sk, perm = api.selftest_radix_sort(keys, nbits, variant)
        ref = np.argsort(keys, kind="stable")
        assert np.array_equal(perm, ref), (variant, n, nbits, int(np.nonzero(perm != ref)[0][0]))
        assert np.array_equal(sk, keys[ref]), (variant, n, nbits)
