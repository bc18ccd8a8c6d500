#!/usr/bin/env python3
"""CPU model of the flat kNN walk's memory pattern (fbr_grid_search.h knn5_grid<.., kFlat>), to size an
LDS-staged design before writing it.

For C2 jobs: the mapping-DS queries in Morton order (the device's order), transformed by the
registered pose, the 1 m (y, z) x 0.25 m (x) grid of the DS map, and a warm-start bound = the
query's true 5th-neighbour d2 (scipy KD-tree; the device's bound, the largest distance to the
previous iteration's 5 neighbours, is >= it).  Per 64-query wave it reports:
  lane points   points a lane scans (its pruned row ranges), and the flat walk's wave trips
                (= max over lanes) and lane efficiency (sum / 64 / max);
  union         distinct map points any lane of the wave scans (cell-level union), and the
                points of the per-row hull [min x0, max x1] (a row-union load);
  windows       for an LDS window of W points walked in address order over the row hulls: wave
                trips = sum over windows of the max per-lane count in the window.
usage: knn_union_sim.py [jobs]
"""
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
import pyoracle as O  # noqa: E402
from feature_base_pointcloud_registration_amd import synth  # noqa: E402

BELOW1 = np.float32(0.99999994)


def morton(ijk):
    def spread(v):
        v = v.astype(np.uint64) & np.uint64(0x1FFFFF)
        out = np.zeros_like(v)
        for b in range(21):
            out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
        return out
    return spread(ijk[:, 0]) | (spread(ijk[:, 1]) << np.uint64(1)) | (spread(ijk[:, 2]) << np.uint64(2))


def ds_morton(cloud, leaf):
    ds = O.voxel_grid(cloud, leaf)
    xyz = np.stack([ds["x"], ds["y"], ds["z"]], 1).astype(np.float32)
    ijk = np.floor(xyz / np.float32(leaf)).astype(np.int64)
    ijk -= ijk.min(0)
    return xyz[np.argsort(morton(ijk), kind="stable")]


def transform(pose, xyz):
    T = O.affine_from_pose(np.asarray(pose, np.float32))
    return (xyz @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def analyse(queries, mapxyz, windows=(128, 256, 512, 1024)):
    tree = cKDTree(mapxyz)
    d5 = tree.query(queries, k=5)[0][:, 4] ** 2
    invx, inv = 4.0, 1.0
    cx = np.floor(mapxyz[:, 0] * invx).astype(np.int64)
    cy = np.floor(mapxyz[:, 1] * inv).astype(np.int64)
    cz = np.floor(mapxyz[:, 2] * inv).astype(np.int64)
    from collections import Counter
    cell = Counter(zip(cz.tolist(), cy.tolist(), cx.tolist()))
    res = {"waves": 0, "lane_pts": 0, "trips": 0, "union": 0, "hull": 0, "win": {w: 0 for w in windows},
           "rows_per_wave": 0, "hulls": [], "boxes": []}
    for w0 in range(0, len(queries) - 63, 64):
        lanes = []
        for q, b in zip(queries[w0:w0 + 64], d5[w0:w0 + 64]):
            cut = min(np.float32(b), BELOW1)
            fx, fy, fz = np.floor(q[0] * invx), np.floor(q[1] * inv), np.floor(q[2] * inv)
            rows = []
            for oz in (-1, 0, 1):
                for oy in (-1, 0, 1):
                    def lb(qq, f, o, c):
                        if o == 0:
                            return 0.0
                        return (f + o) * c - qq if o > 0 else qq - (f + o + 1) * c
                    ly, lz = lb(q[1], fy, oy, 1.0), lb(q[2], fz, oz, 1.0)
                    base = ly * ly + lz * lz
                    if base > cut:
                        continue
                    xa = xb = 0
                    for o in range(1, 5):
                        a = lb(q[0], fx, -o, 0.25)
                        if a * a + base <= cut:
                            xa = -o
                        else:
                            break
                    for o in range(1, 5):
                        a = lb(q[0], fx, o, 0.25)
                        if a * a + base <= cut:
                            xb = o
                        else:
                            break
                    rows.append((int(fz + oz), int(fy + oy), int(fx + xa), int(fx + xb)))
            lanes.append(rows)
        per_lane = [sum(cell.get((z, y, x), 0) for z, y, x0, x1 in r for x in range(x0, x1 + 1)) for r in lanes]
        cells = {(z, y, x) for r in lanes for z, y, x0, x1 in r for x in range(x0, x1 + 1)}
        hull = {}
        for r in lanes:
            for z, y, x0, x1 in r:
                a, b = hull.get((z, y), (x0, x1))
                hull[(z, y)] = (min(a, x0), max(b, x1))
        # address order over the row hulls: (z, y) rows, then x cells
        order = []
        for (z, y), (x0, x1) in sorted(hull.items()):
            for x in range(x0, x1 + 1):
                order.append(((z, y, x), cell.get((z, y, x), 0)))
        pos, cum = {}, 0
        for key, n in order:
            pos[key] = (cum, n)
            cum += n
        res["waves"] += 1
        res["lane_pts"] += sum(per_lane)
        res["trips"] += max(per_lane)
        res["union"] += sum(cell.get(c, 0) for c in cells)
        res["hull"] += cum
        res["rows_per_wave"] += len(hull)
        res["hulls"].append(cum)
        zs = [k[0] for k in hull] or [0]
        ys = [k[1] for k in hull] or [0]
        res["boxes"].append((max(zs) - min(zs) + 1) * (max(ys) - min(ys) + 1))
        for W in windows:
            nwin = (cum + W - 1) // W
            cnt = np.zeros((64, max(nwin, 1)), np.int64)
            for li, r in enumerate(lanes):
                for z, y, x0, x1 in r:
                    for x in range(x0, x1 + 1):
                        s, n = pos[(z, y, x)]
                        for i in range(s, s + n):
                            cnt[li, i // W] += 1
            res["win"][W] += int(cnt.max(0).sum())
    return res


def main():
    nj = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    P = synth.config_params("C2")
    cmap, smap = synth.config_map("C2")
    omap = O.Map(P, cmap, smap)
    mc, ms = omap.arrays()
    mcx = np.stack([mc["x"], mc["y"], mc["z"]], 1).astype(np.float32)
    msx = np.stack([ms["x"], ms["y"], ms["z"]], 1).astype(np.float32)
    tot = {}
    for pts, guess, gt in synth.make_jobs("C2", nj, base_seed=1000):
        f = O.Stream(P).features(pts)
        pose, st, _ = omap.register(f["corner"], f["surf"], guess)
        for name, cloud, leaf, mp in (("corner", f["corner"], P.mapping_corner_leaf_size, mcx),
                                      ("surf", f["surf"], P.mapping_surf_leaf_size, msx)):
            q = transform(pose, ds_morton(cloud, leaf))
            r = analyse(q, mp)
            t = tot.setdefault(name, {"waves": 0, "lane_pts": 0, "trips": 0, "union": 0, "hull": 0, "rows_per_wave": 0,
                                      "win": {}, "hulls": [], "boxes": []})
            t["hulls"] += r["hulls"]
            t["boxes"] += r["boxes"]
            for k in ("waves", "lane_pts", "trips", "union", "hull", "rows_per_wave"):
                t[k] += r[k]
            for W, v in r["win"].items():
                t["win"][W] = t["win"].get(W, 0) + v
    for name, t in tot.items():
        w = max(t["waves"], 1)
        print(f"{name}: waves {w}, points per lane {t['lane_pts'] / w / 64:.1f}, flat trips per wave {t['trips'] / w:.1f} "
              f"(lane eff {t['lane_pts'] / 64 / max(t['trips'], 1):.2f}), rows per wave {t['rows_per_wave'] / w:.1f}, "
              f"union points {t['union'] / w:.0f}, row-hull points {t['hull'] / w:.0f}")
        h, b = np.array(t["hulls"]), np.array(t["boxes"])
        print("   hull points p50/p90/p99/max", np.percentile(h, [50, 90, 99]).round(), h.max(),
              " <=256:", (h <= 256).mean().round(3), "<=384:", (h <= 384).mean().round(3), "<=512:", (h <= 512).mean().round(3))
        print("   row box (ny*nz) p50/p90/max", np.percentile(b, [50, 90]).round(), b.max(), "<=64:", (b <= 64).mean().round(3))
        for W, v in sorted(t["win"].items()):
            print(f"   window {W:5d}: wave trips {v / w:.1f} (lane eff {t['lane_pts'] / 64 / max(v, 1):.2f})")


if __name__ == "__main__":
    main()
