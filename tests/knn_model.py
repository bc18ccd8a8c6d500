"""The Gauss-Newton neighbour search restated: a float32 brute force and the inputs on which a
grid search goes wrong (NumPy only; tests/test_knn_model.py checks this file against the oracle's
KD-tree on the CPU, tests/test_knn_direct.py compares the device with it per query).

brute_knn5 is the search of fbr_gn.h as a definition: float32 squared distances in the device's
operation order (d = 0; d += dx*dx; d += dy*dy; d += dz*dz, each step rounded, no contraction),
only map points inside the inclusive crop box, order by (d2, map index), five kept, and the query
rejected unless the fifth has d2 < 1.  Because it is the same float32 arithmetic, no query is
ambiguous: the device has to return the same five indices in the same order.

Every case lives on exactly representable coordinates: a 0.5 m lattice over +-6 x +-6 x +-3 m
(8,125 points before the edits below), shuffled so that a map index says nothing about a position,
under a crop box of +-4 x +-4 x +-2 m whose planes cut the lattice.  A scan cloud is down-sampled
before the search (one voxel of the mapping leaf keeps one point), so the queries of a case set
are packed into sets in which every query has a voxel of its own; a query then reaches the search
bit for bit, which the device test asserts.
"""
import numpy as np

from feature_base_pointcloud_registration_amd.fbr_types import POINT_XYZI

F = np.float32
LEAF_C, LEAF_S = 0.2, 0.4          # mapping leaves of the lattice contexts (the defaults)
CROP_HALF = (4.0, 4.0, 2.0)
EDGE_MIN, SURF_MIN = 10, 100       # edge / surf_feature_min_valid_num (the defaults)
ONE = F(1.0)
BELOW_ONE = np.nextafter(F(1.0), F(0.0))


def cloud(xyz):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    out = np.zeros(len(xyz), POINT_XYZI)
    out["x"], out["y"], out["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out["intensity"] = np.arange(len(xyz), dtype=F)
    return out


def xyz_of(c):
    return np.stack([c["x"], c["y"], c["z"]], axis=1).astype(F)


def crop_box(guess, crop_half=CROP_HALF):
    """registration's box (:289-292) as k_gn_init stores it: -half + t and half + t in float32."""
    t = np.asarray(guess, F)[3:6]
    h = np.asarray(crop_half, F)
    return (-h) + t, h + t


def dist2(q, m):
    """float32 squared distances (len(q), len(m)) in flann::L2_Simple's order, each step rounded."""
    q = np.asarray(q, F).reshape(-1, 1, 3)
    m = np.asarray(m, F).reshape(1, -1, 3)
    d = q[..., 0] - m[..., 0]
    acc = d * d                      # 0 + dx * dx is dx * dx
    d = q[..., 1] - m[..., 1]
    acc = acc + d * d
    d = q[..., 2] - m[..., 2]
    acc = acc + d * d
    assert acc.dtype == F
    return acc


def brute_knn5(map_xyz, queries, bmin, bmax, chunk=256):
    """(len(queries), 5) int32 map indices in (d2, index) order, or -1 five times."""
    m = np.ascontiguousarray(map_xyz, F).reshape(-1, 3)
    q = np.ascontiguousarray(queries, F).reshape(-1, 3)
    bmin, bmax = np.asarray(bmin, F), np.asarray(bmax, F)
    keep = np.flatnonzero(np.all((m >= bmin) & (m <= bmax), axis=1)).astype(np.int32)  # pcl::CropBox, inclusive
    out = np.full((len(q), 5), -1, np.int32)
    if len(keep) < 5:
        return out
    mk = m[keep]
    for r0 in range(0, len(q), chunk):
        d = dist2(q[r0:r0 + chunk], mk)
        fifth = np.partition(d, 4, axis=1)[:, 4]
        for r in range(len(d)):
            if not fifth[r] < ONE:
                continue
            cand = np.flatnonzero(d[r] <= fifth[r])                 # ascending index: every tie is in
            cand = cand[np.argsort(d[r][cand], kind="stable")[:5]]  # (d2, index)
            out[r0 + r] = keep[cand]
    return out


def fifth_tie(map_xyz, query, bmin, bmax):
    """(d2 of the fifth neighbour, how many box points have exactly that d2, how many are nearer)."""
    m = np.ascontiguousarray(map_xyz, F).reshape(-1, 3)
    inb = np.all((m >= np.asarray(bmin, F)) & (m <= np.asarray(bmax, F)), axis=1)
    d = np.sort(dist2(np.asarray(query, F).reshape(1, 3), m[inb])[0])
    return d[4], int((d == d[4]).sum()), int((d < d[4]).sum())


# ------------------------------------------------------------------------------------ voxels
def voxel_keys(xyz, leaf):
    """PCL VoxelGrid's cell of each point up to the cloud's offset: floor(p * (1 / leaf)) in float."""
    inv = F(1.0) / F(leaf)
    return np.floor(np.asarray(xyz, F).reshape(-1, 3) * inv).astype(np.int64)


def one_per_voxel(xyz, leaf):
    k = voxel_keys(xyz, leaf)
    return len(np.unique(k, axis=0)) == len(k)


# ------------------------------------------------------------------------------------ the map
GATE_EQ1 = (-2.5, -2.0, 0.0)     # four points at d2 0.25, the fifth at d2 == 1.0f          -> rejected
GATE_BELOW = (1.0, -2.0, 0.0)    # four at 0.25, the fifth at d2 == nextafter(1, 0)          -> accepted
GATE_FOUR = (2.5, -0.5, 0.0)     # four at 0.25, nothing else below 1.25                     -> rejected
STARS = ((-1.0, -0.5, 1.0), (0.5, -3.5, -1.0), (3.0, -3.0, -0.5))  # point and its 6 face neighbours removed
HOLE = ((-2.0, 2.0), (1.0, 3.0))  # x in [-2, 2), y in [1, 3), every z: removed (absent chunks)
GATE_BELOW_POINT = (2.0 ** -24, -2.0 + 2.0 ** -12, 0.0)  # (1 - 2^-24)^2 -> 1 - 2^-23, + 2^-24 = 1 - 2^-24


def lattice_points():
    """The edited lattice in a fixed shuffled order (float32 (n, 3))."""
    gx = np.arange(-12, 13) * 0.5
    gz = np.arange(-6, 7) * 0.5
    p = np.array(np.meshgrid(gx, gx, gz, indexing="ij")).reshape(3, -1).T.astype(F)
    keep = np.ones(len(p), bool)
    # holes: the slab under which a row range of the hashed-chunk grid loses its left chunk, its
    # right chunk, or both (chunks of 16 x-cells start at the grid's first cell, x = -6)
    keep &= ~((p[:, 0] >= HOLE[0][0]) & (p[:, 0] < HOLE[0][1]) & (p[:, 1] >= HOLE[1][0]) & (p[:, 1] < HOLE[1][1]))
    # the gate cavities: everything within d2 <= 1 of the centre goes, except the four at
    # (+-0.5, 0, 0), (0, +-0.5, 0) and, for GATE_EQ1, the one at (+1, 0, 0)
    for c, fifth in ((GATE_EQ1, True), (GATE_BELOW, False), (GATE_FOUR, False)):
        d = p.astype(np.float64) - np.asarray(c)
        d2 = (d * d).sum(1)
        four = (d2 == 0.25) & (d[:, 2] == 0.0)
        one = (d[:, 0] == 1.0) & (d2 == 1.0)
        stay = (four | one) if fifth else four
        keep &= ~((d2 <= 1.0) & ~stay)
    for c in STARS:  # the 12 edge neighbours at d2 0.5 become the nearest: a 12-way tie
        d = p.astype(np.float64) - np.asarray(c)
        keep &= ~((d * d).sum(1) <= 0.25)
    p = p[keep]
    # the crop planes (guess translation 0): points with odd tangential parity move one float
    # beyond their plane (dropped), the others stay exactly on it (kept: the box is inclusive)
    ij = np.rint(p.astype(np.float64) * 2).astype(np.int64)
    for ax in range(3):
        h = F(CROP_HALF[ax])
        odd = (ij[:, (ax + 1) % 3] + ij[:, (ax + 2) % 3]) % 2 == 1
        for s in (-1.0, 1.0):
            on = (p[:, ax] == F(s) * h) & odd
            p[on, ax] = np.nextafter(F(s) * h, F(s) * F(np.inf))
    # points in the last x-cell before the seam x = -2 of the rows the hole empties (0.25 m and
    # 0.125 m cells alike): the end of a row range whose right chunk is absent has to include them
    seam = [(-2.0625, y, z) for y in (1.0, 1.5, 2.0, 2.5) for z in gz[2:-2]]
    p = np.vstack([p, np.asarray(seam, F), np.asarray([GATE_BELOW_POINT], F)])
    return p[np.random.default_rng(20240611).permutation(len(p))]


# ------------------------------------------------------------------------------------ queries
def _nudge(v, n):
    v = F(v)
    for _ in range(abs(n)):
        v = np.nextafter(v, F(np.inf) if n > 0 else F(-np.inf))
    return v


# fraction of a 1 m cell and a nudge in floats: faces of the 1 / 0.5 / 0.25 / 0.125 m grids, the
# half-cell switch of sgy / sgz (>= 0.5 of the 1 m cell, 0.25 / 0.75 of the 0.5 m cell) from either
# side, a lattice point from below, and a cell centre of the finest grid
FRACS = ((0.0, 0), (0.0, -1), (0.125, 0), (0.25, 0), (0.5, 0), (0.5, -1), (0.75, 0), (0.9375, 0))


def grid_queries():
    """Every combination of FRACS on the three axes, each in its own 1 m cell of the region below
    the hole (x in [-4, 4), y in [-4, 0), z in [-2, 2): negative and positive coordinates)."""
    cells = [(i, j, k) for k in range(-2, 2) for j in range(-4, 0) for i in range(-4, 4)]
    out, n = [], 0
    for fx, nx in FRACS:
        for fy, ny in FRACS:
            for fz, nz in FRACS:
                i, j, k = cells[(n * 37) % len(cells)]
                n += 1
                out.append((_nudge(i + fx, nx), _nudge(j + fy, ny), _nudge(k + fz, nz)))
    return np.asarray(out, F)


def tie_queries():
    """name -> (query, ties at the fifth distance, nearer points): the kept five are decided by map
    index alone.  On a lattice point: itself, then 6 at 0.25.  A cube centre: 8 at 0.1875.  A face
    centre: 4 at 0.125, then 8 at 0.375.  An edge midpoint: 2 at 0.0625, then 8 at 0.3125.  A star
    centre: 12 at 0.5."""
    q = {"point6_a": ((-3.0, -1.0, -1.0), 6, 1), "point6_b": ((3.0, -3.0, 1.5), 6, 1),
         "cube8_a": ((-3.25, -0.75, -1.25), 8, 0), "cube8_b": ((2.75, -3.25, 1.25), 8, 0),
         "face8_a": ((-0.75, -1.75, 0.0), 8, 4), "face8_b": ((0.25, -1.5, -1.25), 8, 4),
         "edge8_a": ((-0.25, -3.0, -0.5), 8, 2), "edge8_b": ((-1.0, -2.5, 1.25), 8, 2)}
    for n, c in enumerate(STARS):
        q["star12_%d" % n] = (c, 12, 0)
    return q


def gate_queries():
    """name -> (query, expected: True accepted / False rejected)."""
    return {"fifth_at_one": (GATE_EQ1, False), "fifth_below_one": (GATE_BELOW, True), "four_in_reach": (GATE_FOUR, False),
            "on_a_map_point": ((-3.5, -3.0, 1.0), True)}


def crop_queries():
    """Around each of the six planes (normal offsets -0.5 .. +0.5: inside, on the plane, outside with
    the nearest five inside) at tangential positions on and off the lattice, and the box's corners
    from inside, on them and outside."""
    tx, ty, tz = (1.0, -2.75, 0.625, 3.5), (-1.0, -2.75, -0.625, -3.5), (0.5, -0.25, 1.0, -1.5)
    out = []
    for s in (-1.0, 1.0):
        for off in (-0.5, -0.25, -0.125, 0.0, 0.125, 0.25, 0.5):
            for n in range(4):
                out.append((s * (CROP_HALF[0] + off), ty[n], tz[n]))
                out.append((tx[n], s * (CROP_HALF[1] + off), tz[n]))  # y = +4 lies beyond the hole: whole rows
                out.append((tx[n], ty[n], s * (CROP_HALF[2] + off)))
    for sx in (-1, 1):
        for sz in (-1, 1):
            out.append((sx * 3.75, -3.75, sz * 1.75))
            out.append((sx * 4.0, -4.0, sz * 2.0))
            out.append((sx * 4.25, -4.25, sz * 2.25))
    return np.asarray(out, F)


def hole_queries():
    """At the chunk seams x = -2 and x = 2 (0.25 m x-cells: chunks of 4 m from x = -6; 0.125 m:
    2 m), from either side and inside the hole, on rows the hole empties and rows it leaves."""
    xs = (-2.25, -2.0, float(_nudge(-2.0, -1)), float(_nudge(-2.0, 1)), -1.75, -1.5, 0.0, 0.125, 1.5, 1.75,
          float(_nudge(2.0, -1)), 2.0, 2.25)
    out = [(x, y, z) for x in xs for y in (0.75, 1.0, 1.5, 2.25, 2.75, 3.0, 3.5) for z in (-1.0, 0.25)]
    return np.asarray(out, F)


def extent_queries(sign):
    """Map-frame queries for the guess translation sign * (4, 4, 2) (box [0, 8] x [0, 8] x [0, 4] or
    its mirror image, which holds the lattice's corner): 0.25 .. 3.5 m outside the occupied box on
    each axis (found up to 0.75 m out where five points are in reach; rejected beyond; past R cells
    the search returns at once), and inside next to the faces."""
    top = (6.0, 6.0, 3.0)
    out = []
    for ax in range(3):
        for d in (-0.25, 0.0, 0.25, 0.5, 0.75, 0.875, 1.0, 1.25, 1.5, 2.0, 2.5, 3.5):
            for u, v in ((1.0, 1.0), (2.25, 0.75), (3.0, 2.5)):
                q = [0.0, 0.0, 0.0]
                q[ax] = top[ax] + d
                o = [a for a in range(3) if a != ax]
                q[o[0]], q[o[1]] = u, v
                out.append(tuple(sign * c for c in q))
    out.append(tuple(sign * c for c in (6.5, 6.5, 3.5)))
    out.append(tuple(sign * c for c in (6.25, 6.25, 3.25)))
    return np.asarray(out, F)


def filler_queries(n, seed):
    """General positions around the box (inside, across its planes and in the hole)."""
    rng = np.random.default_rng(seed)
    return rng.uniform((-4.6, -4.6, -2.6), (4.6, 4.6, 2.6), (n, 3)).astype(F)


# ------------------------------------------------------------------------------------ case sets
def pack_sets(queries, n_surf_min=300, n_corner_min=24, seed=1):
    """Split queries (n, 3) into scan clouds in which every point has its own voxel: a list of
    (corner (k, 3), surf (m, 3)).  Every sixth query is a corner query; each set is topped up with
    filler queries to more than one work item of surf queries (256 slots: slot 255, slot 256 and a
    partial last item) and more corners than edge_feature_min_valid_num."""
    sets = []
    for n, q in enumerate(np.asarray(queries, F).reshape(-1, 3)):
        kind = 0 if n % 6 == 5 else 1
        key = tuple(voxel_keys(q, (LEAF_C, LEAF_S)[kind])[0])
        for s in sets:
            if key not in s[kind]:
                break
        else:
            s = ({}, {})
            sets.append(s)
        s[kind][key] = q
    out = []
    for n, s in enumerate(sets):
        fill = iter(filler_queries(4000, seed * 1000 + n))
        for kind, want in ((0, n_corner_min), (1, n_surf_min)):
            while len(s[kind]) < want:
                q = next(fill)
                s[kind].setdefault(tuple(voxel_keys(q, (LEAF_C, LEAF_S)[kind])[0]), q)
        out.append((np.asarray(list(s[0].values()), F), np.asarray(list(s[1].values()), F)))
    return out


def lattice_cases():
    """The case sets on the lattice map: a list of dicts {name, guess (6,), corner, surf (scan-frame
    POINT_XYZI clouds), designed (map-frame (n, 3) queries that must reach the search bit for bit)}.
    Identity rotation: a map-frame query is scan point + translation, exact for these values."""
    cases = []

    def add(name, queries, t=(0.0, 0.0, 0.0), scan_frame=False, **kw):
        g = np.zeros(6, F)
        g[3:] = t
        queries = np.asarray(queries, F).reshape(-1, 3)
        if scan_frame:  # the search sees fl(p + t), one rounding
            scan, queries = queries, queries + g[3:]
        else:
            scan = queries - g[3:]
            assert np.array_equal(scan + g[3:], queries)  # T p is the designed query, bit for bit
        for n, (c_scan, s_scan) in enumerate(pack_sets(scan, **kw)):  # fillers: around the box, scan frame
            assert one_per_voxel(c_scan, LEAF_C) and one_per_voxel(s_scan, LEAF_S)
            cases.append(dict(name="%s_%d" % (name, n), guess=g, corner=cloud(c_scan), surf=cloud(s_scan),
                              designed=queries))

    special = [q for q, _, _ in tie_queries().values()] + [q for q, _ in gate_queries().values()]
    add("grid", grid_queries(), seed=1)
    add("ties_gate_crop", np.vstack([np.asarray(special, F), crop_queries()]), seed=2)
    add("holes", hole_queries(), seed=3)
    add("extent_pos", extent_queries(1.0), t=(4.0, 4.0, 2.0), seed=4)
    add("extent_neg", extent_queries(-1.0), t=(-4.0, -4.0, -2.0), seed=5)
    # planes off the lattice: the same grid queries under a box shifted by fractions of a cell
    add("shifted_box", grid_queries()[::3], t=(0.25, -0.375, 0.125), scan_frame=True, seed=6)
    # a query beyond 1e7 on either cloud: the scan's VoxelGrid then overflows its index range and
    # keeps the cloud as it is (PCL's "leaf size too small"), so this set is its own
    c, s = pack_sets(filler_queries(40, 77), seed=7)[0]
    c = np.vstack([c, np.asarray([(0.5, -1.0, -3.0e7)], F)])
    s = np.vstack([s, np.asarray([(3.0e7, 0.25, 0.5), (1.0, 2.0e7, 0.0)], F)])
    cases.append(dict(name="far", guess=np.zeros(6, F), corner=cloud(c), surf=cloud(s), designed=np.vstack([c[-1:], s[-2:]])))
    return cases


# ------------------------------------------------------------------------------------ structure
def structured_case():
    """A world with structure, so that iteration 0 keeps its rows and later passes run with the warm
    start: surf map = a floor and two walls on the 0.5 m lattice, corner map = vertical poles of
    points 0.25 m apart; the scan samples them off the lattice, with 1 cm of noise, from a pose
    about 10 cm and 30 mrad away from the guess (three iterations do not converge it).  Returns {corner_map, surf_map, corner, surf, guess, gt}."""
    g = np.arange(-12, 13) * 0.5
    gz = np.arange(-2, 5) * 0.5
    floor = [(x, y, -1.5) for x in g for y in g]
    wall_x = [(3.5, y, z) for y in g for z in gz]
    wall_y = [(x, 3.5, z) for x in g for z in gz if x != 3.5]
    surf_map = np.asarray(floor + wall_x + wall_y, F)
    poles = [(x, y) for x in (-3.25, -1.75, -0.25, 1.25, 2.75) for y in (-3.25, -1.75, -0.25, 1.25, 2.75)]
    corner_map = np.asarray([(x, y, z) for x, y in poles for z in np.arange(-6, 9) * 0.25], F)
    rng = np.random.default_rng(5)
    surf_map = surf_map[rng.permutation(len(surf_map))]
    corner_map = corner_map[rng.permutation(len(corner_map))]
    n = 900
    fl = np.stack([rng.uniform(-3.4, 3.3, n), rng.uniform(-3.4, 3.3, n), np.full(n, -1.5)], 1)
    wx = np.stack([np.full(n // 3, 3.5), rng.uniform(-3.4, 3.3, n // 3), rng.uniform(-1.3, 1.8, n // 3)], 1)
    wy = np.stack([rng.uniform(-3.4, 3.3, n // 3), np.full(n // 3, 3.5), rng.uniform(-1.3, 1.8, n // 3)], 1)
    pc = np.asarray([(x, y, z) for x, y in poles for z in rng.uniform(-1.3, 1.8, 6)])
    gt = np.array([0.02, -0.015, 0.03, 0.12, -0.1, 0.06])
    guess = np.zeros(6, F)

    def to_scan(w):  # world -> sensor at gt (roll, pitch, yaw, x, y, z), float64
        cr, sr, cp, sp, cy, sy = np.cos(gt[0]), np.sin(gt[0]), np.cos(gt[1]), np.sin(gt[1]), np.cos(gt[2]), np.sin(gt[2])
        R = np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                      [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                      [-sp, cp * sr, cp * cr]])
        return ((w - gt[3:]) @ R).astype(F)

    def thin(p, leaf):  # one point per voxel of the scan-side down-sample
        _, first = np.unique(voxel_keys(p, leaf), axis=0, return_index=True)
        return p[np.sort(first)]

    noise = lambda p: p + rng.normal(0.0, 0.01, p.shape)  # 1 cm: the steps do not vanish after one solve
    surf = thin(to_scan(noise(np.vstack([fl, wx, wy]))), LEAF_S)
    corner = thin(to_scan(noise(pc)), LEAF_C)
    return dict(corner_map=cloud(corner_map), surf_map=cloud(surf_map), corner=cloud(corner), surf=cloud(surf),
                guess=guess, gt=gt.astype(F))


def dense_cluster_case():
    """For the LDS block tiles: mapping leaves of 0.03 m and a solid 0.04 m lattice over a 0.72 m
    cube (18^3 = 5,832 points), so the tile of a 0.5 m block and one fine cell around it holds more
    than its 2,048 points and the block's queries take the over-capacity fallback; blocks at the
    cube's rim hold fewer and are served from their tiles."""
    k = np.arange(18) * 0.04
    m = np.array(np.meshgrid(k + 0.52, k - 0.86, k + 0.02, indexing="ij")).reshape(3, -1).T.astype(F)
    rng = np.random.default_rng(9)
    m = m[rng.permutation(len(m))]
    q = rng.uniform((0.5, -0.88, 0.0), (1.26, -0.12, 0.76), (1500, 3))
    gt = np.array([0.01, -0.008, 0.012, 0.011, -0.009, 0.007])
    cr, sr, cp, sp, cy, sy = np.cos(gt[0]), np.sin(gt[0]), np.cos(gt[1]), np.sin(gt[1]), np.cos(gt[2]), np.sin(gt[2])
    R = np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                  [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr], [-sp, cp * sr, cp * cr]])
    q = ((q - gt[3:]) @ R).astype(F)
    _, first = np.unique(voxel_keys(q, 0.03), axis=0, return_index=True)
    q = q[np.sort(first)]
    return dict(corner_map=cloud(m), surf_map=cloud(m), corner=cloud(q[:200]), surf=cloud(q[200:]),
                guess=np.zeros(6, F), gt=gt.astype(F), leaf=0.03)


# ------------------------------------------------------------------------------------ poses
def associate(T, p):
    """pointAssociateToMap as gn_knn_block writes it: T (12,) row-major 3 x 4 float32, p (n, 3);
    three products and three sums per coordinate, each rounded to float32."""
    T = np.asarray(T, F).reshape(3, 4)
    p = np.asarray(p, F).reshape(-1, 3)
    return np.stack([((T[k, 0] * p[:, 0] + T[k, 1] * p[:, 1]) + T[k, 2] * p[:, 2]) + T[k, 3] for k in range(3)], axis=1)


def pose_matrix64(pose):
    """pcl::getTransformation(x, y, z, roll, pitch, yaw) of [roll, pitch, yaw, x, y, z] in float64 (3 x 4)."""
    r, p, y = (float(v) for v in pose[:3])
    A, B, C, D, E, G = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    return np.array([[A * C, A * D * G - B * E, B * G + A * D * E, float(pose[3])],
                     [B * C, A * E + B * D * G, B * D * E - A * G, float(pose[4])],
                     [-D, C * G, C * E, float(pose[5])]])


def near(map_xyz, queries, r=2.0):
    """Indices (ascending) of the map points that may lie within r of a query: those whose cell of a
    grid of size r touches a query's cell (a superset; it keeps every point within r)."""
    qc = np.unique(np.floor(np.asarray(queries, np.float64) / r).astype(np.int64), axis=0)
    span = np.array(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij")).reshape(3, -1).T
    occ = np.unique((qc[:, None, :] + span[None]).reshape(-1, 3), axis=0)
    off, dim = occ.min(0), occ.max(0) - occ.min(0) + 1
    flat = lambda c: ((c[:, 0] - off[0]) * dim[1] + (c[:, 1] - off[1])) * dim[2] + (c[:, 2] - off[2])
    mc = np.floor(np.asarray(map_xyz, np.float64) / r).astype(np.int64)
    inside = np.all((mc >= off) & (mc < off + dim), axis=1)
    hit = np.zeros(len(mc), bool)
    hit[inside] = np.isin(flat(mc[inside]), flat(occ))
    return np.flatnonzero(hit)


def brute_knn5_near(map_xyz, queries, bmin, bmax):
    """brute_knn5 over the map points near a query only (a fifth neighbour is within 1 m)."""
    sub = near(map_xyz, queries)
    if len(sub) == 0:
        return np.full((len(queries), 5), -1, np.int32)
    idx = brute_knn5(np.asarray(map_xyz, F).reshape(-1, 3)[sub], queries, bmin, bmax)
    return np.where(idx >= 0, sub[np.maximum(idx, 0)], -1).astype(np.int32)
