"""Seeded pose graphs for the pose-graph tests (tests/test_pg_model.py on the CPU,
tests/test_pose_graph.py on the GPU), and what turns one into the NumPy model's factors, the CPU
probe's, or the calls on a Context.

A graph is a dict: poses [N, 6] float32 = the stored key poses [roll, pitch, yaw, x, y, z] (the
optimiser's start), truth [N, 6] float64, and spec, a list of
  ("prior", i, pose6 float32, var6) | ("between_poses", i, j, pose_i float32, pose_j float32, var6) |
  ("between", i, j, M [4, 4] float32, var6) | ("gps", i, xyz float64, var3)
in the order they are added, with the C-ABI's argument types.
"""
import numpy as np

import pg_model as PM

# the reference's noise values (mapOptmization.h:1523, :1531, :746, :1627), as variances
PRIOR_VAR = np.array([1e-2, 1e-2, np.pi * np.pi, 1e8, 1e8, 1e8])
ODOM_VAR = np.array([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4])
LOOP_VAR = np.full(6, 0.1)
GPS_VAR = np.full(3, 1.0)
TIGHT_VAR = np.full(6, 1e-4)

# The end-to-end test of tests/test_pose_graph.py: the model's own error at the last keyframe of the
# drifted out-and-back fixture after optimising (against ground truth, metres), measured from the
# model on the CPU by tests/test_pg_model.py::test_end_to_end_model_error, which keeps it current.
MODEL_E2E_LAST_ERR = 0.4089  # metres (0.4416 before the optimise)


def _matrix(R, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    return M.astype(np.float32)


def circle(n, loops=(), gps_every=0, prior="reference", seed=0, radius=30.0, no_prior=False, yaw_bias=1e-3):
    """A drifting circle: n keyframes once around, roll / pitch a few 0.01 rad; the stored poses
    are the dead reckoning of noisy odometry (2e-3 rad, 0.02 m per step, plus a yaw bias) from the
    true first pose; odometry factors are the stored poses' own increments, as saveKeyFramesAndFactor
    adds them (:1533-1537); loop factors the true relative pose with 1e-3 noise, as float matrices."""
    rng = np.random.default_rng(seed)
    th = 2.0 * np.pi * np.arange(n) / n
    truth = np.stack([0.02 * np.sin(3 * th), 0.03 * np.cos(2 * th), th + np.pi / 2, radius * np.cos(th),
                      radius * np.sin(th), 0.5 * np.sin(th)], 1)
    truth[:, 2] = (truth[:, 2] + np.pi) % (2 * np.pi) - np.pi  # yaw crosses +-pi on the way
    Rt, tt = PM.poses_from_euler(truth)
    R, t = [Rt[0]], [tt[0]]
    for k in range(1, n):
        dR, dt = PM.between_pose(Rt[k - 1], tt[k - 1], Rt[k], tt[k])
        dR = dR @ PM.exp_so3(rng.normal(0, 2e-3, 3) + np.array([0, 0, yaw_bias]))
        dt = dt + rng.normal(0, 0.02, 3)
        R.append(R[-1] @ dR)
        t.append(t[-1] + R[-2] @ dt)
    poses = PM.euler_from_poses(np.stack(R), np.stack(t)).astype(np.float32)
    spec = []
    if not no_prior:
        spec.append(("prior", 0, poses[0].copy(), PRIOR_VAR if prior == "reference" else TIGHT_VAR))
    for k in range(1, n):
        spec.append(("between_poses", k - 1, k, poses[k - 1].copy(), poses[k].copy(), ODOM_VAR))
    for (i, j) in loops:
        dR, dt = PM.between_pose(Rt[i], tt[i], Rt[j], tt[j])
        dR = dR @ PM.exp_so3(rng.normal(0, 1e-3, 3))
        spec.append(("between", i, j, _matrix(dR, dt + rng.normal(0, 1e-3, 3)), LOOP_VAR))
    if gps_every:
        for k in range(0, n, gps_every):
            spec.append(("gps", k, tt[k] + rng.normal(0, 0.1, 3), GPS_VAR))
    return dict(poses=poses, truth=truth, spec=spec, absolute=bool(gps_every) or prior != "reference")


def wrong_chain(n=12, seed=3, prior="tight"):
    """No loop, so H = T; the stored poses disagree with the odometry factors.  Every pair carries two
    odometry factors that disagree with each other (the truth, and the truth with 2e-3 rad / 0.02 m of
    noise; the second one added j -> i), so the minimum's cost is not zero and a relative cost
    difference means something.  The prior is tight by default: see DESIGN §4.10 on why the
    reference's 1e8 prior variance costs the one-iteration solve its last digits."""
    g = circle(n, seed=seed)
    rng = np.random.default_rng(seed + 100)
    Rt, tt = PM.poses_from_euler(g["truth"])
    spec = [("prior", 0, g["truth"][0].astype(np.float32), PRIOR_VAR if prior == "reference" else TIGHT_VAR)]
    for k in range(1, n):
        dR, dt = PM.between_pose(Rt[k - 1], tt[k - 1], Rt[k], tt[k])
        spec.append(("between", k - 1, k, _matrix(dR, dt), ODOM_VAR))
        dR, dt = PM.between_pose(Rt[k], tt[k], Rt[k - 1], tt[k - 1])
        spec.append(("between", k, k - 1, _matrix(dR @ PM.exp_so3(rng.normal(0, 2e-3, 3)), dt + rng.normal(0, 0.02, 3)),
                     ODOM_VAR))
    return dict(poses=g["poses"], truth=g["truth"], spec=spec, absolute=prior != "reference")


def drifted_out_and_back(poses):
    """test_loop_closure's out-and-back key poses (KEYPOSE records) with its drift accumulated along
    the run: keyframe k carries k / 19 of the last keyframe's drift (which stays as it is)."""
    import test_loop_closure as TL
    out = poses.copy()
    n = len(out)
    for name, v in TL.DRIFT.items():
        gt_last = out[name][n - 1] - np.float32(v)
        out[name][n - 1] = gt_last
        out[name] += (np.float32(v) * np.arange(n) / (n - 1)).astype(np.float32)
    return out


def e2e_spec(kposes, loop=None):
    """Prior on keyframe 0, odometry between consecutive stored poses, and the loop (latest, closest,
    between [16] float32, fitness) if there is one, with the reference's noise values."""
    e = np.stack([[k["roll"], k["pitch"], k["yaw"], k["x"], k["y"], k["z"]] for k in kposes]).astype(np.float32)
    spec = [("prior", 0, e[0].copy(), PRIOR_VAR)]
    for k in range(1, len(e)):
        spec.append(("between_poses", k - 1, k, e[k - 1].copy(), e[k].copy(), ODOM_VAR))
    if loop is not None:
        i, j, btw, fitness = loop
        spec.append(("between", i, j, np.asarray(btw, np.float32).reshape(4, 4), np.full(6, float(np.float32(fitness)))))
    return e, spec


def model_factors(spec):
    """The NumPy model's factors of a spec, with the C-ABI's conversions (float inputs widened to
    double, between_poses computed in double)."""
    out = []
    for s in spec:
        if s[0] == "prior":
            R, t = PM.poses_from_euler(np.asarray(s[2], np.float32).astype(np.float64))
            out.append(PM.make_factor("prior", s[1], -1, R[0], t[0], s[3]))
        elif s[0] == "between_poses":
            R, t = PM.poses_from_euler(np.stack([s[3], s[4]]).astype(np.float32).astype(np.float64))
            out.append(PM.make_factor("between", s[1], s[2], *PM.between_pose(R[0], t[0], R[1], t[1]), s[5]))
        elif s[0] == "between":
            M = np.asarray(s[3], np.float32).astype(np.float64).reshape(4, 4)
            out.append(PM.make_factor("between", s[1], s[2], M[:3, :3], M[:3, 3], s[4]))
        else:
            out.append(PM.make_factor("gps", s[1], -1, None, np.asarray(s[2], np.float64), s[3]))
    return out


def add_to_context(ctx, spec):
    for s in spec:
        if s[0] == "prior":
            ctx.pg_add_prior(s[1], s[2], s[3])
        elif s[0] == "between_poses":
            ctx.pg_add_between_poses(s[1], s[2], s[3], s[4], s[5])
        elif s[0] == "between":
            ctx.pg_add_between(s[1], s[2], s[3], s[4])
        else:
            ctx.pg_add_gps(s[1], s[2], s[3])


def n_loop_factors(spec):
    return sum(1 for s in spec if s[0] in ("between", "between_poses") and abs(s[1] - s[2]) != 1)


def run_model(g, **kw):
    """The model's minimiser of a graph: (R, t, info)."""
    f = model_factors(g["spec"])
    R0, t0 = PM.poses_from_euler(g["poses"].astype(np.float64))
    return PM.lm(f, R0, t0, chain_solver=n_loop_factors(g["spec"]) == 0 and len(R0) > 300, **kw)


def compare(g, eul, R, t):
    """Differences of optimised poses `eul` [N, 6] to the model's (R, t): relative poses (m, rad),
    absolute poses (m, rad), node 0's translation (m)."""
    Rd, td = PM.poses_from_euler(eul)
    rel = PM.pose_differences(*PM.relative_poses(Rd, td), *PM.relative_poses(R, t))
    ab = PM.pose_differences(Rd, td, R, t)
    return dict(rel_t=rel[0], rel_r=rel[1], abs_t=ab[0], abs_r=ab[1], node0=float(np.linalg.norm(td[0] - t[0])))
