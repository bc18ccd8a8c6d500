"""The pose-graph optimiser (include/fbr.h "pose graph") through the C-ABI: exports and defaults on
the CPU; on the GPU the device's minimiser against the NumPy model's (tests/pg_model.py) with the
bars of tests/test_pg_model.py, bookkeeping, byte-stable results, optimise changing nothing, apply,
the loop closed end to end, the error paths and the resources.

Bars (the issue's): cost within 1e-8 relative; relative poses T_0^-1 T_i within 1e-6 m / 1e-7 rad;
absolute poses within the same only with GPS factors or a tight prior; with the reference's prior
(variance 1e8 on the translation) node 0 within 1e-3 m of the model's.
"""
import ctypes
import functools
import json

import numpy as np
import pytest

import pg_fixtures as F
import pg_model as PM
import test_loop_closure as TL
import test_resources as TR
from feature_base_pointcloud_registration_amd import api
from feature_base_pointcloud_registration_amd.fbr_types import (FBR_LOOP_CLOSED, FBR_PG_CONVERGED, FBR_PG_EMPTY,
                                                                FBR_PG_ITERATIONS, KEYPOSE, POINT_XYZI, FbrLoopResult,
                                                                FbrPgParams, FbrPgResult, default_params, keyframe_params,
                                                                pg_params)

PG_SYMBOLS = ["fbr_pg_params_default", "fbr_pg_reset", "fbr_pg_add_prior", "fbr_pg_add_between",
              "fbr_pg_add_between_poses", "fbr_pg_add_gps", "fbr_pg_add_loop", "fbr_pg_factor_count", "fbr_pg_optimize",
              "fbr_pg_poses", "fbr_pg_apply"]
TIGHT = dict(rel_cost_tol=1e-12, abs_cost_tol=1e-12, max_iterations=60)


# ---- CPU ------------------------------------------------------------------------------------------
def test_pose_graph_interface_is_exported():
    lib = ctypes.CDLL(api.lib_path())
    for name in PG_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in api.EXPORTED_SYMBOLS
    assert api.lib().fbr_abi_version() == 4
    assert ctypes.sizeof(FbrPgParams) == 72 and ctypes.sizeof(FbrPgResult) == 72
    p = FbrPgParams()
    ctypes.memset(ctypes.byref(p), 0xFF, ctypes.sizeof(p))
    api.lib().fbr_pg_params_default(ctypes.byref(p))
    q = pg_params()
    assert ctypes.string_at(ctypes.addressof(p), ctypes.sizeof(p)) == ctypes.string_at(ctypes.addressof(q), ctypes.sizeof(q))
    assert (p.max_iterations, p.max_pcg_iterations, p.rel_cost_tol, p.abs_cost_tol, p.pcg_rel_tol, p.lambda_init,
            p.lambda_factor, p.lambda_max) == (30, 200, 1e-5, 1e-5, 1e-8, 1e-5, 10.0, 1e10)
    for m in ("pg_reset", "pg_add_prior", "pg_add_between", "pg_add_between_poses", "pg_add_gps", "pg_add_loop",
              "pg_factor_count", "pg_optimize", "pg_apply"):
        assert callable(getattr(api.Context, m))


# ---- GPU ------------------------------------------------------------------------------------------
def tiny_cloud(k, n=5):
    rng = np.random.default_rng(1000 + k)
    c = np.zeros(n, POINT_XYZI)
    c["x"], c["y"], c["z"] = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-1, 1, n)
    return c


def keyposes(eul):
    kp = np.zeros(len(eul), KEYPOSE)
    e = np.asarray(eul, np.float32)
    kp["roll"], kp["pitch"], kp["yaw"], kp["x"], kp["y"], kp["z"] = e.T
    kp["time"] = 2.0 * np.arange(len(e))
    return kp


def load(ctx, g):
    ctx.keyframes_reset()
    for k, p in enumerate(keyposes(g["poses"])):
        ctx.keyframes_add(p, tiny_cloud(k), tiny_cloud(k + 7))
    assert ctx.pg_factor_count() == 0  # keyframes_reset emptied the list
    F.add_to_context(ctx, g["spec"])
    assert ctx.pg_factor_count() == len(g["spec"])


@pytest.fixture(scope="module")
def ctx():
    with api.Context(default_params(16, 1800)) as c:
        yield c


GRAPHS = {
    "n2": lambda: F.wrong_chain(2),
    "n3": lambda: F.wrong_chain(3),
    "n5": lambda: F.wrong_chain(5),
    "n64_k1": lambda: F.circle(64, loops=[(63, 0)], seed=11),
    # three loop factors: one two nodes apart, and one pair twice
    "n65_k3": lambda: F.circle(65, loops=[(64, 0), (40, 38), (64, 0)], seed=12),
    "n60_gps": lambda: F.circle(60, loops=[(59, 0)], gps_every=10, seed=3),
    "n257_k1_gps": lambda: F.circle(257, loops=[(256, 0)], gps_every=32, seed=13),
    "n1025_k0": lambda: F.wrong_chain(1025),
}


@functools.lru_cache(maxsize=None)
def graph_and_model(name):
    g = GRAPHS[name]()
    return g, F.run_model(g, **TIGHT)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRAPHS))
def test_device_reaches_the_models_minimiser(ctx, name):
    g, (R, t, mi) = graph_and_model(name)
    load(ctx, g)
    eul, r = ctx.pg_optimize(pg_params(**TIGHT))
    d = F.compare(g, eul, R, t)
    dc = abs(r["cost_final"] - mi["cost_final"]) / mi["cost_final"]
    print(f"{name}: model {mi['iterations']} steps, cost {mi['cost_initial']:.6g} -> {mi['cost_final']:.12g}; device "
          f"{r['iterations']} steps / {r['trials']} trials, {r['pcg_iterations']} PCG; cost diff {dc:.2e}; rel "
          f"{d['rel_t']:.2e} m {d['rel_r']:.2e} rad; abs {d['abs_t']:.2e} m {d['abs_r']:.2e} rad; node 0 {d['node0']:.2e} m")
    assert r["status"] in (FBR_PG_CONVERGED, FBR_PG_ITERATIONS)
    assert (r["n_nodes"], r["n_factors"], r["n_loop_factors"]) == (len(g["poses"]), len(g["spec"]),
                                                                  F.n_loop_factors(g["spec"]))
    assert r["iterations"] <= r["trials"] and r["cost_final"] <= r["cost_initial"]
    assert abs(r["cost_initial"] - mi["cost_initial"]) <= 1e-9 * mi["cost_initial"]
    assert dc < 1e-8
    assert d["rel_t"] < 1e-6 and d["rel_r"] < 1e-7
    if g["absolute"]:
        assert d["abs_t"] < 1e-6 and d["abs_r"] < 1e-7
    else:
        assert d["node0"] < 1e-3
    if r["n_loop_factors"] == 0:
        assert r["pcg_iterations"] == r["trials"]  # H = T: one iteration per solve
    assert r["max_translation_change"] > 0 and r["max_rotation_change"] > 0


@pytest.mark.gpu
def test_single_node_with_a_prior_returns_at_once(ctx):
    g = F.circle(1, seed=4)
    load(ctx, g)
    eul, r = ctx.pg_optimize()
    assert (r["status"], r["iterations"], r["trials"], r["pcg_iterations"]) == (FBR_PG_CONVERGED, 0, 0, 0)
    assert r["cost_initial"] == 0.0 and r["cost_final"] == 0.0 and r["n_nodes"] == 1
    R, t = PM.poses_from_euler(g["poses"].astype(np.float64))
    Rd, td = PM.poses_from_euler(eul)
    assert PM.pose_differences(Rd, td, R, t) < (1e-12, 1e-12)


@pytest.mark.gpu
def test_graph_without_a_prior(ctx):
    """The damping makes it solvable; the gauge is free, so relative poses only (default tolerances
    on both sides: lambda stays far above the rounding of the pivots)."""
    g = F.circle(40, loops=[(39, 0)], seed=14, no_prior=True)
    R, t, mi = F.run_model(g)
    load(ctx, g)
    eul, r = ctx.pg_optimize()
    d = F.compare(g, eul, R, t)
    print(f"no prior: model {mi['iterations']} steps, device {r['iterations']}; rel {d['rel_t']:.2e} m {d['rel_r']:.2e} rad")
    assert r["status"] == FBR_PG_CONVERGED and r["iterations"] == mi["iterations"]
    assert abs(r["cost_final"] - mi["cost_final"]) < 1e-8 * mi["cost_final"]
    assert d["rel_t"] < 1e-6 and d["rel_r"] < 1e-7


def result_bytes(r):
    return ctypes.string_at(ctypes.addressof(r), ctypes.sizeof(r))


def local_map_bytes(c, stamp):
    """The keyframe local map around the last keyframe, as bytes: it moves with the key poses (the
    store has no pose getter)."""
    c.extract_surrounding_keyframes(stamp, keyframe_params(search_radius=1e4))
    cm, sm = c.get_map()
    assert len(cm) + len(sm) > 0
    return cm.tobytes() + sm.tobytes()


@pytest.mark.gpu
def test_same_bytes_optimise_changes_nothing_and_apply(ctx):
    g = F.circle(65, loops=[(64, 0), (40, 38)], seed=15)
    load(ctx, g)
    before = local_map_bytes(ctx, 128.0)
    e1, r1 = ctx.pg_optimize(raw=True)
    e2, r2 = ctx.pg_optimize(raw=True)
    assert e1.tobytes() == e2.tobytes() and result_bytes(r1) == result_bytes(r2)
    assert r1.status == FBR_PG_CONVERGED and r1.iterations >= 1
    assert local_map_bytes(ctx, 128.0) == before  # no key pose moved: the local map's bytes are the same
    ctx.pg_apply()
    after = local_map_bytes(ctx, 128.0)
    assert after != before
    # a second context given the float-rounded result pose by pose builds the same local map
    with api.Context(default_params(16, 1800)) as other:
        kp = keyposes(g["poses"])
        for k, p in enumerate(kp):
            other.keyframes_add(p, tiny_cloud(k), tiny_cloud(k + 7))
        new = keyposes(e1.astype(np.float32))
        for k in range(len(kp)):
            other.keyframes_set_pose(k, new[k])
        assert local_map_bytes(other, 128.0) == after
    # the applied poses are the new start: the optimum of the same factors, so the next optimise
    # starts at a cost no higher than the last one ended
    # (rounding 65 poses to float: residuals of ~1e-4 sigma each, ~1e-6 of cost in all)
    _, r3 = ctx.pg_optimize()
    assert r3["cost_initial"] <= r1.cost_final * 1.001 + 1e-5


@pytest.mark.gpu
def test_loop_closed_end_to_end():
    """perform_loop_closure -> pg_add_loop -> optimise -> apply on the out-and-back run with its
    drift accumulated along the stored poses: the last keyframe ends within twice the model's own
    error (F.MODEL_E2E_LAST_ERR, measured on the CPU) and nearer the truth than before."""
    P, poses, corners, surfs, lp, _ = TL.fixture()
    kposes = F.drifted_out_and_back(poses)
    with api.Context(P) as c:
        TL.add_keyframes(c, kposes, corners, surfs)
        e0, spec = F.e2e_spec(kposes)
        F.add_to_context(c, spec)
        r = c.perform_loop_closure(TL.STAMP, lp, raw=True)
        assert r.status == FBR_LOOP_CLOSED and (r.latest_id, r.closest_id) == (19, 0)
        assert c.pg_add_loop(r) and c.pg_factor_count() == len(spec) + 1
        rejected = FbrLoopResult()
        rejected.status = 3
        assert not c.pg_add_loop(rejected) and c.pg_factor_count() == len(spec) + 1
        # the model on the same factors (the device's own loop measurement), both sides tight: every
        # keyframe within the bars of a reference-prior graph (1e-3 m for the gauge, 1e-6 m beside it)
        _, full = F.e2e_spec(kposes, (19, 0, np.array(r.between[:], np.float32), r.icp.fitness))
        R, t, mi = PM.lm(F.model_factors(full), *PM.poses_from_euler(e0.astype(np.float64)), **TIGHT)
        me = PM.euler_from_poses(R, t)
        tight, _ = c.pg_optimize(pg_params(**TIGHT))
        eul, res = c.pg_optimize()
        c.pg_apply()
        assert res["status"] == FBR_PG_CONVERGED and res["n_loop_factors"] == 1
    gt = np.stack([TL.gt_pose(k) for k in range(TL.N_KF)])
    err = np.linalg.norm(eul[:, 3:] - gt[:, 3:], axis=1)
    err_model = np.linalg.norm(me[:, 3:] - gt[:, 3:], axis=1)
    err_before = np.linalg.norm(e0[:, 3:].astype(np.float64) - gt[:, 3:], axis=1)
    err_tight = np.linalg.norm(tight[:, 3:] - gt[:, 3:], axis=1)
    print(f"last keyframe: before {err_before[-1]:.4f} m, device {err[-1]:.4f} m (model on the CPU, its own ICP: "
          f"{F.MODEL_E2E_LAST_ERR} m); tight tolerances: device {err_tight[-1]:.4f} m, model {err_model[-1]:.4f} m, "
          f"largest difference over the keyframes {np.abs(err_tight - err_model).max():.2e} m")
    assert np.abs(err_tight - err_model).max() < 1e-3 + 1e-6
    assert err[-1] <= 2.0 * F.MODEL_E2E_LAST_ERR
    assert err[-1] < err_before[-1]


@pytest.mark.gpu
def test_errors(ctx):
    g = F.circle(5, seed=16)
    load(ctx, g)
    n = ctx.pg_factor_count()
    var6, pose, eye = np.ones(6), np.zeros(6, np.float32), np.eye(4, dtype=np.float32)

    def refused(call):
        with pytest.raises(api.FbrError) as e:
            call()
        assert e.value.status == -1 and ctx.pg_factor_count() == n

    refused(lambda: ctx.pg_add_prior(5, pose, var6))
    refused(lambda: ctx.pg_add_prior(-1, pose, var6))
    refused(lambda: ctx.pg_add_between(0, 5, eye, var6))
    refused(lambda: ctx.pg_add_between(2, 2, eye, var6))
    refused(lambda: ctx.pg_add_between_poses(1, 1, pose, pose, var6))
    refused(lambda: ctx.pg_add_gps(7, np.zeros(3), np.ones(3)))
    for bad in (0.0, -1.0, np.nan, np.inf):
        v = var6.copy()
        v[4] = bad
        refused(lambda: ctx.pg_add_prior(0, pose, v))
        refused(lambda: ctx.pg_add_between(0, 1, eye, v))
        refused(lambda: ctx.pg_add_between_poses(0, 1, pose, pose, v))
        refused(lambda: ctx.pg_add_gps(0, np.zeros(3), v[3:]))
    # a node no factor touches
    ctx.keyframes_add(keyposes(g["poses"][:1])[0], tiny_cloud(0), tiny_cloud(1))
    with pytest.raises(api.FbrError) as e:
        ctx.pg_optimize()
    assert e.value.status == -7
    # apply after the store changed size, and without a result
    ctx.pg_add_between_poses(4, 5, g["poses"][4], g["poses"][0], F.ODOM_VAR)
    ctx.pg_optimize()
    ctx.keyframes_add(keyposes(g["poses"][:1])[0], tiny_cloud(0), tiny_cloud(1))
    with pytest.raises(api.FbrError) as e:
        ctx.pg_apply()
    assert e.value.status == -7
    ctx.keyframes_reset()
    with pytest.raises(api.FbrError) as e:
        ctx.pg_apply()
    assert e.value.status == -7
    # the empty store
    eul, r = ctx.pg_optimize()
    assert r["status"] == FBR_PG_EMPTY and len(eul) == 0
    ctx.pg_reset()
    assert ctx.pg_factor_count() == 0


PG_LIFE_CYCLE = """
import json
import numpy as np
import sys
sys.path.insert(0, "tests")
import pg_fixtures as F
from feature_base_pointcloud_registration_amd import api
from feature_base_pointcloud_registration_amd.fbr_types import KEYPOSE, POINT_XYZI, default_params
base = api.live_resources()
ctx = api.Context(default_params(16, 1800))
alive = api.live_resources()
grown = []
for n in (20, 3000):  # the second graph outgrows every buffer of the first
    g = F.circle(n, loops=[(n - 1, 0)], seed=n)
    ctx.keyframes_reset()
    for k in range(n):
        e = g["poses"][k]
        kp = np.array((e[3], e[4], e[5], k, e[0], e[1], e[2], 0.0, 2.0 * k), KEYPOSE)
        ctx.keyframes_add(kp, np.zeros(3, POINT_XYZI), np.zeros(3, POINT_XYZI))
    F.add_to_context(ctx, g["spec"])
    _, r = ctx.pg_optimize()
    ctx.pg_optimize()
    grown.append(api.live_resources())
    assert r["status"] in (0, 1), r  # converged, or 30 steps made
ctx.close()
print(json.dumps(dict(base=base, alive=alive, grown=grown, end=api.live_resources())))
"""


@pytest.mark.gpu
def test_pose_graph_buffers_return_to_baseline():
    """fbr_create allocates nothing for the optimiser; its buffers come with the first optimise (four
    device arrays and the host-mapped progress word), grow in place with a larger graph, and go with
    the context."""
    r = TR.run_child(PG_LIFE_CYCLE)
    created = [a - b for a, b in zip(r["alive"], r["base"])]
    assert created[:2] == [51, 7]
    assert r["grown"][0] == r["grown"][1]  # grown, not added to
    assert [g - a for g, a in zip(r["grown"][0], r["alive"])][2:] == [0, 0]
    assert r["end"] == r["base"]
