"""The marginal covariances of the key poses (include/fbr.h "marginal covariances") through the
C-ABI: exports and defaults on the CPU; on the GPU Context.pg_marginals against the dense NumPy
model (tests/pg_marg_model.py) linearised at the device's own pg_poses() output, byte-stable
results, the GPS gate's two outcomes and the error paths.

The bar is the one of tests/test_pg_marginals_model.py: max |Sigma_ii - model| over nodes and
entries, over the largest model entry, at most max(64 cond(H) 2^-53, 2^-40).  A bad pivot
(FBR_PG_NUMERICAL) is covered on the CPU only: the device is not made to fail on purpose.
"""
import ctypes

import numpy as np
import pytest

import pg_fixtures as F
import pg_marg_model as MM
from feature_base_pointcloud_registration_amd import api
from feature_base_pointcloud_registration_amd.fbr_types import (FBR_PG_CONVERGED, FBR_PG_EMPTY, FbrPgMarginalParams,
                                                                FbrPgMarginalResult, default_params, pg_marginal_params,
                                                                pg_params)
from test_pose_graph import load

SYMBOLS = ["fbr_pg_marginal_params_default", "fbr_pg_marginals", "fbr_pg_gps_gate"]


# ---- CPU ------------------------------------------------------------------------------------------
def test_marginals_interface_is_exported():
    lib = ctypes.CDLL(api.lib_path())
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in api.EXPORTED_SYMBOLS
    assert api.lib().fbr_abi_version() == 4
    assert ctypes.sizeof(FbrPgMarginalParams) == 24 and ctypes.sizeof(FbrPgMarginalResult) == 24
    p = FbrPgMarginalParams()
    ctypes.memset(ctypes.byref(p), 0xFF, ctypes.sizeof(p))
    api.lib().fbr_pg_marginal_params_default(ctypes.byref(p))
    q = pg_marginal_params()
    assert ctypes.string_at(ctypes.addressof(p), ctypes.sizeof(p)) == ctypes.string_at(ctypes.addressof(q), ctypes.sizeof(q))
    assert (p.rhs_chunk, p.max_work_bytes) == (0, 0)
    assert callable(api.Context.pg_marginals) and callable(api.Context.pg_gps_gate)


# ---- GPU ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    with api.Context(default_params(16, 1800)) as c:
        yield c


def optimised(ctx, name):
    g, f = MM.graph(name)
    load(ctx, g)
    eul, r = ctx.pg_optimize(pg_params(**MM.TIGHT) if name in MM.FIXTURES else None)
    return g, f, eul, r


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MM.FIXTURES))
def test_device_against_the_dense_inverse(ctx, name):
    g, f, eul, _ = optimised(ctx, name)
    cov, info = ctx.pg_marginals()
    ref, H = MM.dense_marginals(f, eul)
    err, bar = np.abs(cov - ref).max() / np.abs(ref).max(), MM.bar(H)
    print(f"{name}: device against dense inverse {err:.2e}, bar {bar:.2e} (cond {np.linalg.cond(H):.2e}); "
          f"work {info['work_bytes']} bytes")
    assert info["status"] == FBR_PG_CONVERGED
    assert (info["n_nodes"], info["n_loop_factors"], info["n_out"]) == (len(eul), F.n_loop_factors(g["spec"]), len(eul))
    assert cov.shape == (len(eul), 6, 6)
    assert np.array_equal(cov, cov.transpose(0, 2, 1))
    assert np.all(np.diagonal(cov, axis1=1, axis2=2) > 0.0)
    assert err <= bar
    # the same bytes again
    again, _ = ctx.pg_marginals()
    assert again.tobytes() == cov.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n5_k2", "n40_k12_gps", "n300_k2_gps"])
def test_subset_equals_the_rows_of_the_full_call(ctx, name):
    _, _, eul, _ = optimised(ctx, name)
    full, _ = ctx.pg_marginals()
    n = len(eul)
    nodes = [n - 1, 0, n // 2, n - 1]  # out of order, and one node twice
    sub, info = ctx.pg_marginals(nodes)
    assert info["status"] == FBR_PG_CONVERGED and info["n_out"] == 4
    assert sub.tobytes() == full[nodes].tobytes()
    none, info = ctx.pg_marginals([])
    assert info["status"] == FBR_PG_EMPTY and len(none) == 0


@pytest.mark.gpu
def test_both_forward_substitutions_give_the_same_bytes(ctx):
    """Up to 1,024 (node, entry) lanes, 170 nodes, the forward substitution runs a workgroup per lane,
    above that a thread per lane: both sides of the threshold against the all-nodes call (1,800 lanes)."""
    optimised(ctx, "n300_k2_gps")
    full, _ = ctx.pg_marginals()
    for count in (1, 170, 171):
        nodes = np.arange(299, 299 - count, -1)
        sub, info = ctx.pg_marginals(nodes)
        assert info["status"] == FBR_PG_CONVERGED and sub.tobytes() == full[nodes].tobytes()


@pytest.mark.gpu
def test_rhs_chunk_does_not_change_the_bytes(ctx):
    optimised(ctx, "n33_k3")  # 18 columns
    ref, _ = ctx.pg_marginals()
    for chunk in (7, 1):
        cov, info = ctx.pg_marginals(rhs_chunk=chunk)
        assert info["status"] == FBR_PG_CONVERGED and cov.tobytes() == ref.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MM.GATE_FIXTURES))
def test_gps_gate(ctx, name):
    """Only the decision and agreement within a factor 2: under the reference prior cond(H) ~ 2e16."""
    _, f, eul, _ = optimised(ctx, name)
    ref, _ = MM.dense_marginals(f, eul)
    wanted, xy = ctx.pg_gps_gate(25.0)
    print(f"{name}: device xx {xy[0]:.6g} yy {xy[1]:.6g}; model xx {ref[-1][3, 3]:.6g} yy {ref[-1][4, 4]:.6g}")
    assert wanted == bool(MM.GATE_FIXTURES[name][1])
    for a, b in zip(xy, (ref[-1][3, 3], ref[-1][4, 4])):
        assert 0.5 * b <= a <= 2.0 * b
    last, _ = ctx.pg_marginals([len(eul) - 1])
    assert (last[0][3, 3], last[0][4, 4]) == (xy[0], xy[1])


def status_of(call):
    with pytest.raises(api.FbrError) as e:
        call()
    return e.value.status


@pytest.mark.gpu
def test_errors():
    g, _ = MM.graph("n5_k2")
    with api.Context(default_params(16, 1800)) as c:
        load(c, g)
        assert status_of(c.pg_marginals) == -7  # no optimise yet
        assert status_of(c.pg_gps_gate) == -7
        c.pg_optimize()
        cov, _ = c.pg_marginals()
        assert len(cov) == 5
        assert status_of(lambda: c.pg_marginals([5])) == -1
        assert status_of(lambda: c.pg_marginals([-1])) == -1
        assert status_of(lambda: c.pg_marginals(max_work_bytes=1)) == -4  # (two loop factors)
        assert status_of(lambda: c.pg_marginals(rhs_chunk=-1)) == -1
        c.pg_add_gps(2, np.zeros(3), np.ones(3))
        assert status_of(c.pg_marginals) == -7  # the factor count has changed since the optimise
        assert status_of(c.pg_gps_gate) == -7
        c.pg_optimize()
        assert len(c.pg_marginals()[0]) == 5
        c.keyframes_reset()
        assert status_of(c.pg_marginals) == -7
    assert api.lib().fbr_abi_version() == 4
