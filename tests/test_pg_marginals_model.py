"""The marginal covariances on the CPU: the CPU build of the kernels' arithmetic
(tests/native/pg_marg_probe.cpp over csrc/fbr_pg_host.h and csrc/fbr_pg.h) and the NumPy restatement
of the selected-inversion-plus-Woodbury route against a dense float64 inverse
(tests/pg_marg_model.py).  No GPU is needed.

The bar is derived, not tuned: max |Sigma_ii - model| over nodes and entries, over the largest model
entry, at most max(64 cond(H) 2^-53, 2^-40): the error bound of a backward-stable solve with a factor
64 for the chain of block operations; the floor covers N = 1, where cond = 1.  Each test prints the
figure it asserts.
"""
import os
import subprocess

import numpy as np
import pytest

import pg_fixtures as F
import pg_marg_model as MM
import pg_model as PM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel_err(cov, ref):
    return np.abs(cov - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("name", list(MM.FIXTURES))
def test_probe_against_the_dense_inverse(name):
    _, f, e = MM.fixture(name)
    ref, H = MM.dense_marginals(f, e)
    rc, cov = MM.probe_marginals(f, e)
    err, bar = rel_err(cov, ref), MM.bar(H)
    print(f"{name}: probe against dense inverse {err:.2e}, bar {bar:.2e} (cond {np.linalg.cond(H):.2e})")
    assert rc == PM.CONVERGED
    assert err <= bar


@pytest.mark.parametrize("name", list(MM.FIXTURES))
def test_numpy_restatement_against_the_dense_inverse(name):
    _, f, e = MM.fixture(name)
    ref, H = MM.dense_marginals(f, e)
    err, bar = rel_err(MM.selinv_marginals(f, e), ref), MM.bar(H)
    print(f"{name}: restatement against dense inverse {err:.2e}, bar {bar:.2e}")
    assert err <= bar


@pytest.mark.parametrize("name", list(MM.FIXTURES))
def test_blocks_are_symmetric_with_a_positive_diagonal(name):
    _, f, e = MM.fixture(name)
    rc, cov = MM.probe_marginals(f, e)
    assert rc == PM.CONVERGED
    assert np.array_equal(cov, cov.transpose(0, 2, 1))
    assert np.all(np.diagonal(cov, axis1=1, axis2=2) > 0.0)


@pytest.mark.parametrize("name", ["n5_k2", "n33_k3", "n40_k12_gps"])
def test_subset_equals_the_rows_of_the_full_call(name):
    _, f, e = MM.fixture(name)
    _, full = MM.probe_marginals(f, e)
    n = len(e)
    nodes = [n - 1, 0, n // 2, n - 1]  # out of order, and one node twice
    rc, sub = MM.probe_marginals(f, e, nodes=nodes)
    assert rc == PM.CONVERGED
    assert sub.tobytes() == full[nodes].tobytes()


def test_rhs_chunk_does_not_change_the_bytes():
    _, f, e = MM.fixture("n33_k3")  # 18 columns
    _, ref = MM.probe_marginals(f, e)
    for chunk in (7, 1):
        rc, cov = MM.probe_marginals(f, e, rhs_chunk=chunk)
        assert rc == PM.CONVERGED and cov.tobytes() == ref.tobytes()


def test_graph_without_a_prior_is_numerical():
    """T0 of a chain without a prior or GPS factor is singular: FBR_PG_NUMERICAL and a zeroed output.
    Through the probe only; the device is not made to fail on purpose."""
    g = F.circle(12, loops=[(11, 0)], seed=28, no_prior=True)
    rc, cov = MM.probe_marginals(F.model_factors(g["spec"]), g["poses"].astype(np.float64))
    assert rc == PM.NUMERICAL
    assert not cov.any()


def test_bad_node_index_is_refused():
    _, f, e = MM.fixture("n5_k2")
    assert MM.probe_marginals(f, e, nodes=[5])[0] == -1
    assert MM.probe_marginals(f, e, nodes=[-1])[0] == -1


@pytest.mark.parametrize("name", list(MM.GATE_FIXTURES))
def test_gps_gate(name):
    """Under the reference prior cond(H) ~ 2e16 and the dense inverse itself is good to ~1e-3
    relative: only the decision and agreement within a factor 2 are asserted."""
    _, f, e = MM.fixture(name)
    wanted = MM.GATE_FIXTURES[name][1]
    ref, _ = MM.dense_marginals(f, e)
    rc, w, xy = MM.probe_gps_gate(f, e, 25.0)
    print(f"{name}: probe xx {xy[0]:.6g} yy {xy[1]:.6g}; model xx {ref[-1][3, 3]:.6g} yy {ref[-1][4, 4]:.6g}")
    assert rc == PM.CONVERGED and w == wanted
    for a, b in zip(xy, (ref[-1][3, 3], ref[-1][4, 4])):
        assert 0.5 * b <= a <= 2.0 * b


def test_host_driver_under_sanitizers(tmp_path):
    """A stand-alone program (its own main, never loaded into Python, never run on a GPU) runs the
    host driver on a 33-node graph with three loops under AddressSanitizer and UBSan: every node, a
    subset with a repeat, rhs_chunk 7 and 1, a graph without a prior, a single node."""
    exe = str(tmp_path / "pg_marg_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(REPO, "feature_base_pointcloud_registration_amd", "csrc"),
                           "-o", exe, os.path.join(REPO, "tests", "native", "pg_marg_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pg_marg_check ok" in r.stdout
