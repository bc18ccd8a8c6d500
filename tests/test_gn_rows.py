"""The per-query functions of the Gauss-Newton residual pass on the device against tests/gn_model.py,
bit for bit: corner_fit, surf_fit, corner_apply, surf_apply and the LMOptimization row on the cases
of tests/gn_cases.py (fbr_selftest_gn_rows: one launch), res_reduce's index map on rows of the
test's choosing (fbr_selftest_gn_reduce), qr_solve6 and lu_inv6 against the oracle's pinned
routines (fbr_selftest_solve6).  tests/test_gn_model.py checks the model itself, and that the case
table keeps its shares of accepted and rejected cases, on the CPU.
"""
import numpy as np
import pytest

import gn_cases as C
import gn_model as G
import knn_model as K
import pyoracle as O
from feature_base_pointcloud_registration_amd import api
from feature_base_pointcloud_registration_amd.fbr_types import default_params, ptr

pytestmark = pytest.mark.gpu
F = np.float32


def same_bits(got, want):
    """Equal as bits; where the model yields NaN the device must too, at the same positions (the
    sign and payload of the NaN of 0 / 0 or inf - inf are undefined in the reference as well: they
    are the host instruction set's choice)."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    nan = np.isnan(want)
    return (np.isnan(got) == nan) & (nan | (got.view(np.uint32) == want.view(np.uint32)))


def test_fits_residuals_and_rows_equal_the_model():
    c = C.build()
    want = C.model_rows(c)
    got = api.selftest_gn_rows(C.device_input(c))
    n = len(c["kind"])
    assert n >= 200 and len(got["fit_ok"]) == n
    bad = []
    for i in range(n):
        for f in ("fit_ok", "ok"):
            if bool(got[f][i]) != bool(want[f][i]):
                bad.append((i, c["tag"][i], f, bool(got[f][i]), bool(want[f][i])))
        for f in ("fit", "coeff", "row"):
            if not same_bits(got[f][i], want[f][i]).all():
                bad.append((i, c["tag"][i], f, got[f][i], want[f][i]))
        if not same_bits(got["b"][i:i + 1], want["b"][i:i + 1]).all():
            bad.append((i, c["tag"][i], "b", got["b"][i], want["b"][i]))
    assert not bad, (len(bad), bad[:6])
    # every case ran, and the table keeps its shares (asserted on the model in test_gn_model.py)
    for kind in (C.CORNER, C.SURF):
        acc = got["ok"][c["kind"] == kind].mean()
        assert acc >= 1 / 3 and 1 - acc >= 1 / 5, (kind, acc)


PRIMES = np.array([2, 3, 5, 7, 11, 13], F)  # every product of two of them, and of one with 17, is distinct


def reduce_sets():
    """(rows (s, 256, 6), b (s, 256), ok (s, 256), exact (s,)): one row at each slot in turn, all
    rows equal, rows in wave 3 only, rows in every fourth slot, a random set with holes."""
    rng = np.random.default_rng(8)
    rows, b, ok, exact = [], [], [], []

    def add(r, bb, o, ex):
        rows.append(np.asarray(r, F)); b.append(np.asarray(bb, F)); ok.append(np.asarray(o, bool)); exact.append(ex)

    for slot in range(256):
        r, bb, o = np.zeros((256, 6), F), np.zeros(256, F), np.zeros(256, bool)
        r[slot], bb[slot], o[slot] = PRIMES * F(1 + slot % 5), F(17.0), True
        add(r, bb, o, True)
    add(np.tile(PRIMES * F(0.375), (256, 1)), np.full(256, -17.0, F), np.ones(256, bool), True)  # 256 t: exact
    o = np.arange(256) >= 192
    add(np.where(o[:, None], PRIMES, 0), np.where(o, 17.0, 0), o, True)  # 64 equal rows in wave 3
    add(rng.standard_normal((256, 6)) * 30 * o[:, None], rng.standard_normal(256) * o, o, False)
    o = np.arange(256) % 4 == 1
    add(rng.standard_normal((256, 6)) * o[:, None], rng.standard_normal(256) * o, o, False)
    o = rng.random(256) < 0.6
    # rows behind a cleared flag hold values: they must contribute nothing
    add(rng.standard_normal((256, 6)) * 100, rng.standard_normal(256), o, False)
    return np.stack(rows), np.stack(b), np.stack(ok), np.array(exact)


def test_reduction_puts_every_sum_in_its_place():
    rows, b, ok, exact = reduce_sets()
    got = api.selftest_gn_reduce(rows, b, ok)
    assert got.shape == (len(rows), 28)
    for s in range(len(rows)):
        want = G.item_partial(rows[s], b[s], ok[s])
        assert got[s, 27] == want[27], (s, got[s, 27], want[27])
        if exact[s]:  # one product, or equal products summed in a power-of-two tree: no rounding
            assert np.array_equal(got[s, :27], np.array(want[:27])), (s, got[s], want)
        else:  # any summation order of 256 exact terms
            t = np.abs(G.item_products(rows[s], b[s], ok[s])).sum(0)
            assert (np.abs(got[s, :27] - np.array(want[:27])) <= 256 * 2.0 ** -53 * t).all(), (s, got[s], want)


@pytest.fixture(scope="module")
def real_normal_matrices():
    """AtA, AtB of real registrations: the structured world's passes 0 .. 2 (diag_gn_last)."""
    s = K.structured_case()
    out = []
    for it in (1, 2, 3):
        with api.Context(default_params(16, 1800, crop_half=K.CROP_HALF, max_iterations=it)) as ctx:
            ctx.set_map(s["corner_map"], s["surf_map"])
            _, st = ctx.register(s["corner"], s["surf"], s["guess"])
            g = ctx.diag_gn_last()
        assert st["iterations"] == it and len(g["partial"]) > 0
        acc = np.zeros(28)
        for part in g["partial"]:
            acc = acc + part[:28]
        assert acc[27] == st["n_sel"] >= 50
        A = np.zeros((6, 6), F)
        q = 0
        for r in range(6):
            for c in range(r, 6):
                A[r, c] = A[c, r] = F(acc[q])
                q += 1
        out.append((A, acc[21:27].astype(F)))
    return out


def solve_cases(real):
    rng = np.random.default_rng(21)
    mats, rhs = [a for a, _ in real], [b for _, b in real]
    for _ in range(40):  # well-conditioned and not
        m = rng.standard_normal((6, 6)) * np.geomspace(1, rng.choice([1, 1e2, 1e4]), 6)
        mats.append((m @ m.T).astype(F)); rhs.append(rng.standard_normal(6).astype(F))
    for _ in range(20):  # general, not symmetric
        mats.append(rng.standard_normal((6, 6)).astype(F)); rhs.append(rng.standard_normal(6).astype(F))
    mats.append(np.diag([1, 1, 1, 1, 1, 1e-8]).astype(F)); rhs.append(np.ones(6, F))  # singular: return 0
    sing = rng.standard_normal((6, 6)).astype(F)
    sing[:, 2] = 0  # a zero column: no pivot in LU
    mats.append(sing); rhs.append(np.ones(6, F))
    mats.append(np.eye(6, dtype=F)[[3, 0, 5, 1, 2, 4]]); rhs.append(np.arange(1, 7, dtype=F))  # a permutation
    piv = np.triu(rng.uniform(1, 2, (6, 6)))[::-1].astype(F)  # the largest entry of every column lies below the diagonal
    piv += np.eye(6, dtype=F) * F(0.125)
    mats.append(np.ascontiguousarray(piv)); rhs.append(rng.standard_normal(6).astype(F))
    return np.stack(mats), np.stack(rhs)


def test_qr_solve_and_lu_inverse_equal_the_oracle(real_normal_matrices):
    mats, rhs = solve_cases(real_normal_matrices)
    qr_ret, x, lu_ret, inv = api.selftest_solve6(mats, rhs)
    n_sing_qr = n_sing_lu = 0
    with np.errstate(all="ignore"):
        for i in range(len(mats)):
            a, xb = mats[i].copy(), rhs[i].copy()
            want_ret = O.lib().orc_qr_solve(ptr(a), 6, ptr(xb))
            assert qr_ret[i] == want_ret, (i, qr_ret[i], want_ret)
            if want_ret:
                assert same_bits(x[i], xb).all(), (i, x[i], xb)
            else:
                n_sing_qr += 1
            wi = np.zeros((6, 6), F)
            want_ret = O.lib().orc_lu_inv(ptr(np.ascontiguousarray(mats[i])), 6, ptr(wi))
            assert lu_ret[i] == want_ret, (i, lu_ret[i], want_ret)
            if want_ret:
                assert same_bits(inv[i], wi).all(), (i, inv[i], wi)
            else:
                n_sing_lu += 1
    assert n_sing_qr >= 1 and n_sing_lu >= 1
    assert qr_ret[:3].all() and lu_ret[:3].all()  # the real normal matrices solve
