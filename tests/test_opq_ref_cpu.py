"""tests/opq_ref.py checked without a GPU: the reference of the resident OPQ trainer's tests
against plainer statements of the same thing, and the condition that keeps its ``tied`` data
honest: the codes of a plain left-to-right fp32 sum differ from those of Faiss's fvec_L2sqr
order (``tree_np``) in many rows, so a kernel that summed in another order cannot pass."""
import functools

import numpy as np
import pytest

import opq_ref as R
from indexpq_ref import KIND_L2, ref_encode, tree_np

MIN_DIFFER = 50  # rows per sub-quantizer; a seeded trial at n = 1100 gave 110 (dsub 4) to 451 (dsub 48)


def ltr_np(x, y, kind):
    """tree_np's signature, the squares added left to right in float32."""
    assert kind == KIND_L2
    t = np.asarray(x, np.float32) - np.asarray(y, np.float32)
    p = t * t
    acc = p[..., 0]
    for i in range(1, p.shape[-1]):
        acc = acc + p[..., i]
    assert acc.dtype == np.float32
    return acc


@functools.lru_cache(maxsize=None)
def differing_rows(n, d, d2, M):
    """Per sub-quantizer: rows of the tied case whose code depends on the summation order."""
    c = R.tied_case(n, d, d2, M, R.SEED)
    xp = R.rotate(R.center(c.x), c.A)
    return (R.codes(xp, c.cb) != R.codes_by(ltr_np, xp, c.cb)).sum(0)


@pytest.mark.parametrize("dsub", [4, 6, 8, 12, 16, 24, 32, 48, 64])
def test_tied_codes_depend_on_the_order(dsub):
    diff = differing_rows(1100, 2 * dsub, 2 * dsub, 2)
    print(f"dsub {dsub}: rows that differ per sub-quantizer, of 1100: {diff.tolist()}")
    assert (diff >= MIN_DIFFER).all()


@pytest.mark.parametrize("shape", [s for s in R.ASSIGN_SHAPES + R.TIED_ONLY_SHAPES if s[2] // s[3] >= 4 and s[0] >= 300],
                         ids=str)
def test_tied_gpu_cases_depend_on_the_order(shape):
    """The same condition on the very arrays tests/test_gpu_opq_assign.py hands to the kernel."""
    diff = differing_rows(*shape)
    print(f"{shape}: rows that differ per sub-quantizer: {diff.tolist()}")
    assert (diff >= MIN_DIFFER).all()


@pytest.mark.parametrize("dsub", [1, 2, 3])
def test_orders_coincide_up_to_dsub_3(dsub):
    """(p0 + p1) + (p2 + 0) is the left-to-right sum: at dsub <= 3 the tied cases cannot tell the
    orders apart (they still check the first-minimum rule among exact ties), and this says so."""
    assert (differing_rows(1100, 3 * dsub, 3 * dsub, 3) == 0).all()


@pytest.mark.parametrize("kind", ["random", "tied"])
@pytest.mark.parametrize("shape", [(1025, 18, 18, 3), (300, 50, 48, 3), (37, 3, 3, 1)], ids=str)
def test_codes_are_the_oracle_encoder_s(kind, shape):
    n, d, d2, M = shape
    c = R.CASES[kind](n, d, d2, M, R.SEED)
    xp = R.rotate(R.center(c.x), c.A)
    np.testing.assert_array_equal(R.codes(xp, c.cb), ref_encode(xp, c.cb))


def test_tied_construction():
    n, d, d2, M = 1025, 20, 18, 3
    c = R.tied_case(n, d, d2, M, R.SEED)
    m32 = R.mean32(c.x)
    assert (m32 != 0).all() and len(np.unique(m32)) > d // 2  # a mean of its own per column
    xp = R.rotate(R.center(c.x), c.A).reshape(n, M, d2 // M)
    assert (xp == xp[:, :, :1]).all() and len(np.unique(xp[:, 0, 0])) > n // 2
    x64, cb64 = xp.astype(np.float64), c.cb.astype(np.float64)
    for m in range(M):  # every centroid has a twin: the same components in another order, in another slot
        _, inv, cnt = np.unique(np.sort(c.cb[m], axis=1), axis=0, return_inverse=True, return_counts=True)
        assert len(cnt) == 128 and (cnt == 2).all()
        pair = np.argsort(np.ravel(inv), kind="stable").reshape(128, 2)
        assert (c.cb[m][pair[:, 0]] != c.cb[m][pair[:, 1]]).any(1).sum() > 100
        # a row's two distances are sums of the same squares: one number once the order is fixed
        sq = np.sort((x64[:, m, None, :] - cb64[m][None]) ** 2, axis=-1).sum(-1)
        np.testing.assert_array_equal(sq[:, pair[:, 0]], sq[:, pair[:, 1]])


def test_random_rows_have_a_mean_off_the_grid():
    c = R.random_case(1100, 24, 16, 4, R.SEED)
    m32 = R.mean32(c.x)
    assert (np.abs(m32) >= 0.05).all()
    assert (c.x / R.GRID == np.round(c.x / R.GRID)).all() and (m32 / R.GRID != np.round(m32 / R.GRID)).any()
    assert not np.array_equal(R.center(c.x), c.x)


def test_mean32_is_one_rounding_of_the_exact_mean():
    from fractions import Fraction

    c = R.random_case(37, 5, 4, 2, R.SEED)
    got = R.mean32(c.x)
    for j in range(5):
        exact = sum(Fraction(float(v)) for v in c.x[:, j])  # the grid sum, exactly
        assert got[j] == np.float32(float(exact) / 37)  # float(exact) is exact: 37 grid values
        # any order of the fp64 additions gives that sum
        assert float(exact) == float(np.cumsum(c.x[::-1, j].astype(np.float64))[-1]) == c.x[:, j].astype(np.float64).sum()


def test_lloyd_against_a_float64_loop():
    rng = np.random.default_rng(3)
    n, M, dsub = 40, 2, 3
    xp = rng.standard_normal((n, M * dsub)).astype(np.float32)
    cb = rng.standard_normal((M, 256, dsub)).astype(np.float32)
    cd = rng.integers(0, 5, (n, M)).astype(np.uint8)  # centroids 5 .. 255 stay empty
    want = cb.copy()
    for m in range(M):
        for j in range(5):
            s, cnt = [0.0] * dsub, 0
            for r in range(n):
                if cd[r, m] == j:
                    cnt += 1
                    for t in range(dsub):
                        s[t] += float(xp[r, m * dsub + t])
            if cnt:
                want[m, j] = [np.float32(v / cnt) for v in s]
    got = R.lloyd(xp, cb, cd)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[:, 5:], cb[:, 5:])


def test_iterate_threads_its_steps():
    n, d, d2, M = 300, 10, 8, 2
    c = R.random_case(n, d, d2, M, R.SEED)
    init = np.concatenate([np.random.default_rng(m).choice(n, 256, replace=False) for m in range(M)]).astype(np.int64)
    r = R.iterate(c.x, c.A, 2, M, init=init, chunks=2)
    xp = R.rotate(R.center(c.x), c.A)
    cb = R.gather_init(xp, init, M)
    np.testing.assert_array_equal(cb[1, 7], xp[init[256 + 7], 4:8])
    for _ in range(2):
        cb = R.lloyd(xp, cb, R.codes(xp, cb))
    np.testing.assert_array_equal(r.cb, cb)
    np.testing.assert_array_equal(r.codes, R.codes(xp, cb))
    rec = R.decode(cb, r.codes)
    np.testing.assert_array_equal(rec[5, 4:8], cb[1, r.codes[5, 1]])
    np.testing.assert_allclose(r.cross, np.einsum("ri,rj->ij", r.xt.astype(np.float64), rec.astype(np.float64)), rtol=1e-12,
                               atol=1e-9)
    k = n + 2
    np.testing.assert_array_equal(r.bound, k * R.U / (1 - k * R.U) * (np.abs(r.xt).astype(np.float64).T @ np.abs(rec)))
    # an fp32 evaluation of the same sums sits inside the bound
    c32 = np.zeros((d, d2), np.float32)
    for row in range(n):
        c32 = c32 + np.outer(r.xt[row], rec[row])
    R.assert_cross(c32, r)


def test_get_codes_is_bound_and_null_safe():
    from faiss_amd import _lib

    L = _lib.load()
    assert L.ivfpq_opq_get_codes.argtypes == [_lib.c_handle, _lib.c_u8p]
    assert L.ivfpq_opq_get_codes(None, None) != 0 and L.ivfpq_last_error()
