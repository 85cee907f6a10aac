"""One ivfpq_opq handle through many calls, as OPQMatrix.train_device drives it, against
tests/opq_ref.py: several Lloyd steps from a cold start, a hot-started second round, the rows
replaced on the same handle, rows taken from HBM on a stream of their own, and the errors a
caller can provoke.  ``random`` rows with a non-zero mean per column (opq_ref.random_case);
codebooks and codes are compared bit for bit, the cross within opq_ref.cross64's bound.
"""
import functools

import numpy as np
import pytest

import opq_ref as R
from faiss_amd.transform import opq_plan

pytestmark = pytest.mark.gpu

SHAPE = (1100, 24, 16, 4)


def rows(n, d, d2, M, seed=R.SEED):
    """(x, A, init): init draws 256 distinct rows per sub-quantizer, as _pq_kmeans does."""
    c = R.random_case(n, d, d2, M, seed)
    rng = np.random.default_rng([seed, n, 2])
    init = np.concatenate([rng.choice(n, 256, replace=False) for _ in range(M)]).astype(np.int64)
    return c.x, c.A, init


def chunks_of(n, d, d2):
    return opq_plan(n, d, d2)["chunks"]


def assert_round(h, cross, ref):
    np.testing.assert_array_equal(h.codebook(), ref.cb)
    np.testing.assert_array_equal(h.codes(), ref.codes)
    R.assert_cross(cross, ref)


@functools.lru_cache(maxsize=None)
def two_rounds():
    """The reference of a cold start with three Lloyd steps, then a hot start with two under another rotation."""
    n, d, d2, M = SHAPE
    x, A, init = rows(*SHAPE)
    _, _, A2 = R.signed_perm(np.random.default_rng(99), d, d2)
    first = R.iterate(x, A, 3, M, init=init, chunks=chunks_of(n, d, d2))
    second = R.iterate(x, A2, 2, M, cb=first.cb, chunks=chunks_of(n, d, d2))
    return x, A, init, A2, first, second


def test_three_lloyd_steps_from_a_cold_start():
    _, d, d2, M = SHAPE
    x, A, init, _, first, _ = two_rounds()
    assert len(np.unique(first.codes[:, 0])) > 128 and not np.array_equal(first.cb, R.gather_init(first.xp, init, M))
    with R.Handle(d, d2, M) as h:
        h.set_rows(x)
        assert_round(h, h.iterate(A, 3, init), first)


def test_hot_start_continues_from_the_kept_codebook():
    _, d, d2, M = SHAPE
    x, A, init, A2, first, second = two_rounds()
    assert not np.array_equal(A, A2) and not np.array_equal(first.cb, second.cb)
    with R.Handle(d, d2, M) as h:
        h.set_rows(x)
        h.iterate(A, 3, init)
        kept = h.codebook()
        cross = h.iterate(A2, 2, None)
        assert_round(h, cross, second)
    with R.Handle(d, d2, M) as g:  # the codebook carried by hand into a fresh handle: identical bits
        g.set_rows(x)
        g.set_codebook(kept)
        np.testing.assert_array_equal(g.iterate(A2, 2, None), cross)
        assert_round(g, cross, second)


def test_rows_replaced_on_the_same_handle():
    """300 rows, then 1100 (every buffer regrown, the pass scratch carved again), then 300 other rows
    with another mean: each round is the reference's for the rows then held."""
    d, d2, M = SHAPE[1:]
    with R.Handle(d, d2, M) as h:
        means = []
        for n, seed in [(300, R.SEED), (1100, R.SEED), (300, R.SEED + 1)]:
            x, A, init = rows(n, d, d2, M, seed)
            means.append(R.mean32(x))
            h.set_rows(x)
            with pytest.raises(RuntimeError, match="no codes yet"):  # the codes of the rows before are gone
                h.codes()
            assert_round(h, h.iterate(A, 1, init), R.iterate(x, A, 1, M, init=init, chunks=chunks_of(n, d, d2)))
        assert (means[0] != means[2]).all() and np.abs(means[0] - means[2]).max() > 1  # (the third mean is its own)


def test_rows_from_hbm_on_a_stream_of_their_own():
    import torch

    _, d, d2, M = SHAPE
    x, A, init, _, first, _ = two_rounds()
    host = torch.from_numpy(x.copy()).pin_memory()
    side = torch.cuda.Stream()
    with R.Handle(d, d2, M) as h:
        with torch.cuda.stream(side):  # produced on the side stream and handed over with no synchronisation between
            t = host.to("cuda", non_blocking=True) * 2.0 - host.to("cuda", non_blocking=True)
            h.set_rows_device(t, side.cuda_stream)
        assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
        assert_round(h, h.iterate(A, 3, init), first)
    side.synchronize()
    np.testing.assert_array_equal(t.cpu().numpy(), x)  # (2 x - x is x exactly)


def test_errors_leave_the_handle_usable():
    n, d, d2, M = 300, 24, 16, 4
    x, A, init = rows(n, d, d2, M)
    with R.Handle(d, d2, M) as h:
        with pytest.raises(RuntimeError, match="no training rows"):
            h.iterate(A, 1, init)
        with pytest.raises(RuntimeError, match="no codes yet"):
            h.codes()
        h.set_rows(x)
        with pytest.raises(RuntimeError, match="no codebook"):
            h.iterate(A, 1, None)
        bad = init.copy()
        bad[M * 256 - 1] = n
        with pytest.raises(RuntimeError, match=r"init_rows\[1023\] is outside"):
            h.iterate(A, 1, bad)
        with pytest.raises(RuntimeError, match="no codebook"):  # the rejected call set nothing
            h.iterate(A, 0, None)
        assert_round(h, h.iterate(A, 1, init), R.iterate(x, A, 1, M, init=init, chunks=chunks_of(n, d, d2)))
