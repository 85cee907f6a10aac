"""k_opq_assign at every instantiated width, k_opq_center and k_opq_cross, on real values, against
tests/opq_ref.py (``ivfpq_opq_set_rows``, ``ivfpq_opq_set_codebook``, ``ivfpq_opq_iterate(A, 0)``).

Every case asserts the codes of ``ivfpq_opq_get_codes`` bit for bit and, for the ``random`` data, the
cross matrix within the derived bound of opq_ref.cross64.  The ``random`` rows have a non-zero
mean of their own per column, off the grid, so a wrong mean, a wrong mean index or a stale mean
moves every xt and with it the codes; the ``tied`` rows make the fp32 summation order of tree_l2
decide the codes (tests/test_opq_ref_cpu.py holds the condition).  Shapes and what each reaches:
opq_ref.ASSIGN_SHAPES, TIED_ONLY_SHAPES, CHUNKED_SHAPES.
"""
import functools

import numpy as np
import pytest

import opq_ref as R
from faiss_amd.transform import opq_plan, opq_set_chunk_rows

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(kind, n, d, d2, M):
    c = R.CASES[kind](n, d, d2, M, R.SEED)
    for a in (c.x, c.A, c.cb):
        a.setflags(write=False)
    return c


def run(kind, n, d, d2, M, cross=True):
    c = case(kind, n, d, d2, M)
    chunks = opq_plan(n, d, d2)["chunks"]
    ref = R.iterate(c.x, c.A, 0, M, cb=c.cb, chunks=chunks)
    with R.Handle(d, d2, M) as h:
        h.set_rows(c.x)
        h.set_codebook(c.cb)
        got_cross = h.iterate(c.A, 0)
        got = h.codes()
    np.testing.assert_array_equal(got, ref.codes)
    if cross:
        R.assert_cross(got_cross, ref)
    return chunks


@pytest.mark.parametrize("kind", ["random", "tied"])
@pytest.mark.parametrize("shape", R.ASSIGN_SHAPES, ids=str)
def test_assign_and_cross(shape, kind):
    chunks = run(kind, *shape)
    if shape == (1100, 128, 128, 2):
        assert chunks == 5 and opq_plan(*shape[:3])["chunk_rows"] == 256  # the last chunk has 76 rows


@pytest.mark.parametrize("shape", R.TIED_ONLY_SHAPES, ids=str)
def test_assign_tied_at_the_widths_the_integer_cases_reach(shape):
    run("tied", *shape, cross=False)


@pytest.fixture
def chunked(request):
    n, d, d2, M, rows = request.param
    opq_set_chunk_rows(rows)
    yield n, d, d2, M, rows
    opq_set_chunk_rows(0)


@pytest.mark.parametrize("chunked", R.CHUNKED_SHAPES, indirect=True, ids=str)
def test_cross_with_a_set_chunk_length(chunked):
    n, d, d2, M, rows = chunked
    assert run("random", n, d, d2, M) == -(-n // rows)
