"""Shared reference of the resident OPQ trainer's tests (tests/test_gpu_opq_assign.py,
tests/test_gpu_opq_rounds.py; its own CPU checks are tests/test_opq_ref_cpu.py): one
``ivfpq_opq_iterate`` restated in plain numpy so that every device result is known in advance,
bit for bit except the cross matrix, which has a derived bound.

Rows lie on a dyadic grid (multiples of 2^-10, |x| < 2^10): their fp64 column sums are exact in
any order, so ``mean32`` is k_pca_colsum / k_pca_mean's ``(float)(s / (double)n)`` whatever the
chunking.  A is the first d2 rows of a signed permutation, so a row of xp = xt A^T is an exact
signed selection of xt (the other d - 1 products of each sum are zeros).  The codes are the first
argmin of ``tree_np`` (tests/indexpq_ref.py: Faiss's fvec_L2sqr order in float32).  The Lloyd
update is one fp64 chain per (centroid, dimension) over the members in ascending row order,
divided in fp64 and rounded to fp32 once; empty centroids stay (k_km_mean).

Two data sets, both with a non-zero column mean that differs per column:

``random``  real-valued rows on the grid, whose mean32 is not a grid value (xt = x - mean32 is
            rounded), codebooks drawn from the rotated rows plus noise.
``tied``    built so that the fp32 summation order decides the codes.  For every m each row's
            sub-vector of xp is one value repeated dsub times; the 256 centroids are 128 random
            vectors and 128 twins, a twin being a random coordinate permutation of its partner,
            scattered over the slots.  A row's distances to a centroid and to its twin are sums
            of the same dsub squares in two orders: equal in exact arithmetic, different only by
            fp32 rounding.  xp is built first with columns that sum to exactly 0 (z, -z and a
            zero row where n is odd), mapped back through A, and a grid offset is added per
            column: mean32 is then that offset exactly and the kernel reads xt = x - mean32
            exactly in the constructed form (``tied`` asserts both).
"""
import ctypes
from types import SimpleNamespace

import numpy as np

from indexpq_ref import KIND_L2, tree_np

GRID = 2.0 ** -10
U = 2.0 ** -24  # the unit roundoff of fp32


def signed_perm(rng, d, d2):
    """(cols, signs, A): A [d2][d] has A[j][cols[j]] = signs[j] and zeros elsewhere."""
    cols = rng.permutation(d)[:d2]
    signs = rng.choice([-1.0, 1.0], d2).astype(np.float32)
    A = np.zeros((d2, d), np.float32)
    A[np.arange(d2), cols] = signs
    return cols, signs, A


def on_grid(a):
    return (np.round(np.asarray(a, np.float64) / GRID) * GRID).astype(np.float32)


def offsets(rng, d):
    """A non-zero grid offset per column, all different in general, in +-[1/8, 3]."""
    return on_grid(rng.choice([-1.0, 1.0], d) * rng.uniform(0.125, 3.0, d))


def mean32(x):
    assert x.dtype == np.float32
    return (x.astype(np.float64).sum(0) / x.shape[0]).astype(np.float32)


def center(x):
    xt = x - mean32(x)[None, :]
    assert xt.dtype == np.float32
    return xt


def rotate(xt, A):
    """xt A^T for a signed-permutation A: the selection itself, no sum."""
    cols = np.argmax(np.abs(A), axis=1)
    signs = A[np.arange(A.shape[0]), cols]
    assert (np.abs(A).sum(1) == 1).all() and (np.abs(signs) == 1).all()
    return np.ascontiguousarray(xt[:, cols] * signs[None, :])


def codes_by(dist, xp, cb):
    """[n][M] uint8: the first argmin over the 256 centroids of dist(x_m, c) (dist: tree_np's signature)."""
    M, _, dsub = cb.shape
    out = np.empty((xp.shape[0], M), np.uint8)
    for m in range(M):
        xs = xp[:, m * dsub:(m + 1) * dsub]
        for r in range(0, xp.shape[0], 256):
            out[r:r + 256, m] = np.argmin(dist(xs[r:r + 256, None, :], cb[m][None], KIND_L2), axis=1)
    return out


def codes(xp, cb):
    return codes_by(tree_np, xp, cb)


def gather_init(xp, init, M):
    """The codebook ivfpq_opq_iterate starts from: centroid (m, j) is sub-vector m of row init[m 256 + j]."""
    dsub = xp.shape[1] // M
    return np.stack([xp[init[m * 256:(m + 1) * 256], m * dsub:(m + 1) * dsub] for m in range(M)]).astype(np.float32)


def lloyd(xp, cb, cd):
    """One update: per (m, centroid) the sequential fp64 sum of the members in ascending row order."""
    M, _, dsub = cb.shape
    out = cb.copy()
    for m in range(M):
        xs = xp[:, m * dsub:(m + 1) * dsub].astype(np.float64)
        for j in np.unique(cd[:, m]):
            rows = xs[cd[:, m] == j]
            out[m, j] = (np.cumsum(rows, axis=0)[-1] / float(rows.shape[0])).astype(np.float32)
    return out


def decode(cb, cd):
    M = cb.shape[0]
    return np.concatenate([cb[m][cd[:, m]] for m in range(M)], axis=1)


def cross64(xt, rec, chunks):
    """(C, bound): C = xt^T rec in float64 and the elementwise forward-error bound of the same sums
    in fp32: gamma_k (|xt|^T |rec|), gamma_k = k u / (1 - k u), k = n + chunks (a length-n dot
    product in any association, then the chunk additions)."""
    a, b = xt.astype(np.float64), rec.astype(np.float64)
    k = xt.shape[0] + chunks
    return a.T @ b, (k * U / (1.0 - k * U)) * (np.abs(a).T @ np.abs(b))


def iterate(x, A, niter_pq, M, cb=None, init=None, chunks=1):
    """One ivfpq_opq_iterate over the rows x (as given to ivfpq_opq_set_rows): from the codebook cb,
    or from the rows init [M * 256] when given; chunks: the cross's row chunks (opq_plan)."""
    xt = center(x)
    xp = rotate(xt, A)
    if init is not None:
        cb = gather_init(xp, init, M)
    for _ in range(niter_pq):
        cb = lloyd(xp, cb, codes(xp, cb))
    cd = codes(xp, cb)
    C, bound = cross64(xt, decode(cb, cd), chunks)
    return SimpleNamespace(xt=xt, xp=xp, cb=cb, codes=cd, cross=C, bound=bound)


def random_case(n, d, d2, M, seed):
    rng = np.random.default_rng([seed, n, d, d2, M, 0])
    x = on_grid(4.0 * rng.standard_normal((n, d))) + offsets(rng, d)[None, :]
    _, _, A = signed_perm(rng, d, d2)
    xp = rotate(center(x), A)
    dsub = d2 // M
    cb = np.stack([xp[rng.choice(n, 256, replace=n < 256), m * dsub:(m + 1) * dsub] for m in range(M)])
    cb = (cb + 0.25 * rng.standard_normal(cb.shape)).astype(np.float32)
    return SimpleNamespace(x=np.ascontiguousarray(x), A=A, cb=cb)


def tied_case(n, d, d2, M, seed):
    rng = np.random.default_rng([seed, n, d, d2, M, 1])
    dsub = d2 // M
    half = n // 2

    def balanced(cols):  # [n][cols] on the grid, every column sums to exactly 0
        z = on_grid(4.0 * rng.standard_normal((half, cols)))
        return np.concatenate([z, -z, np.zeros((n % 2, cols), np.float32)])

    order = rng.permutation(n)
    xp = np.repeat(balanced(M), dsub, axis=1)[order]
    cols, signs, A = signed_perm(rng, d, d2)
    xt = balanced(d)[order]
    xt[:, cols] = xp * signs[None, :]
    off = offsets(rng, d)
    x = np.ascontiguousarray(xt + off[None, :])
    # what the kernels read is the construction itself: the mean is the offset, centring undoes it exactly
    assert x.dtype == np.float32 and np.array_equal(x.astype(np.float64), xt.astype(np.float64) + off.astype(np.float64))
    assert np.array_equal(mean32(x), off) and np.array_equal(center(x), xt) and np.array_equal(rotate(xt, A), xp)
    base = (4.0 * rng.standard_normal((M, 128, dsub))).astype(np.float32)
    twin = np.stack([np.stack([v[rng.permutation(dsub)] for v in base[m]]) for m in range(M)])
    cb = np.concatenate([base, twin], axis=1)
    cb = np.stack([cb[m][rng.permutation(256)] for m in range(M)])
    return SimpleNamespace(x=x, A=A, cb=np.ascontiguousarray(cb))


CASES = {"random": random_case, "tied": tied_case}
SEED = 11

# (n, d, d2, M) of tests/test_gpu_opq_assign.py, both data sets each; what a shape reaches:
ASSIGN_SHAPES = [
    (1100, 6, 3, 3),      # dsub 1, RPT 4: one full 1024-row pass, then a tile of 76 rows; M = 3; d < 8
    (1100, 9, 9, 3),      # dsub 3: tree_l2 is its tail alone; non-VEC cross
    (1025, 18, 18, 3),    # dsub 6: the 4-wide step and a tail of 2; a last tile of one row
    (300, 50, 48, 3),     # dsub 16, RPT 4 with the lanes' rows 2-4 past the tile
    (1100, 72, 72, 3),    # dsub 24, RPT 2: 512-row passes, a 76-row tile
    (600, 64, 64, 2),     # dsub 32, RPT 2, the second pass partly filled
    (1100, 100, 96, 2),   # dsub 48, RPT 1
    (1100, 128, 128, 2),  # dsub 64, RPT 1, the 64 KiB stage; the default plan: 5 chunks, the last of 76 rows
    (300, 96, 96, 1),     # dsub 96 > 64: launch_pq_encode_flat
    (1, 4, 4, 4),         # n = 1; VEC cross with d == 4
    (37, 3, 3, 1),        # d < 4, non-VEC
]
# dsub 2, 4, 8, 12: widths the integer-valued cases of test_gpu_opq_train.py reach; here with values that tie
TIED_ONLY_SHAPES = [(1100, 8, 6, 3), (1100, 12, 12, 3), (1100, 24, 16, 2), (1100, 40, 36, 3)]
# (n, d, d2, M, chunk_rows): the cross's chunking set by hand; 1024 at n = 1025 leaves a last chunk of one row
CHUNKED_SHAPES = [(1100, 24, 16, 4, 64), (1025, 24, 16, 4, 1024)]


# ---- the C-ABI handle the GPU tests drive -------------------------------------------------------

def _p(a, t):
    assert a.flags.c_contiguous
    return a.ctypes.data_as(t)


class Handle:
    """One ivfpq_opq handle; every call raises RuntimeError with the library's message on failure."""

    def __init__(self, d, d2, M):
        from faiss_amd import _lib

        self._lib, self.L, self.h, self.shape, self.n = _lib, _lib.load(), _lib.c_handle(), (d, d2, M), 0
        _lib.check(self.L.ivfpq_opq_create(d, d2, M, 0, ctypes.byref(self.h)))

    def close(self):
        if self.h:
            self.L.ivfpq_opq_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_rows(self, x):
        assert x.dtype == np.float32 and x.shape[1] == self.shape[0]
        self._lib.check(self.L.ivfpq_opq_set_rows(self.h, x.shape[0], _p(x, self._lib.c_f32p)))
        self.n = x.shape[0]

    def set_rows_device(self, t, stream):
        self._lib.check(self.L.ivfpq_opq_set_rows_device(self.h, t.shape[0], t.data_ptr(), ctypes.c_void_p(stream)))
        self.n = t.shape[0]

    def set_codebook(self, cb):
        d, d2, M = self.shape
        assert cb.dtype == np.float32 and cb.shape == (M, 256, d2 // M)
        self._lib.check(self.L.ivfpq_opq_set_codebook(self.h, _p(cb, self._lib.c_f32p)))

    def iterate(self, A, niter_pq, init=None):
        d, d2, _ = self.shape
        cross = np.empty((d, d2), np.float32)
        self._lib.check(self.L.ivfpq_opq_iterate(self.h, _p(A, self._lib.c_f32p), niter_pq,
                                                 None if init is None else _p(init, self._lib.c_i64p),
                                                 _p(cross, self._lib.c_f32p)))
        return cross

    def codebook(self):
        d, d2, M = self.shape
        out = np.empty((M, 256, d2 // M), np.float32)
        self._lib.check(self.L.ivfpq_opq_get_codebook(self.h, _p(out, self._lib.c_f32p)))
        return out

    def codes(self):
        out = np.full((max(self.n, 1), self.shape[2]), 255, np.uint8)
        self._lib.check(self.L.ivfpq_opq_get_codes(self.h, _p(out, self._lib.c_u8p)))
        return out[:self.n]


def assert_cross(got, ref):
    err = np.abs(got.astype(np.float64) - ref.cross)
    assert (err <= ref.bound).all(), f"cross off by {(err - ref.bound).max():.3g} beyond the bound {ref.bound.max():.3g}"
