"""Two arithmetic edges of the float16 lookup tables (k_scan_lists_h), bit for bit
against tests/ivfpq_f16lut_ref.py; the documented rule is one IEEE rounding to half, nearest even, of the
entry clamped to +-65504, and an exact conversion back when the entry is added.

Half-subnormal entries (0 < |x| < 2^-14).  The kernel converts with v_cvt_f16_f32 and adds with a hand-written
v_fma_mix_f32; either could flush half denormals under the mode the library is built with.  One list around
the origin, dis0 = 0 and a codebook of size 2^-16 make every key a sum of entries of which more than half are
non-zero half subnormals.  Held on the CPU first: a reference that flushes them to zero returns other top-10
labels for every query, and the fp32 tables give other distances.

Ties and the clamp edge.  Real-valued random data never holds an exact tie.  Here the table is written by hand
through set_trained (inner product: dsub = 1 and a query of ones make the entry the negated codebook value;
L2: the query and the centroid at the origin make it |c|^2, a sum of four squares), one row per entry, so that
every entry decides a rank: 2049, 2051, 4098 and 4102 round to even (2048, 2052, 4096, 4104), 65519.996
rounds down to 65504, 65520 -- which a bare conversion would round to inf -- and everything above clamp to
65504, and so do the negatives.  Neighbouring exact entries (2048, 2050, 2052, ...) fix the ranks on both
sides; equal keys rank by label.  No row has a zero key (asserted): the sign of a zero distance is no part of
the rule, and the scan's differs from numpy's for the inner product of a query with the origin."""
import functools

import numpy as np
import pytest

import faiss_amd as faiss
import ivfpq_f16lut_ref as RH

F = np.float32
TINY = F(2.0 ** -14)  # the smallest normal half


def gpu_index(d, M, ip, cent, cb, codes, ids):
    ix = faiss.GpuIndexIVFPQ(None, d, 1, M, 8, faiss.METRIC_INNER_PRODUCT if ip else faiss.METRIC_L2, 0)
    ix.set_trained(cent, cb)
    ix.add_preencoded(np.zeros(len(ids), np.int64), codes, ids)
    ix.use_float16_lut = True
    ix.nprobe = 1
    return ix


def check(got, ref, msg):
    np.testing.assert_array_equal(got[1], ref[1], err_msg=msg)
    np.testing.assert_array_equal(got[0].view(np.uint32), ref[0].view(np.uint32), err_msg=msg)


def clean(ix, e0, rs0):
    assert ix.error_count() == e0
    assert ix.repair_stats() == rs0


# ---------------------------------------------------------------- half-subnormal entries
NQ, NROWS = 9, 700  # two chunks of 256 rows and a tail


@functools.lru_cache(maxsize=None)
def subnormal_case(M, ip):
    rng = np.random.default_rng(300 + M + ip)
    d = 2 * M
    cent = np.zeros((1, d), F)
    cb = (rng.standard_normal((M, 256, 2)) * 2.0 ** -16).astype(F)
    xq = rng.standard_normal((NQ, d)).astype(F)
    codes = rng.integers(0, 256, (NROWS, M), dtype=np.uint8)
    ids = np.sort(rng.permutation(10 * NROWS)[:NROWS]).astype(np.int64)
    probes, dis0 = np.zeros((NQ, 1), np.int64), np.zeros((NQ, 1), F)
    args = (xq, 100, probes, dis0, cent, cb, [codes], [ids], ip)
    ref, flushed, fp32 = RH.search_preassigned(*args), RH.search_preassigned(*args, flush=True), \
        RH.search_preassigned(*args, half=False)
    return dict(d=d, cent=cent, cb=cb, xq=xq, codes=codes, ids=ids, probes=probes, dis0=dis0, ref=ref,
                flushed=flushed, fp32=fp32)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("M", [8, 32])
def test_subnormal_case_preconditions(M, ip):
    """On the CPU: what makes the GPU case below mean what it claims."""
    from oracle import oracle as O

    c = subnormal_case(M, ip)
    T3 = O.ip_table(c["xq"], c["cb"])
    T1 = O.precompute_T1(c["cent"], c["cb"])[0]
    for q in range(NQ):
        h = RH.entries(RH.lut32(T3[q], T1, ip))
        sub = (h != 0) & (np.abs(h) < TINY)
        assert 2 * sub.sum() >= h.size, (q, sub.mean())
        assert not np.array_equal(c["ref"][1][q, :10], c["flushed"][1][q, :10])
    assert not np.array_equal(c["ref"][0], c["fp32"][0])
    if not ip:  # dis0 is given as 0 and the centroid is the origin: the keys are sums of entries alone
        assert not c["cent"].any() and not c["dis0"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("M", [8, 32])
def test_subnormal_entries_are_kept(M, ip):
    c = subnormal_case(M, ip)
    ix = gpu_index(c["d"], M, ip, c["cent"], c["cb"], c["codes"], c["ids"])
    e0, rs0 = ix.error_count(), ix.repair_stats()
    for k in (10, 100):  # G = 4; G = 2 (M = 8) and G = 4 (M = 32)
        got = ix.search_preassigned(c["xq"], k, c["probes"], None if ip else c["dis0"])
        check(got, RH.prefix(c["ref"], k), f"k={k}")
    clean(ix, e0, rs0)


# ---------------------------------------------------------------- ties and the clamp edge
BELOW_65520 = float(np.nextafter(F(65520), F(0)))  # 65519.996
EDGES = [2049.0, 2051.0, 4098.0, 4102.0, BELOW_65520, 65520.0, 65536.0, 70000.0, 1.0e6]
ROUNDED = [2048.0, 2052.0, 4096.0, 4104.0, 65504.0, 65504.0, 65504.0, 65504.0, 65504.0]
EXACT = [0.0, 1.0, 2046.0, 2048.0, 2050.0, 2052.0, 2054.0, 4092.0, 4096.0, 4100.0, 4104.0, 4108.0, 65472.0, 65504.0]
TIE_M, TIE_K = 8, 128  # more than the rows of either case


def four_squares(n):
    """Four integers whose squares sum to n."""
    r = int(np.sqrt(n))
    for a in range(r, -1, -1):
        for b in range(int(np.sqrt(n - a * a)), -1, -1):
            rest = n - a * a - b * b
            for c in range(int(np.sqrt(rest)), -1, -1):
                e = int(round(np.sqrt(rest - c * c)))
                if e * e == rest - c * c:
                    return a, b, c, e
    raise ValueError(n)


@functools.lru_cache(maxsize=None)
def tie_case(ip):
    """Sub-quantizers 0 and M - 1 hold the table, the others zeros; row r has the code of one entry in one
    of the two and code 0 (entry 0) everywhere else."""
    M = TIE_M
    if ip:
        vals = np.asarray([0.0] + [s * v for v in EXACT[1:] + EDGES for s in (1, -1)], F)
        d = M
        cb = np.zeros((M, 256, 1), F)
        cb[0, :len(vals), 0] = cb[M - 1, :len(vals), 0] = -vals  # entry = -<x, c>
        xq = np.zeros((5, d), F)
        xq[0] = 1
        xq[1] = -1
        xq[2, 0], xq[2, M - 1] = 1, 0.5
        xq[3], xq[4] = 0.5, 2
    else:
        vals = np.asarray([v for v in EXACT + EDGES if v == int(v)], F)
        d = 4 * M
        cb = np.zeros((M, 256, 4), F)
        for j, v in enumerate(vals):
            cb[0, j] = cb[M - 1, j] = four_squares(int(v))
        xq = np.zeros((3, d), F)
        xq[1, 0], xq[2, 1] = 1, -0.5  # entries |c|^2 - 2 <x, c>: off the hand-made values
    n = len(vals) - 1  # entry 0 is 0, the code of the other sub-quantizers, and has no row of its own
    codes = np.zeros((2 * n, M), np.uint8)
    codes[:n, 0] = codes[n:, M - 1] = 1 + np.arange(n)
    ids = 7 + 3 * np.random.default_rng(9).permutation(2 * n).astype(np.int64)
    by_id = np.argsort(ids)  # device lists are label-sorted
    cent = np.zeros((1, d), F)
    probes, dis0 = np.zeros((len(xq), 1), np.int64), np.zeros((len(xq), 1), F)
    args = (xq, TIE_K, probes, dis0, cent, cb, [codes[by_id]], [ids[by_id]], ip)
    return dict(d=d, vals=vals, cent=cent, cb=cb, xq=xq, codes=codes, ids=ids, probes=probes, dis0=dis0,
                ref=RH.search_preassigned(*args), fp32=RH.search_preassigned(*args, half=False))


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
def test_tie_case_preconditions(ip):
    """On the CPU: query 0's fp32 entries are the hand-made values; the reference rounds them
    as the docstring says; every row's key is its entry."""
    from oracle import oracle as O

    c = tie_case(ip)
    np.testing.assert_array_equal(RH.entries(np.asarray(EDGES, F)), np.asarray(ROUNDED, F))
    np.testing.assert_array_equal(RH.entries(-np.asarray(EDGES, F)), -np.asarray(ROUNDED, F))
    np.testing.assert_array_equal(RH.entries(np.asarray(EXACT, F)), np.asarray(EXACT, F))
    assert BELOW_65520 < 65520 and F(BELOW_65520) == BELOW_65520 and f"{BELOW_65520:.3f}" == "65519.996"
    n = len(c["vals"])
    assert c["vals"][0] == 0 and 2 * (n - 1) + 5 <= TIE_K
    lut = RH.lut32(O.ip_table(c["xq"][:1], c["cb"])[0], O.precompute_T1(c["cent"], c["cb"])[0], ip)
    for m in (0, TIE_M - 1):
        np.testing.assert_array_equal(lut[m, :n], c["vals"])
    assert not lut[1:TIE_M - 1].any() and not lut[:, n:].any()
    for v in EDGES if ip else [v for v in EDGES if v == int(v)]:
        assert (c["vals"] == F(v)).sum() == 1 and (not ip or (c["vals"] == F(-v)).sum() == 1)
    D, I = c["ref"]
    want = RH.entries(np.concatenate([c["vals"][1:], c["vals"][1:]]))
    order = np.lexsort((c["ids"], want))
    n2 = len(want)
    np.testing.assert_array_equal(I[0, :n2], c["ids"][order])
    np.testing.assert_array_equal(D[0, :n2], -want[order] if ip else want[order])
    assert (I[0, n2:] == -1).all() and np.isfinite(D[0, :n2]).all()
    assert (c["ref"][0][c["ref"][1] >= 0] != 0).all()  # no key is zero: the sign of a zero distance is not pinned
    assert not np.array_equal(c["ref"][1], c["fp32"][1])


@pytest.mark.gpu
@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
def test_ties_round_to_even_and_the_clamp_edge(ip):
    c = tie_case(ip)
    ix = gpu_index(c["d"], TIE_M, ip, c["cent"], c["cb"], c["codes"], c["ids"])
    e0, rs0 = ix.error_count(), ix.repair_stats()
    n2 = len(c["ids"])
    for k in (1, 10, 64, n2, n2 + 5, TIE_K):  # every row is returned from n2 on; beyond it the result is padded
        got = ix.search_preassigned(c["xq"], k, c["probes"], None if ip else c["dis0"])
        check(got, RH.prefix(c["ref"], k), f"k={k}")
    clean(ix, e0, rs0)
