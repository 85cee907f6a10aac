"""IndexPQ on the GPU, path by path: the scan loop over several passes, every table and
encoder width, every table blocking, the k and nb boundaries, many partial lists, crafted
keys that drive the admission logic and the candidate queue to their limits.

The reference is tests/indexpq_ref.py: Faiss's IndexPQ::search restated in numpy (tables in
fvec order, ``acc = 0; acc += tab[m][code[m]]`` in ascending m in float32, the k best by
(key, label)).  Every comparison is ``assert_array_equal`` on D and I.  Quantizers are
installed with ``set_trained``; data is standard normal, so sums have mixed signs.

A test that relies on a geometry asserts it first through ``plan`` (ivfpq_pq_debug_plan):
a chunk of queries is scanned by ``ranges`` workgroups per query group, each over ``rows``
rows in passes of ``pass_rows(k)`` (2048 at k <= 64, 1024 above), and leaves S = 4 * ranges
partial lists per query.  With few queries a range is a single pass at k <= 64 unless
nb > 2048 * 12288 / (4 k); thousands of queries (>= 2049: at most two ranges) are what makes
a workgroup loop, which is how the production shapes run.
"""
import numpy as np
import pytest

import faiss_amd as faiss
from indexpq_ref import (IP, L2, pass_rows, plan, ref_encode, ref_order, ref_sums, ref_tables, ref_topk, sums64)

pytestmark = pytest.mark.gpu

METRICS = pytest.mark.parametrize("metric", [L2, IP], ids=["l2", "ip"])


def normal(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


def make_index(d, M, metric, cb, xb=None):
    ix = faiss.IndexPQ(d, M, 8, metric)
    ix.set_trained(cb)
    if xb is not None:
        ix.add(xb)
    return ix


def check(D, I, acc, k, metric, order=None):
    Dr, Ir = ref_topk(acc, k, metric, order)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)


def encoded(d, M, metric, seed, nb, nq):
    """A seeded codebook, base and queries; the index over the base, its codes checked."""
    cb = normal(seed, M, 256, d // M)
    xb = normal(seed + 1, nb, d)
    xq = normal(seed + 2, nq, d)
    ix = make_index(d, M, metric, cb, xb)
    codes = ref_encode(xb, cb)
    np.testing.assert_array_equal(ix.codes.reshape(nb, M), codes)
    return ix, cb, xq, codes


# ------------------------------------- a. several passes at k <= 64, query chunks
NB_A = 2 * 2048 + 777
NQ_A = 4100
KS_A = (1, 10, 64)


def assert_one_range_of_three_passes(M, k):
    p = plan(M, k, NQ_A, NB_A)
    assert (p.chunk, p.ranges, p.rows) == (4096, 1, 6144)  # passes of 2048, 2048 and 777 rows
    assert p.rows // pass_rows(k) >= 2
    assert plan(M, k, NQ_A - p.chunk, NB_A).ranges == 3  # the last 4 queries: a second chunk, single passes


@METRICS
@pytest.mark.parametrize("M", [8, 16])
def test_multipass_with_resident_table(M, metric):
    """M = 8 / 16 is one table block: it is loaded in the first pass only and stays in LDS."""
    d = 32
    ix, cb, xq, codes = encoded(d, M, metric, 100 + M, NB_A, NQ_A)
    acc = ref_sums(ref_tables(xq, cb, metric), codes)
    order = ref_order(acc, max(KS_A), metric)
    for k in KS_A:
        assert_one_range_of_three_passes(M, k)
        D, I = ix.search(xq, k)
        check(D, I, acc, k, metric, order)
        # 513 query groups: one range of two passes and a ragged range of one
        p = plan(M, k, 2049, NB_A)
        assert (p.chunk, p.ranges, p.rows) == (2049, 2, 4096)
        D, I = ix.search(xq[:2049], k)
        check(D, I, acc[:2049], k, metric, order[:2049])
    if M == 8:
        import torch

        Dd, Id = ix.search_device(torch.from_numpy(xq).cuda(), 10)
        torch.cuda.synchronize()
        check(Dd.cpu().numpy(), Id.cpu().numpy(), acc, 10, metric, order)


@METRICS
def test_multipass_with_reloaded_table(metric):
    """M = 32 is two table blocks: both are loaded again in every pass."""
    d, M, k = 64, 32, 10
    assert_one_range_of_three_passes(M, k)
    ix, cb, xq, codes = encoded(d, M, metric, 140, NB_A, NQ_A)
    acc = ref_sums(ref_tables(xq, cb, metric), codes)
    D, I = ix.search(xq, k)
    check(D, I, acc, k, metric)


# ----------------------------------------- b. every L2-table and encoder width
@METRICS
@pytest.mark.parametrize("dsub", [1, 2, 3, 5, 6, 7, 12, 16, 20, 256])
def test_every_table_and_encoder_width(dsub, metric):
    """k_l2_table<2 | 12 | 16 | 0> and the encoder's tree<> with a 4-wide remainder and a masked
    tail; 5 and 17 queries: either side of the 16-query tiles, and a ragged group of them."""
    M, nb, k = 8, 300, 10
    ix, cb, xq, codes = encoded(M * dsub, M, metric, 200 + dsub, nb, 17)
    acc = ref_sums(ref_tables(xq, cb, metric), codes)
    for nq in (5, 17):
        D, I = ix.search(xq[:nq], k)
        check(D, I, acc[:nq], k, metric)


# ------------------------------------------------------ c. every table blocking
@METRICS
@pytest.mark.parametrize("M", [32, 48, 64, 80, 112, 128])
def test_every_table_blocking(M, metric):
    """nblk = M / 16 = 2, 3, 4, 5, 7, 8 table blocks, the partial sums kept across them."""
    nb, nq = 2048 + 552, 5
    ix, cb, xq, codes = encoded(2 * M, M, metric, 300 + M, nb, nq)
    acc = ref_sums(ref_tables(xq, cb, metric), codes)
    for k in (10, 100):
        p = plan(M, k, nq, nb)
        assert (p.ranges, p.rows) == (2, 2048)
        D, I = ix.search(xq, k)
        check(D, I, acc, k, metric)


# --------------------------------------------------------- d. k and nb boundaries
@METRICS
@pytest.mark.parametrize("nb", [1024, 1025, 2047, 2048, 2049, 4096])
def test_k_and_nb_boundaries(nb, metric):
    """nb on a pass (1024) or range (2048) boundary and one row to either side of it; k at the
    switches of the top-k's register rows (64 | 65, 256 | 257) and at a full row pair (128 | 129)."""
    d, M, nq = 32, 8, 5
    ix, cb, xq, codes = encoded(d, M, metric, 400, nb, nq)
    acc = ref_sums(ref_tables(xq, cb, metric), codes)
    order = ref_order(acc, 257, metric)
    for k in (64, 65, 128, 129, 256, 257):
        p = plan(M, k, nq, nb)
        assert (p.ranges, p.rows) == ((nb + 2047) // 2048, 2048)
        D, I = ix.search(xq, k)
        check(D, I, acc, k, metric, order)


# --------------------------------------------------------- e. many partial lists
@METRICS
def test_many_partial_lists(metric):
    d, M, nq, nb = 32, 8, 5, 33 * 2048 + 5
    for k, want in ((1, (34, 2048, 136)), (10, (34, 2048, 136)), (64, (34, 2048, 136)), (96, (17, 4096, 68))):
        p = plan(M, k, nq, nb)
        assert (p.ranges, p.rows, p.S) == want
    assert plan(M, 10, nq, nb).S * 10 <= 2048  # the merge stages its input in LDS
    assert plan(M, 64, nq, nb).S * 64 > 2048   # ... and here it reads it from memory
    ix, cb, xq, codes = encoded(d, M, metric, 500, nb, nq)
    acc = ref_sums(ref_tables(xq, cb, metric), codes)
    order = ref_order(acc, 96, metric)
    for k in (1, 10, 64, 96):
        D, I = ix.search(xq, k)
        check(D, I, acc, k, metric, order)


# ------------------------------------------------------------ f. crafted keys
# dsub 1, M 8, the query all ones: under inner product a row's similarity is exactly the
# integer key = 256 * code[0] + code[1] < 65536 in float32.
KS_F = (1, 10, 64, 65, 256, 257, 1024)
NB_F = 3 * 2048 + 777
NQ_F = 4097  # a chunk of 4096 queries: one range, so every workgroup passes over all rows; and one more


def key_codes(keys):
    keys = np.asarray(keys, np.int64)
    assert keys.min() >= 0 and keys.max() < 65536
    codes = np.zeros((len(keys), 8), np.uint8)
    codes[:, 0] = keys >> 8
    codes[:, 1] = keys & 255
    return codes


def key_index_ip(keys):
    cb = np.zeros((8, 256, 1), np.float32)
    cb[0, :, 0] = 256 * np.arange(256)
    cb[1, :, 0] = np.arange(256)
    codes = key_codes(keys)
    ix = make_index(8, 8, IP, cb)
    ix.add_codes(codes)
    xq = np.ones((1, 8), np.float32)
    acc = ref_sums(ref_tables(xq, cb, IP), codes)
    np.testing.assert_array_equal(acc[0], np.asarray(keys, np.float32))
    return ix, xq, acc


def search_same_query(ix, xq, acc, metric, ks=KS_F):
    """NQ_F copies of one query: every one must come back as the reference of that query."""
    nb = acc.shape[1]
    order = ref_order(acc, max(ks), metric)
    xqs = np.repeat(xq, NQ_F, 0)
    for k in ks:
        p = plan(8, k, NQ_F, nb)
        assert (p.chunk, p.ranges) == (4096, 1)
        assert -(-nb // pass_rows(k)) >= 4  # passes of the one range
        D, I = ix.search(xqs, k)
        Dr, Ir = ref_topk(acc, k, metric, order)
        np.testing.assert_array_equal(I, np.broadcast_to(Ir, I.shape))
        np.testing.assert_array_equal(D, np.broadcast_to(Dr, D.shape))
    return I


def test_keys_ascending_every_row_is_admitted():
    keys = 9 * np.arange(NB_F)  # every row beats all earlier rows
    ix, xq, acc = key_index_ip(keys)
    search_same_query(ix, xq, acc, IP)


def test_keys_descending_nothing_is_admitted_after_the_fill():
    keys = 65535 - 9 * np.arange(NB_F)
    ix, xq, acc = key_index_ip(keys)
    search_same_query(ix, xq, acc, IP)


def test_all_keys_equal_come_back_in_label_order():
    """Ties by label across the waves' lists, the passes, the ranges and the merge."""
    ix, xq, acc = key_index_ip(np.full(NB_F, 12345))
    for k in KS_F:  # (the second chunk's one query: a range per tile, or 2 of 2 tiles at k = 1024)
        assert plan(8, k, 1, NB_F).ranges == (2 if k == 1024 else 4)
    I = search_same_query(ix, xq, acc, IP)
    np.testing.assert_array_equal(I, np.broadcast_to(np.arange(KS_F[-1]), I.shape))
    for k in (10, 257):
        D, I = ix.search(xq, k)
        np.testing.assert_array_equal(I[0], np.arange(k))
        assert (D == 12345).all()


def test_l2_sums_descending_every_row_is_admitted():
    """The ascending-key case under L2: the query is 0, |0 - cb[0][j]|^2 = (256 + j)^2 steps by
    more than 513 and |0 - cb[1][j]|^2 ~ 2 j stays below 511, so the sum grows with the key."""
    cb = np.zeros((8, 256, 1), np.float32)
    cb[0, :, 0] = 256 + np.arange(256)
    cb[1, :, 0] = np.sqrt(2 * np.arange(256))
    codes = key_codes(9 * (NB_F - 1 - np.arange(NB_F)))
    ix = make_index(8, 8, L2, cb)
    ix.add_codes(codes)
    xq = np.zeros((1, 8), np.float32)
    acc = ref_sums(ref_tables(xq, cb, L2), codes)
    assert (np.diff(acc[0]) < 0).all()  # every row is nearer than all earlier rows
    search_same_query(ix, xq, acc, L2)


@pytest.mark.parametrize("k,nb", [(256, 24 * 2048), (257, 24 * 2048), (1000, 9 * 2048)])
def test_candidate_queue_at_capacity(k, nb):
    """k > 64 queues admitted rows per (wave, query), 64 + 4 * 64 = 320 slots, and merges full
    batches of 64 after every pass, so up to 63 stay pending.  Per wave: a = ceil(k / 256)
    passes of keys from a band fill the top-k (all admitted: the bound is +inf until k rows
    are in); in pass a exactly 63 of its 256 rows lie above the band and the rest below it
    (63 pending, no merge); in pass a + 1 all 256 rows beat everything so far: slots 0..318,
    and a first merge that moves 255 candidates to the front."""
    M = 8
    p = plan(M, k, 1, nb)
    a = -(-k // 256)
    npass = p.rows // pass_rows(k)
    assert pass_rows(k) == 1024 and npass >= a + 2 and nb == p.ranges * p.rows  # every range is full
    assert a * 256 >= k > (a - 1) * 256

    # row = r0 + pass * 1024 + i * 256 + tid, wave = tid >> 6
    row = np.arange(nb)
    in_range = row % p.rows
    ps = in_range // 1024
    tid = in_range % 256
    slot = (in_range % 1024) // 256 * 64 + (tid & 63)  # 0..255 within (range, pass, wave)
    group = row // p.rows * 4 + (tid >> 6)             # (range, wave)
    ngroups = p.ranges * 4
    rng = np.random.default_rng(600 + k)
    mix = rng.integers(0, 10000, nb)
    rank = rng.permuted(np.tile(np.arange(256), (ngroups, 1)), axis=1)
    above = (ps == a) & (rank[group, slot] < 63)
    keys = mix.copy()                       # below the band: [0, 10000)
    keys[ps < a] += 20000                   # the band: [20000, 30000)
    keys[above] += 40000                    # above the band
    keys[ps == a + 1] += 50000              # above everything before

    def per_group(mask):
        return np.bincount(group[mask], minlength=ngroups)

    band = (keys >= 20000) & (keys < 30000)
    assert (per_group((ps < a) & band) == a * 256).all() and not band[ps >= a].any()
    assert (per_group((ps == a) & (keys >= 30000)) == 63).all()
    assert (per_group((ps == a) & (keys < 20000)) == 256 - 63).all()
    best_before = np.full(ngroups, -1)
    np.maximum.at(best_before, group[ps <= a], keys[ps <= a])
    nxt = ps == a + 1
    assert (per_group(nxt) == 256).all() and (keys[nxt] > best_before[group[nxt]]).all()
    assert 63 + 256 - 1 == 318 < 64 + 4 * 64

    ix, xq, acc = key_index_ip(keys)
    D, I = ix.search(xq, k)
    check(D, I, acc, k, IP)


# ----------------------------------------------------- g. mixed-sign accuracy
@METRICS
@pytest.mark.parametrize("d,M", [(32, 8), (768, 96)], ids=["d32_m8", "d768_m96"])
def test_mixed_sign_accuracy(d, M, metric):
    """Against the same sums in float64 (from the float32 inputs), where terms cancel and no
    fixed relative tolerance holds.  With u = 2^-24 and A the float64 sum of the absolute values
    of the d terms of a (query, row) pair (products for inner product, squared differences for
    L2): a term carries at most 3 roundings (the subtraction, counted twice by the square, and
    the product; one for an inner-product term), relative error <= 3 u; the d terms are then
    added in dsub - 1 additions per table entry and M per row (0 + t[0] + ...), and any order
    of n additions has forward error <= n u * sum |terms| to first order.  Hence
        |D - D64| <= (dsub + M + 3) * u * A."""
    nb, nq, k = 3001, 5, 10
    dsub = d // M
    ix, cb, xq, codes = encoded(d, M, metric, 700 + M, nb, nq)
    acc = ref_sums(ref_tables(xq, cb, metric), codes)
    D, I = ix.search(xq, k)
    check(D, I, acc, k, metric)
    want = np.take_along_axis(sums64(xq, cb, codes, metric), I, 1)
    bound = (dsub + M + 3) * 2.0 ** -24 * np.take_along_axis(sums64(xq, cb, codes, metric, absolute=True), I, 1)
    err = np.abs(D.astype(np.float64) - want)
    print(f"max |D - D64| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
