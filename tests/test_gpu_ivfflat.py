"""IndexIVFFlat on the GPU against Faiss's IndexIVFFlat::search restated in numpy on the
oracle (tests/ivfflat_ref.py): labels and distances must be identical to it, and on the
random-data cases within 1e-4 relative of the same sums in float64.  The float64 check
needs sums without cancellation: for L2 every term is a square; for inner product the data
are non-negative.  Each of the eight accumulators adds d / 8 such terms, so the fp32 sum is
within (d / 8 + 4) * 2^-24 relative of the exact one: 1.6e-5 at d = 2048, inside 1e-4.

Quantizers are installed with ``set_trained`` from seeded data, except in the training
test.  A list longer than RANGE_ROWS (``kIvfFlatRangeRows`` in csrc/ivf_flat.h, checked
in tests/test_ivfflat_cpu.py) is scanned as several row ranges; each (probe, range) gives
four sorted partial lists (one per wave), and the final merge runs in rounds of at most
16 lists and 2048 entries per query: k = 1024 merges two lists per round, so nlist =
nprobe = 64 reaches eight rounds.
"""
import functools

import numpy as np
import pytest

import faiss_amd as faiss
import ivfflat_ref as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-4
IP, L2 = faiss.METRIC_INNER_PRODUCT, faiss.METRIC_L2
METRICS = [pytest.param(IP, id="ip"), pytest.param(L2, id="l2")]
G = R.RANGE_ROWS


def data(seed, n, d, metric):
    """Seeded vectors: uniform [0, 1) for inner product (non-negative), normal for L2."""
    rng = np.random.default_rng(seed)
    return (rng.random((n, d)) if metric == IP else rng.standard_normal((n, d))).astype(np.float32)


def build(xb, cent, metric, ids=None):
    ix = faiss.IndexIVFFlat(None, xb.shape[1], len(cent), metric)
    ix.set_trained(cent)
    if ids is None:
        ix.add(xb)
    else:
        ix.add_with_ids(xb, ids)
    return ix


def check(got, want, ref=None, xq=None):
    D, I = got
    Dr, Ir = want
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)
    if ref is not None:  # against the float64 sums, where a result exists
        d64 = ref.dist64(xq)
        pos = {int(v): i for i, v in enumerate(ref.ids)}
        for q in range(len(I)):
            ok = I[q] >= 0
            want64 = d64[q, [pos[int(v)] for v in I[q][ok]]]
            np.testing.assert_allclose(D[q][ok], want64, rtol=RTOL, atol=0)


# ------------------------------------------------------------------ base sweep
@functools.lru_cache(maxsize=None)
def base(metric):
    d, nlist, nb, nq = 32, 16, 5000, 37
    xb = data(1, nb, d, metric)
    cent = data(2, nlist, d, metric)
    xq = data(3, nq, d, metric)
    ids = np.random.default_rng(4).permutation(nb).astype(np.int64)  # position order != label order across lists
    return build(xb, cent, metric, ids), R.Ref(xb, cent, metric, ids), xq


@pytest.mark.parametrize("k", [1, 10, 64, 65, 100, 1024])
@pytest.mark.parametrize("nprobe", [1, 4, 16])
@pytest.mark.parametrize("metric", METRICS)
def test_base_sweep(metric, nprobe, k):
    ix, ref, xq = base(metric)
    ix.nprobe = nprobe
    want = ref.search(xq, k, nprobe=nprobe)
    if nprobe == 1 and k == 1024:
        assert (want[1] == -1).any()  # fewer candidates than k: padded
    check(ix.search(xq, k), want, ref, xq)


# ------------------------------------------------- every phase of the reduction
@pytest.mark.parametrize("d,nb,nlist", [(4, 1500, 8), (12, 1500, 8), (200, 1500, 8), (2048, 300, 4)],
                         ids=["d4-remainder", "d12-8+4", "d200-chunks", "d2048"])
@pytest.mark.parametrize("metric", METRICS)
def test_reduction_phases(metric, d, nb, nlist):
    xb, cent, xq = data(11, nb, d, metric), data(12, nlist, d, metric), data(13, 9, d, metric)
    ix, ref = build(xb, cent, metric), R.Ref(xb, cent, metric)
    ix.nprobe = 3
    for k in (10, 100):
        check(ix.search(xq, k), ref.search(xq, k, nprobe=3), ref, xq)


# ------------------------------------------------------------------ exact ties
@pytest.mark.parametrize("metric", METRICS)
def test_exact_ties_are_ordered_by_label(metric):
    rng = np.random.default_rng(21)
    nb, nlist, nq = 4000, 8, 9
    xb = rng.integers(0, 4, (nb, 8)).astype(np.float32)
    xq = rng.integers(0, 4, (nq, 8)).astype(np.float32)
    cent = rng.integers(0, 4, (nlist, 8)).astype(np.float32) + np.float32(0.25) * np.arange(nlist, dtype=np.float32)[:, None]
    ids = rng.permutation(nb).astype(np.int64)
    ix, ref = build(xb, cent, metric, ids), R.Ref(xb, cent, metric, ids)
    ix.nprobe = 8
    want = ref.search(xq, 100, nprobe=8)
    assert max(len(np.unique(row)) for row in want[0]) < 60  # nearly every rank is decided by label
    check(ix.search(xq, 100), want)


# ------------------------------------------------------------------ long lists
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("metric", METRICS)
def test_ivf1_list_of_several_ranges(metric, k):
    ix, ref, xq = ivf1(metric)
    check(ix.search(xq, k), ref.search(xq, k, nprobe=1), ref, xq)


@functools.lru_cache(maxsize=None)
def ivf1(metric):
    d, nb = 16, 3 * G + 5
    xb, xq = data(31, nb, d, metric), data(32, 6, d, metric)
    cent = data(33, 1, d, metric)
    ix = faiss.index_factory(d, "IVF1,Flat", metric)
    ix.set_trained(cent)
    ix.add(xb)
    assert ix.invlists.list_size(0) == nb
    return ix, R.Ref(xb, cent, metric), xq


@functools.lru_cache(maxsize=None)
def two_lists(metric):
    d, n0 = 16, 2 * G + 777
    xb = data(34, n0 + 3, d, metric)
    cent = np.zeros((2, d), np.float32)
    cent[0, 0] = cent[1, 1] = 50.0
    xb[:n0, 0] += 50.0  # next to the first centroid under either metric
    xb[n0:, 1] += 50.0  # three vectors next to the second
    ix, ref = build(xb, cent, metric), R.Ref(xb, cent, metric)
    assert list(np.bincount(ref.list_of, minlength=2)) == [n0, 3]
    xq = data(35, 7, d, metric)
    xq[:5, 0] += 50.0
    xq[5:, 1] += 50.0
    return ix, ref, xq


@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("metric", METRICS)
def test_long_list_beside_a_short_one(metric, k):
    ix, ref, xq = two_lists(metric)
    ix.nprobe = 2
    check(ix.search(xq, k), ref.search(xq, k, nprobe=2), ref, xq)
    ix.nprobe = 1
    check(ix.search(xq, k), ref.search(xq, k, nprobe=1), ref, xq)


# ---------------------------------------------------------- many partial lists
@pytest.mark.parametrize("metric", METRICS)
def test_many_partial_lists_merge_in_rounds(metric):
    d, nlist, nb = 16, 64, 6000
    xb, cent, xq = data(41, nb, d, metric), data(42, nlist, d, metric), data(43, 5, d, metric)
    ids = np.random.default_rng(44).permutation(nb).astype(np.int64)
    ix, ref = build(xb, cent, metric, ids), R.Ref(xb, cent, metric, ids)
    ix.nprobe = 64
    check(ix.search(xq, 1024), ref.search(xq, 1024, nprobe=64), ref, xq)


# ----------------------------------------------------------------------- edges
@pytest.mark.parametrize("metric", METRICS)
def test_empty_index(metric):
    ix = faiss.IndexIVFFlat(None, 8, 4, metric)
    ix.set_trained(data(51, 4, 8, metric))
    assert ix.ntotal == 0
    D, I = ix.search(data(52, 3, 8, metric), 5)
    assert (I == -1).all() and (D == (-R.FMAX if metric == IP else R.FMAX)).all()


@pytest.mark.parametrize("metric", METRICS)
def test_empty_probed_list_clamped_nprobe_and_one_query(metric):
    d, nlist = 8, 5
    xb, cent = data(53, 700, d, metric), data(54, nlist, d, metric)
    cent[3] = -40.0  # no vector is assigned here (L2: far away; IP: the smallest similarity)
    ix, ref = build(xb, cent, metric), R.Ref(xb, cent, metric)
    assert ix.invlists.list_size(3) == 0 and (ref.list_of != 3).all()
    xq = data(55, 4, d, metric)
    ix.nprobe = nlist
    want = ref.search(xq, 10, nprobe=nlist)
    check(ix.search(xq, 10), want, ref, xq)
    ix.nprobe = 50  # > nlist: clamped
    check(ix.search(xq, 10), want)
    check(ix.search(xq[:1], 10), (want[0][:1], want[1][:1]))


@pytest.mark.parametrize("metric", METRICS)
def test_search_preassigned(metric):
    ix, ref, xq = base(metric)
    ix.nprobe = 4
    Iq = R.probes(xq, ref.cent, 4, metric).copy()
    Iq[0, 2] = -1
    Iq[1] = -1            # nothing to scan
    Iq[2, 3] = Iq[2, 0]   # a repeated list is scanned once
    Iq[3, :] = Iq[3, 0]
    want = ref.search(xq, 20, Iq=Iq)
    assert (want[1][1] == -1).all()
    got = ix.search_preassigned(xq, 20, Iq)
    check(got, want, ref, xq)
    Dq = np.random.default_rng(56).standard_normal(Iq.shape).astype(np.float32)
    check(ix.search_preassigned(xq, 20, Iq, Dq), want)  # Dq is ignored
    D = np.empty((len(xq), 20), np.float32)
    I = np.empty((len(xq), 20), np.int64)
    assert ix.search_preassigned(len(xq), faiss.swig_ptr(xq), 20, faiss.swig_ptr(Iq), faiss.swig_ptr(Dq),
                                 faiss.swig_ptr(D), faiss.swig_ptr(I), False) is None
    check((D, I), want)
    check(faiss.ivf_tools.search_preassigned(ix, xq, 20, Iq), want)
    with pytest.raises(RuntimeError, match="nprobe"):
        ix.search_preassigned(xq, 20, Iq[:, :3])


# ------------------------------------------------------------------------ adds
@pytest.mark.parametrize("metric", METRICS)
def test_adds_build_the_same_label_sorted_lists(metric):
    import torch

    d, nlist, nb = 32, 16, 5000
    xb, cent = data(1, nb, d, metric), data(2, nlist, d, metric)
    ref = R.Ref(xb, cent, metric)
    one = build(xb, cent, metric)  # one add: ids 0 .. nb - 1
    assert one.ntotal == nb and one.code_size == 4 * d and one.invlists.code_size == 4 * d
    parts = faiss.IndexIVFFlat(None, d, nlist, metric)
    parts.set_trained(cent)
    perm = np.random.default_rng(61).permutation(nb)
    for sl in np.array_split(perm, 5):
        parts.add_with_ids(xb[sl], sl.astype(np.int64))
    dev = faiss.IndexIVFFlat(None, d, nlist, metric)
    dev.set_trained(cent)
    tx = torch.from_numpy(xb).cuda()
    dev.add_device(tx[:2000])
    dev.add_device(tx[2000:], torch.arange(2000, nb, dtype=torch.int64, device="cuda"))
    want = ref.lists()
    sizes = np.array([len(i) for i, _ in want])
    for ix in (one, parts, dev):
        assert ix.ntotal == nb
        np.testing.assert_array_equal(ix.invlists.list_sizes(), sizes)
        for l in range(nlist):
            ids = ix.invlists.get_ids(l)
            assert (np.diff(ids) > 0).all()
            np.testing.assert_array_equal(ids, want[l][0])
            codes = ix.invlists.get_codes(l)
            assert codes.dtype == np.uint8 and codes.tobytes() == want[l][1].tobytes()
        assert ix.invlists.imbalance_factor() == pytest.approx(nlist * (sizes.astype(float) ** 2).sum() / nb ** 2)
    # sequential ids continue after an add
    one.add(xb[:3])
    assert one.ntotal == nb + 3
    assert sorted(np.concatenate([one.invlists.get_ids(l) for l in range(nlist)]))[-3:] == [nb, nb + 1, nb + 2]
    # reset drops the vectors and keeps the centroids
    one.reset()
    assert one.ntotal == 0 and one.is_trained
    np.testing.assert_array_equal(one.centroids(), cent)
    assert (one.search(xb[:2], 3)[1] == -1).all()
    one.add(xb[:100])
    assert one.ntotal == 100 and one.invlists.list_sizes().sum() == 100
    np.testing.assert_array_equal(np.sort(np.concatenate([one.invlists.get_ids(l) for l in range(nlist)])),
                                  np.arange(100))


def test_add_device_with_ids_past_the_pending_threshold():
    """Exercises the add that merges its own pending set: one as large as the image and of at
    least 256 MiB (kChunkBytes of csrc/host_common.h); 32768 vectors of d = 2048 are the fewest
    that reach it.  Device vectors and device labels; a later small add then waits beside the
    image.  The test cannot see when the merge ran (reading the lists merges whatever is
    pending): it checks that the lists are right after this sequence, not that the add merged.
    Rows sit 0.01 around centroids 10 apart, so the expected lists need no reference search."""
    import torch

    d, nlist, nb, extra = 2048, 4, (256 << 20) // (4 * 2048), 10
    cent = np.zeros((nlist, d), np.float32)
    cent[np.arange(nlist), np.arange(nlist)] = 10.0
    g = torch.Generator(device="cuda").manual_seed(5)
    n = nb + extra
    lists = torch.arange(n, device="cuda") % nlist
    tx = torch.from_numpy(cent).cuda()[lists] + 0.01 * torch.randn((n, d), generator=g, device="cuda")
    tid = 3 * torch.arange(n - 1, -1, -1, dtype=torch.int64, device="cuda") + 7  # decreasing: label order != add order
    ix = faiss.IndexIVFFlat(None, d, nlist, L2)
    ix.set_trained(cent)
    ix.add_device(tx[:nb], tid[:nb])
    ix.add_device(tx[nb:], tid[nb:])
    assert ix.ntotal == n
    np.testing.assert_array_equal(ix.invlists.list_sizes(), np.bincount(lists.cpu().numpy(), minlength=nlist))
    for l in range(nlist):
        rows = torch.nonzero(lists == l).flatten().flip(0)  # the list's rows by increasing label
        np.testing.assert_array_equal(ix.invlists.get_ids(l), tid[rows].cpu().numpy())
        if l == 1:
            assert ix.invlists.get_codes(l).tobytes() == tx[rows].cpu().numpy().tobytes()


# -------------------------------------------------------------------- training
@pytest.mark.parametrize("metric", METRICS)
def test_training_is_the_coarse_kmeans_of_ivfpq(metric):
    d, nlist, n, niter, seed = 32, 16, 2000, 4, 99
    x = data(71, n, d, metric)
    ix = faiss.IndexIVFFlat(None, d, nlist, metric)
    assert not ix.is_trained
    ix.niter_coarse, ix.seed = niter, seed
    ix.train(x)
    assert ix.is_trained
    np.testing.assert_array_equal(ix.centroids(), O.kmeans(x, nlist, niter, seed, metric=metric))
    assert ix.quantizer.ntotal == nlist
    np.testing.assert_array_equal(ix.quantizer.xb.reshape(nlist, d), ix.centroids())
    pq = faiss.IndexIVFPQ(None, d, nlist, 8, 8, metric)
    pq.niter_coarse, pq.niter_pq, pq.seed = niter, 1, seed
    pq.train(x)
    np.testing.assert_array_equal(ix.centroids(), pq.centroids())


# ---------------------------------------------------------- device entry points
@pytest.mark.parametrize("metric", METRICS)
def test_device_entry_points_on_a_side_stream(metric):
    import torch

    ix, ref, xq = base(metric)
    ix.nprobe = 4
    want = ix.search(xq, 10)
    check(want, ref.search(xq, 10, nprobe=4))
    Iq = R.probes(xq, ref.cent, 4, metric).copy()
    Iq[0, 1] = -1
    want_pre = ix.search_preassigned(xq, 10, Iq)
    tx, tIq = torch.from_numpy(xq).cuda(), torch.from_numpy(Iq).cuda()
    tDq = torch.zeros(Iq.shape, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        D, I = ix.search_device(tx, 10)
        Dp, Ip = ix.search_preassigned_device(tx, 10, tIq, tDq)
    D2, I2 = ix.search_device(tx, 10)  # torch's current stream: ordered after the side stream's calls
    side.synchronize()
    torch.cuda.synchronize()
    check((D.cpu().numpy(), I.cpu().numpy()), want)
    check((D2.cpu().numpy(), I2.cpu().numpy()), want)
    check((Dp.cpu().numpy(), Ip.cpu().numpy()), want_pre)
    with pytest.raises(RuntimeError):
        ix.search_device(tx.double(), 10)


# ------------------------------------------------- the segmented coarse quantizer
@pytest.mark.parametrize("metric", METRICS)
def test_segmented_coarse_quantizer_is_the_one_of_ivfpq(metric):
    """nlist = 8192: the coarse quantizer takes its large-nlist path (no key matrix), which
    IndexIVFFlat enters without IVF-PQ's planning arguments.  Self-consistency against an
    IndexIVFPQ on the same centroids: the same top-1 assignment of the adds, and the same
    probes in a search (the IVF-PQ coarse call is the one test_gpu_configs.py holds to the oracle)."""
    import torch

    d, nlist, nb, nq, nprobe, k, M = 16, 8192, 20000, 33, 8, 10, 8
    xb, cent, xq = data(81, nb, d, metric), data(82, nlist, d, metric), data(83, nq, d, metric)
    ids = np.random.default_rng(84).permutation(nb).astype(np.int64)
    flat = build(xb, cent, metric, ids)
    pq = faiss.IndexIVFPQ(None, d, nlist, M, 8, metric)
    pq.set_trained(cent, data(85, M * 256, d // M, metric))
    pq.add_with_ids(xb, ids)
    assert flat.ntotal == pq.ntotal == nb
    np.testing.assert_array_equal(flat.invlists.list_sizes(), pq.invlists.list_sizes())
    flat.nprobe = pq.nprobe = nprobe
    _, Iq = pq.coarse_device(torch.from_numpy(xq).cuda())
    torch.cuda.synchronize()
    Iq = Iq.cpu().numpy()
    assert Iq.shape == (nq, nprobe) and (Iq >= 0).all() and (Iq < nlist).all()
    D, I = flat.search(xq, k)
    Dp, Ip = flat.search_preassigned(xq, k, Iq)
    np.testing.assert_array_equal(I, Ip)
    np.testing.assert_array_equal(D, Dp)
    assert (I >= 0).any()  # (the probed lists are not all empty)


# ------------------------------------------------------------- file round trip
@pytest.mark.parametrize("metric", METRICS)
def test_write_read_index_round_trip(metric, tmp_path):
    ix, ref, xq = base(metric)
    ix.nprobe = 4
    path = str(tmp_path / "ivfflat.index")
    faiss.write_index(ix, path)
    with pytest.raises(RuntimeError):
        faiss.write_index(ix, path + ".native", fmt="native")
    back = faiss.read_index(path)
    assert isinstance(back, faiss.IndexIVFFlat)
    assert (back.d, back.nlist, back.nprobe, back.ntotal, back.metric_type) == (ix.d, ix.nlist, 4, ix.ntotal, metric)
    np.testing.assert_array_equal(back.centroids(), ix.centroids())
    for l in range(ix.nlist):
        np.testing.assert_array_equal(back.invlists.get_ids(l), ix.invlists.get_ids(l))
        assert back.invlists.get_codes(l).tobytes() == ix.invlists.get_codes(l).tobytes()
    check(back.search(xq, 10), ix.search(xq, 10))


# --------------------------------------------------------------- caller replay
def test_bench_gpu_1bn_flat_replay():
    """bench_gpu_1bn.py:571-595 with an index key ending in ",Flat": an IndexFlatL2 coarse
    quantizer, IndexIVFFlat(coarse_quantizer, d, ncent, METRIC_L2), train, then the base
    added in slices (:598-658) and the queries searched in blocks (:788-806)."""
    d, ncent, nb, nq, topK = 32, 32, 6000, 50, 10
    xt, xb, xq = data(81, 3000, d, L2), data(82, nb, d, L2), data(83, nq, d, L2)
    coarse_quantizer = faiss.IndexFlatL2(d)
    idx_model = faiss.IndexIVFFlat(coarse_quantizer, d, ncent, faiss.METRIC_L2)
    idx_model.niter_coarse = 3
    idx_model.train(xt)
    assert coarse_quantizer.ntotal == ncent
    for i0 in range(0, nb, 2500):  # add_batch_size slices
        idx_model.add_with_ids(xb[i0:i0 + 2500], np.arange(i0, min(nb, i0 + 2500)))
    assert idx_model.ntotal == nb
    ps = faiss.ParameterSpace()
    ps.initialize(idx_model)
    ref = R.Ref(xb, idx_model.centroids(), L2)
    for nprobe in (1, 8):
        ps.set_index_parameter(idx_model, "nprobe", nprobe)
        D = np.empty((nq, topK), np.float32)
        I = np.empty((nq, topK), np.int64)
        for q0 in range(0, nq, 16):  # query blocks of qbs
            D[q0:q0 + 16], I[q0:q0 + 16] = idx_model.search(xq[q0:q0 + 16], topK)
        check((D, I), ref.search(xq, topK, nprobe=nprobe), ref, xq)
