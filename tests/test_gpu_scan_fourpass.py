"""The split list scan at M = 16 against the CPU oracle, bit for bit, on the cases
that the four-pass form of k_scan_lean can get wrong.

Built with -DSCAN_LEAN_PASSES=4, k_scan_lean builds and gathers its LUT in four
passes of four sub-quantizers through quarter-size LDS buffers, and pass p
gathers with word p of each 16-byte code, loaded for that pass alone (DESIGN.md
section 4).  The default build is the two-pass form, a loop over the same passes
code.  In either a key is still dis0 + L[0] + ... + L[15] in that order, so D and
I must equal the oracle's exactly; this file passes on both builds.

JB = 6 is the shipped SCAN_LEAN_SPLIT_JB: a super-batch is 256 * JB = 1536 codes,
and a list longer than that rebuilds pass 0 for every further super-batch.  The
list sizes sit on every boundary of that loop: an empty list, one code, a wave
(64), a chunk (256), a super-batch and two of them, each +- 1, three super-batches
and 4700.  In both size sets the last list ends in a partly filled chunk and is
the last of the code buffer, so the lanes past its end are the ones whose clamped
index keeps a per-pass word load inside the buffer.  37 queries probing all 8
lists give every list nine items of four pairs and a tail of one.  Random uint8
codes differ in all four words of every code, so a pass that gathers with the
wrong word changes keys; integer-valued tables make many keys tie exactly, so a
changed order of additions or a lost position tie-break shows.  d = 128 is the
benchmark's sub-vector width of 8.
"""
import numpy as np
import pytest

import faiss_amd as faiss
from oracle import oracle as O

pytestmark = pytest.mark.gpu

JB = 6  # SCAN_LEAN_SPLIT_JB of csrc/ivfpq_kernels.hip
SB = 256 * JB
NLIST = 8
SIZES = {
    "short": [0, 1, 63, 64, 65, 255, 256, 257],
    "long": [SB - 1, SB, SB + 1, 2 * SB + 1, 1023, 3 * SB, 2 * SB - 1, 4700],
}
SHAPES = {"d128_m16": (128, 16), "d64_m16": (64, 16)}
NQ = 37
KS = (1, 10, 16)


def make_data(d, M, sizes, integer, seed):
    rng = np.random.default_rng(seed)
    n = int(np.sum(sizes))
    if integer:
        cent = rng.integers(-3, 4, size=(NLIST, d)).astype(np.float32)
        cb = rng.integers(-2, 3, size=(M, 256, d // M)).astype(np.float32)
        xq = rng.integers(-3, 4, size=(NQ, d)).astype(np.float32)
    else:
        cent = rng.normal(size=(NLIST, d)).astype(np.float32)
        cb = (rng.normal(size=(M, 256, d // M)) * 0.5).astype(np.float32)
        xq = rng.normal(size=(NQ, d)).astype(np.float32)
    codes = rng.integers(0, 256, size=(n, M), dtype=np.uint8)
    list_no = np.repeat(np.arange(NLIST, dtype=np.int64), sizes)
    ids = np.arange(n, dtype=np.int64) * 3 + 1
    return cent, cb, xq, codes, list_no, ids


def make_pair(shape, sizes, metric, integer):
    d, M = SHAPES[shape]
    seed = 5000 + 100 * list(SHAPES).index(shape) + 10 * list(SIZES).index(sizes) + 2 * integer + (metric == "ip")
    cent, cb, xq, codes, list_no, ids = make_data(d, M, SIZES[sizes], integer, seed)
    ip = metric == "ip"
    ix = faiss.IndexIVFPQ(None, d, NLIST, M, 8, faiss.METRIC_INNER_PRODUCT if ip else faiss.METRIC_L2, device=0)
    ix.set_trained(cent, cb)
    ix.add_preencoded(list_no, codes, ids)
    ox = O.OracleIVFPQ(d, NLIST, M, metric=O.METRIC_INNER_PRODUCT if ip else O.METRIC_L2)
    ox.set_trained(cent, cb)
    ox.add_preencoded(list_no, codes, ids)
    return ix, ox, xq


def test_sizes_cover_the_loop_boundaries():
    want = {0, 1, 63, 64, 65, 255, 256, 257, SB - 1, SB, SB + 1, 2 * SB + 1, 4700}
    have = set(SIZES["short"]) | set(SIZES["long"])
    assert want <= have
    for s in SIZES.values():
        assert len(s) == NLIST and s[-1] % 256 != 0  # the buffer ends inside a chunk


@pytest.mark.parametrize("integer", [False, True], ids=["gauss", "integer"])
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("sizes", list(SIZES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_four_pass_scan_matches_oracle(shape, sizes, metric, integer):
    ix, ox, xq = make_pair(shape, sizes, metric, integer)
    for nprobe in (8, 3):
        ix.nprobe = ox.nprobe = nprobe
        for k in KS:
            D, I = ix.search(xq, k)
            Dr, Ir = ox.search(xq, k)
            np.testing.assert_array_equal(I, Ir, err_msg=f"nprobe={nprobe} k={k}")
            np.testing.assert_array_equal(D, Dr, err_msg=f"nprobe={nprobe} k={k}")
    assert ix.error_count() == 0


@pytest.mark.parametrize("integer", [False, True], ids=["gauss", "integer"])
def test_four_pass_scan_batches_in_flight(integer):
    """Eight batches in flight on two streams, each into its own output buffers,
    equal the one-at-a-time searches (and so the oracle), with no stale read or
    repair.  In flight the scan is launched with its own grid and residency."""
    import torch

    ix, ox, xq = make_pair("d128_m16", "long", "l2", integer)
    ix.nprobe = ox.nprobe = 8
    k, nb = 10, 8
    rng = np.random.default_rng(78)
    batches = [xq[rng.permutation(NQ)] for _ in range(nb)]
    xd = [torch.from_numpy(b).cuda() for b in batches]
    ref = []
    for b in range(nb):
        D, I = ix.search_device(xd[b], k)
        torch.cuda.synchronize()
        ref.append((D.cpu().numpy(), I.cpu().numpy()))
    Dr, Ir = ox.search(batches[0], k)
    np.testing.assert_array_equal(ref[0][1], Ir)
    np.testing.assert_array_equal(ref[0][0], Dr)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [(torch.empty((NQ, k), device="cuda"), torch.empty((NQ, k), dtype=torch.int64, device="cuda"))
            for _ in range(nb)]
    e0, rs0 = ix.error_count(), ix.repair_stats()
    ix.inflight = True
    try:
        torch.cuda.synchronize()
        for b in range(nb):
            ix.search_device(xd[b], k, outs[b][0], outs[b][1], stream=streams[b % 2].cuda_stream)
        torch.cuda.synchronize()
    finally:
        ix.inflight = False
    for b in range(nb):
        np.testing.assert_array_equal(outs[b][1].cpu().numpy(), ref[b][1], err_msg=f"batch {b}")
        np.testing.assert_array_equal(outs[b][0].cpu().numpy(), ref[b][0], err_msg=f"batch {b}")
    rs = ix.repair_stats()
    assert (rs[0] - rs0[0], rs[1] - rs0[1]) == (0, 0)
    assert ix.error_count() == e0
