"""Which k > 64 probe merge took each query of the last search (host arithmetic).

After a search, the workspace still holds what the list scan left for the merges:
per (query, probe, scan wave) a sorted partial list of 16-B records {key bits,
tag, code position lo, hi} (`ivfpq_debug_workspace` what = 0) and its (count, tag)
(what = 1); what = 2 is the mask of the probes the scan covered.  From the counts
and the keys alone, `classify` repeats the decisions of the launch code and of
k_merge_radix / k_merge_big (ivfpq_kernels.hip) and says, per query, which kernel
merged it and which of that kernel's exits it took.  It establishes coverage only:
it knows nothing of labels or of expected results, which are always the oracle's.

`passes` of a radix query names the pass of the MSB-first 8-bit select after which
the kernel left, as the kernel counts them: 1 = after 16 bits (bucket and the keys
below it <= 128, k <= 128), 2 = after 24 bits (<= 512), 4 = all four passes;
0 = no select (C <= k).
"""
import ctypes

import numpy as np

RADIX_CAP = 512      # kRadixCap
RADIX_KEYS = 8192    # kRadixU * 256: every key of a query in one workgroup's registers
BIG_CAP = 2048       # kBigCap
BIG_SAMPLES = 1280   # 64 lanes * SV sample slots
TAG_MULT = 0x9E3779B1
TAG_MASK = 0x0FFFFFFF


def ukeys(keys_f32):
    """Order-preserving unsigned words of float keys (ukey_of: -0 folded into +0)."""
    b = (np.asarray(keys_f32, np.float32) + np.float32(0.0)).view(np.int32).astype(np.int64)
    o = np.where(b >= 0, b, b ^ 0x7FFFFFFF)
    return ((o & 0xFFFFFFFF) ^ 0x80000000).astype(np.uint32)


def kernel_for(nprobe, k):
    assert k > 64
    if nprobe > 64:
        return "full"
    return "radix" if 4 * nprobe * k <= RADIX_KEYS else "big"


def radix_select(u, k):
    """The select of k_merge_radix over the present keys u (uint32): (passes, T, n)."""
    u = np.asarray(u, np.uint32)
    C = u.size
    if C <= k:
        return 0, 0xFFFFFFFE, C
    prefix, r, passes = 0, k, 4
    for p in range(4):
        shift = 24 - 8 * p
        m = u if p == 0 else u[(u >> np.uint32(shift + 8)) == np.uint32(prefix >> (shift + 8))]
        hist = np.bincount(((m >> np.uint32(shift)) & np.uint32(255)).astype(np.int64), minlength=256)
        incl = np.cumsum(hist)
        b = int(np.searchsorted(incl, r))  # first bucket whose inclusive count reaches r
        h = int(hist[b])
        r -= int(incl[b]) - h
        prefix |= b << shift
        nb = (k - r) + h
        if (p == 1 and nb <= 128 and k <= 128) or (p == 2 and nb <= RADIX_CAP):
            prefix |= (1 << shift) - 1
            passes = p
            break
    return passes, prefix, int(np.count_nonzero(u <= np.uint32(prefix)))


def classify_query(u, nprobe, k):
    """Path of one query from its present keys u (uint32, every scanned list's valid prefix)."""
    u = np.asarray(u, np.uint32)
    C = int(u.size)
    out = {"kernel": kernel_for(nprobe, k), "C": C}
    if out["kernel"] == "radix":
        passes, T, n = radix_select(u, k)
        over = n > RADIX_CAP
        out.update(passes=passes, T=T, n=n, overflow=over, regsort=(not over) and n <= 128 and k <= 128)
    elif out["kernel"] == "big":
        n_le = C if C <= k else int(np.count_nonzero(u <= np.sort(u)[k - 1]))
        out.update(rounds_entered=C > max(2 * k, k + 64), r=-(-C // BIG_SAMPLES), n_le_T=n_le,
                   overflow_certain=n_le > BIG_CAP)
    return out


def label(c):
    """Short class name of one query's path (for counting)."""
    if c["kernel"] == "radix":
        if c["overflow"]:
            return "radix overflow"
        return f"radix merged p{c['passes']} {'regsort' if c['regsort'] else 'ldssort'}"
    if c["kernel"] == "big":
        if c["overflow_certain"]:
            return "big overflow"
        return "big merged " + ("no rounds" if not c["rounds_entered"] else "r=1" if c["r"] == 1 else "r>1")
    return "full"


def classify(counts, keys, scanned, nprobe, k):
    """counts [nq][nprobe][4], keys float32 [nq][nprobe][4][k], scanned bool [nq][nprobe]."""
    out = []
    for q in range(counts.shape[0]):
        parts = [keys[q, p, w, :counts[q, p, w]] for p in range(nprobe) if scanned[q, p] for w in range(4)]
        u = ukeys(np.concatenate(parts)) if parts else np.zeros(0, np.uint32)
        out.append(classify_query(u, nprobe, k))
    return out


# ---------------------------------------------------------------- workspace access
def _ws(ix, ws, what, dtype):
    from faiss_amd import _lib

    lib = _lib.load()
    nb = ctypes.c_int64(0)
    _lib.check(lib.ivfpq_debug_workspace(ix._h, ws, what, None, 0, ctypes.byref(nb)))
    a = np.zeros(max(nb.value // np.dtype(dtype).itemsize, 1), dtype)
    _lib.check(lib.ivfpq_debug_workspace(ix._h, ws, what, a.ctypes.data, a.nbytes, ctypes.byref(nb)))
    return a, int(nb.value)


def epochs(ix):
    """The epoch (batches planned so far) of each of the handle's three workspaces."""
    return [int(_ws(ix, ws, 7, np.uint64)[0][0]) for ws in range(3)]


def read(ix, before, nq, nprobe, k, grown=False):
    """Paths of the one batch searched since `before` = epochs(ix).  The record buffer must
    be exactly nq * nprobe * 4 * k records (the batch was one chunk); `grown`: the handle
    ran a larger batch before (buffers only grow), so it may be larger."""
    after = epochs(ix)
    moved = [ws for ws in range(3) if after[ws] != before[ws]]
    assert len(moved) == 1 and after[moved[0]] == before[moved[0]] + 1, (before, after)
    ws, epoch = moved[0], after[moved[0]]
    nslot = nq * nprobe * 4
    part, pbytes = _ws(ix, ws, 0, np.uint32)
    assert pbytes >= nslot * k * 16 if grown else pbytes == nslot * k * 16, (pbytes, nslot * k * 16)
    pn, nbytes = _ws(ix, ws, 1, np.uint32)
    assert nbytes >= nslot * 8
    qmw = (nprobe + 63) // 64
    qm, qbytes = _ws(ix, ws, 2, np.uint64)
    assert qbytes >= nq * qmw * 8
    qm = qm[:nq * qmw].reshape(nq, qmw)
    p = np.arange(nprobe)
    scanned = ((qm[:, p >> 6] >> (p & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
    pn = pn[:nslot * 2].reshape(nq, nprobe, 4, 2)
    expect = ((epoch * TAG_MULT + np.arange(nslot, dtype=np.int64)) & TAG_MASK).reshape(nq, nprobe, 4)
    fresh = (pn[..., 1].astype(np.int64) & TAG_MASK) == expect
    assert fresh[scanned].all(), "a scanned list's count is not this batch's"
    counts = np.where(scanned[:, :, None], pn[..., 0].astype(np.int64), 0)
    assert (counts >= 0).all() and (counts <= k).all()
    rec = part[:nslot * k * 4].reshape(nq, nprobe, 4, k, 4)
    valid = np.arange(k)[None, None, None, :] < counts[..., None]
    assert ((rec[..., 1].astype(np.int64) & TAG_MASK) == expect[..., None])[valid].all(), "a stale record"
    keys = np.ascontiguousarray(rec[..., 0]).view(np.float32)
    return classify(counts, keys, scanned, nprobe, k)
