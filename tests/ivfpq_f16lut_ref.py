"""IVF-PQ search with float16 lookup tables, restated in numpy:

    key = dis0 + sum over m ascending of float32(h16(L[m][code_m]))

L[m][j] = T1[l][m][j] + (-2) T3[q][m][j] for L2 (one rounding, equal to the kernel's fma), -T3[q][m][j] for
inner product; h16 clips to +-65504 in fp32 and rounds once to IEEE half, nearest even; every add is fp32;
ranking is by (key, label).  T1 / T3, the probes and dis0 are the oracle's.  `search` runs the oracle's coarse
step; `search_preassigned` takes the probes (and, for L2, dis0) as given; `pair_keys` is the key of every row
of one list for one query, which the builders of tests/scan_order.py order their rows by."""
import numpy as np

from oracle import oracle as O


def entries(lut, half=True):
    """h16 of fp32 LUT entries, back in fp32 (half=False: the fp32 entries as they are)."""
    return np.clip(lut, -65504, 65504).astype(np.float16).astype(np.float32) if half else lut


def lut32(T3q, T1l, ip=False):
    """The fp32 entries [M][256] of one (query, list) pair: T3q = T3[q], T1l = T1[l] (unused for ip)."""
    return -T3q if ip else np.float32(T1l + np.float32(-2) * T3q)


def sum_keys(lut, d0, codes):
    """d0 + the entries lut[m][codes[:, m]], m ascending, every add in fp32."""
    acc = np.full(len(codes), d0, np.float32)
    for m in range(lut.shape[0]):  # sequential fp32 adds in m order
        acc = acc + lut[m, codes[:, m]]
    return acc


def pair_keys(q, cent_l, codebook, codes, d0=None, ip=False, half=True):
    """fp32 keys (ascending = better, so the negated similarity for ip) of the rows `codes` of a list with
    centroid cent_l for the query q.  d0: the pair's dis0 for L2 (default: the oracle's |q - cent_l|^2); for
    the inner product it is formed here, as the scan forms it."""
    q = np.ascontiguousarray(q, np.float32)
    T3q = O.ip_table(q[None], codebook)[0]
    T1l = None if ip else O.precompute_T1(np.ascontiguousarray(cent_l, np.float32)[None], codebook)[0]
    if ip:
        d0 = np.float32(-O.tree(q, cent_l, 0))
    elif d0 is None:
        d0 = np.float32(O.tree(q, cent_l, 1))
    return sum_keys(entries(lut32(T3q, T1l, ip), half), d0, codes)


def search_preassigned(xq, k, probes, dis0, centroids, codebook, list_codes, list_ids, ip=False, half=True,
                       stats=None, flush=False):
    """(D, I) [nq][k] in the library's conventions: L2 distances ascending, padded (FLT_MAX, -1); inner
    products descending, padded (-FLT_MAX, -1).  probes [nq][nprobe]: list numbers, -1 and empty lists
    contribute nothing; dis0 [nq][nprobe] is taken as given for L2 and ignored (None) for the inner product.
    stats (a dict): 'saturated' counts the clipped entries.  flush=True is *not* the library's rule: half
    entries below 2^-14 in magnitude become 0, what hardware that flushes half denormals would compute."""
    xq = np.ascontiguousarray(xq, np.float32)
    probes = np.asarray(probes, np.int64)
    T3 = O.ip_table(xq, codebook)
    used = np.unique(probes[probes >= 0])
    T1 = {} if ip else dict(zip(used.tolist(), O.precompute_T1(np.ascontiguousarray(centroids[used]), codebook)))
    fmax = np.finfo(np.float32).max
    D = np.full((len(xq), k), -fmax if ip else fmax, np.float32)
    I = np.full((len(xq), k), -1, np.int64)
    for q in range(len(xq)):
        keys, labels = [np.zeros(0, np.float32)], [np.zeros(0, np.int64)]
        for p, l in enumerate(probes[q]):
            if l < 0 or len(list_ids[l]) == 0:
                continue
            lut = lut32(T3[q], T1.get(int(l)), ip)
            if stats is not None:
                stats["saturated"] = stats.get("saturated", 0) + int((np.abs(lut) > 65504).sum())
            lut = entries(lut, half)
            if flush:
                lut = np.where(np.abs(lut) < np.float32(2.0 ** -14), np.float32(0), lut)
            d0 = np.float32(-O.tree(xq[q], centroids[l], 0)) if ip else dis0[q, p]
            keys.append(sum_keys(lut, d0, list_codes[l]))
            labels.append(list_ids[l])
        keys, labels = np.concatenate(keys), np.concatenate(labels)
        order = np.lexsort((labels, keys))[:k]
        D[q, :len(order)] = -keys[order] if ip else keys[order]
        I[q, :len(order)] = labels[order]
    return D, I


def search(xq, k, centroids, codebook, list_codes, list_ids, nprobe, ip=False, half=True, stats=None):
    """search_preassigned on the probes (and dis0) of the oracle's coarse step."""
    xq = np.ascontiguousarray(xq, np.float32)
    dis0, probes = O.coarse_search(xq, centroids, nprobe, metric=O.METRIC_INNER_PRODUCT if ip else O.METRIC_L2)
    return search_preassigned(xq, k, probes, dis0, centroids, codebook, list_codes, list_ids, ip, half, stats)


def prefix(DI, k):
    """The answer for k of a result (D, I) for a larger k: its first k columns."""
    return DI[0][:, :k], DI[1][:, :k]
