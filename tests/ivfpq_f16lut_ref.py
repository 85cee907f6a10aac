"""IVF-PQ search with float16 lookup tables, restated in numpy:

    key = dis0 + sum over m ascending of float32(h16(L[m][code_m]))

L[m][j] = T1[l][m][j] + (-2) T3[q][m][j] for L2 (one rounding, equal to the kernel's fma), -T3[q][m][j] for
inner product; h16 clips to +-65504 in fp32 and rounds once to IEEE half, nearest even; every add is fp32;
ranking is by (key, label).  T1 / T3, the probes and dis0 are the oracle's."""
import numpy as np

from oracle import oracle as O


def entries(lut, half=True):
    """h16 of fp32 LUT entries, back in fp32 (half=False: the fp32 entries as they are)."""
    return np.clip(lut, -65504, 65504).astype(np.float16).astype(np.float32) if half else lut


def search(xq, k, centroids, codebook, list_codes, list_ids, nprobe, ip=False, half=True, stats=None):
    """(D, I) [nq][k] in the library's conventions: L2 distances ascending, padded (FLT_MAX, -1); inner
    products descending, padded (-FLT_MAX, -1).  stats (a dict): 'saturated' counts the clipped entries."""
    xq = np.ascontiguousarray(xq, np.float32)
    T3 = O.ip_table(xq, codebook)
    T1 = None if ip else O.precompute_T1(centroids, codebook)
    dis0, probes = O.coarse_search(xq, centroids, nprobe, metric=O.METRIC_INNER_PRODUCT if ip else O.METRIC_L2)
    fmax = np.finfo(np.float32).max
    D = np.full((len(xq), k), -fmax if ip else fmax, np.float32)
    I = np.full((len(xq), k), -1, np.int64)
    rows = np.arange(codebook.shape[0])
    for q in range(len(xq)):
        keys, labels = [], []
        for p, l in enumerate(probes[q]):
            lut = -T3[q] if ip else np.float32(T1[l] + np.float32(-2) * T3[q])
            if stats is not None:
                stats["saturated"] = stats.get("saturated", 0) + int((np.abs(lut) > 65504).sum())
            lut = entries(lut, half)
            d0 = np.float32(-O.tree(xq[q], centroids[l], 0)) if ip else dis0[q, p]
            acc = np.full(len(list_ids[l]), d0, np.float32)
            for m in rows:  # sequential fp32 adds in m order
                acc = acc + lut[m, list_codes[l][:, m]]
            keys.append(acc)
            labels.append(list_ids[l])
        keys, labels = np.concatenate(keys), np.concatenate(labels)
        order = np.lexsort((labels, keys))[:k]
        D[q, :len(order)] = -keys[order] if ip else keys[order]
        I[q, :len(order)] = labels[order]
    return D, I
