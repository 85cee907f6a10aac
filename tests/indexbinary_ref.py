"""IndexBinaryFlat restated in numpy, shared by tests/test_indexbinary_cpu.py and
tests/test_gpu_indexbinary.py: Hamming distances from a 256-entry popcount table in blocks,
the top-k from np.lexsort((label, dist)), padding (2147483647, -1)."""
import numpy as np

PAD_DIST = 2147483647  # Faiss's CMax<int32_t> neutral
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def hamming(xq, xb):
    """int32 [nq][nb] distances between uint8 [nq][cs] and uint8 [nb][cs], in blocks of rows."""
    xq, xb = np.asarray(xq, np.uint8), np.asarray(xb, np.uint8)
    out = np.empty((xq.shape[0], xb.shape[0]), np.int32)
    block = max(1, (1 << 24) // max(1, xq.size))
    for b0 in range(0, xb.shape[0], block):
        blk = xb[b0:b0 + block]
        out[:, b0:b0 + block] = POPCOUNT[xq[:, None, :] ^ blk[None, :, :]].sum(-1, dtype=np.int32)
    return out


def topk(dist, k):
    """Per row of dist the k smallest (dist, label) pairs ascending, ties by label; padded."""
    nq, nb = dist.shape
    D = np.full((nq, k), PAD_DIST, np.int32)
    I = np.full((nq, k), -1, np.int64)
    labels = np.arange(nb)
    for q in range(nq):
        order = np.lexsort((labels, dist[q]))[:k]
        D[q, :len(order)] = dist[q, order]
        I[q, :len(order)] = order
    return D, I


class Ref:
    """The codes of an IndexBinaryFlat and its search."""

    def __init__(self, xb):
        self.xb = np.ascontiguousarray(xb, np.uint8)

    def search(self, xq, k):
        if self.xb.shape[0] == 0:
            n = np.asarray(xq).shape[0]
            return np.full((n, k), PAD_DIST, np.int32), np.full((n, k), -1, np.int64)
        return topk(hamming(xq, self.xb), k)
