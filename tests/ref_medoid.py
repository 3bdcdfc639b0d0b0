"""Numpy checker of the median descriptor (plba_desc_medoid, plslam_desc_medoid_cpu): for a list of n
descriptors the symmetric Hamming table, the k-th smallest value of every row with
k = min(int(1 + 0.5 (n - 1)), n - 1), and the first row whose value is strictly below 99999 and every
earlier row's. An empty list gives -1. Written from the definition (a sort of every row), independent
of the library's counting."""
import numpy as np

_POP = np.array([bin(v).count("1") for v in range(256)], np.int64)
START = 99999


def table(desc):
    d = np.asarray(desc, np.uint8)
    return _POP[d[:, None, :] ^ d[None, :, :]].sum(axis=2)


def row_values(desc):
    """The k-th smallest entry of each row of the table."""
    n = len(desc)
    k = min(int(1 + 0.5 * (n - 1)), n - 1)
    return np.sort(table(desc), axis=1)[:, k]


def medoid(desc):
    n = len(desc)
    if n == 0:
        return -1
    best, best_i = START, 0
    for i, v in enumerate(row_values(desc)):
        if int(v) < best:
            best, best_i = int(v), i
    return best_i


def medoids(list_ptr, desc, desc_bytes):
    d = np.asarray(desc, np.uint8).reshape(-1, desc_bytes)
    return np.array([medoid(d[a:b]) for a, b in zip(list_ptr[:-1], list_ptr[1:])], np.int32)
