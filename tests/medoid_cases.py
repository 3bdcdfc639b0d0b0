"""Descriptor lists for the median-descriptor tests: hand-made lists whose answer is written out, and
seeded random ones. A case is (desc_bytes, [list, ...]), every list uint8 [n][desc_bytes]."""
import numpy as np


def _bits(desc_bytes, *positions):
    """A descriptor with the given bits set."""
    d = np.zeros(desc_bytes, np.uint8)
    for p in positions:
        d[p // 8] |= 1 << (p % 8)
    return d


def _rand(seed, n, desc_bytes):
    return np.random.default_rng(seed).integers(0, 256, (n, desc_bytes), dtype=np.uint8)


def _noisy(seed, n, desc_bytes, flips=12):
    """Observations of one feature: a base descriptor with a few bits flipped in each, as a track has them."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, desc_bytes, dtype=np.uint8)
    out = np.repeat(base[None], n, axis=0)
    for i in range(n):
        for p in rng.choice(8 * desc_bytes, size=int(rng.integers(0, min(flips, 8 * desc_bytes) + 1)), replace=False):
            out[i, p // 8] ^= np.uint8(1 << (p % 8))
    return out


def hand(desc_bytes=32):
    """name -> (list, expected medoid)."""
    B = desc_bytes
    e = lambda *p: _bits(B, *p)
    return {
        "empty": (np.zeros((0, B), np.uint8), -1),
        "one": (np.stack([e(1, 2, 3)]), 0),
        # n = 2: k = 1, both rows hold {0, d}: a tie, the first wins
        "two": (np.stack([e(0), e(1, 2)]), 0),
        # n = 3: k = 2, the largest of a row. Rows: {0,1,3} {0,1,2} {0,3,2}: values 3, 2, 3
        "three_middle": (np.stack([e(), e(0), e(0, 1, 2)]), 1),
        # n = 4: k = 2. d(0,1)=1 d(0,2)=2 d(0,3)=3 d(1,2)=1 d(1,3)=2 d(2,3)=1: values 2, 1, 1, 2: tie of 1 and 2
        "four_tie_first_wins": (np.stack([e(), e(0), e(0, 1), e(0, 1, 2)]), 1),
        # n = 5: k = 3. A chain 0..4 of one more bit each: values 3, 2, 2, 2, 3 -> row 1 before rows 2 and 3
        "five_chain": (np.stack([e(), e(0), e(0, 1), e(0, 1, 2), e(0, 1, 2, 3)]), 1),
        # identical descriptors: every value is 0, and only row 0 is strictly below the start value
        "identical": (np.repeat(e(5, 77, 200)[None], 7, axis=0), 0),
        # every pair at the same distance 2 (one own bit each): all values equal, strict < keeps row 0
        "equidistant": (np.stack([e(10 + i) for i in range(6)]), 0),
        # the minimum comes last: a later row replaces an earlier one only when strictly smaller
        "last_is_best": (np.stack([e(0, 1, 2, 3), e(4, 5, 6, 7), e(8, 9), e()]), 3),
        # all ones against all zeros: the largest distance there is, 8 * desc_bytes
        "max_distance": (np.stack([np.zeros(B, np.uint8), np.full(B, 255, np.uint8), np.zeros(B, np.uint8)]), 0),
    }


def small_lists(desc_bytes):
    """n = 0 .. 5 random and noisy lists: the median index for even and odd n."""
    out = []
    for n in range(6):
        out.append(_rand(100 + n, n, desc_bytes))
        out.append(_noisy(200 + n, n, desc_bytes))
    return out


def wave_lists(desc_bytes):
    """n = 63, 64, 65: the last list of one wave and the first of a workgroup."""
    return [_noisy(300 + n, n, desc_bytes, flips=40) for n in (63, 64, 65)] + [_rand(310 + n, n, desc_bytes) for n in (63, 64, 65)]


def mixed_batch(desc_bytes, n_lists=300, seed=7):
    """Track lengths 0 .. 130 with empty lists among them, short and long lists interleaved."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_lists):
        r = rng.random()
        n = 0 if r < 0.1 else int(rng.integers(1, 12)) if r < 0.6 else int(rng.integers(12, 65)) if r < 0.9 else int(rng.integers(65, 131))
        out.append(_noisy(1000 + i, n, desc_bytes, flips=30) if i % 2 else _rand(1000 + i, n, desc_bytes))
    return out


def pack(lists, desc_bytes):
    """(list_ptr int32 [B+1], desc uint8 [total][desc_bytes])."""
    ptr = np.zeros(len(lists) + 1, np.int32)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    desc = np.concatenate([np.asarray(x, np.uint8).reshape(-1, desc_bytes) for x in lists] + [np.zeros((0, desc_bytes), np.uint8)])
    return ptr, np.ascontiguousarray(desc)
