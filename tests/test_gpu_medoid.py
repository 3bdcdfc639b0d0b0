"""The median descriptor on the GPU (plba_desc_medoid, Solver.desc_medoid) against the checker
tests/ref_medoid.py: the CPU cases, the wave boundary, the largest list and one above it, a batch of one
and a mixed batch of 300 lists. Integers: equality."""
import numpy as np
import pytest

import medoid_cases as MC
import ref_medoid as RM
from plba import capi
from plba.lib import PlbaError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from plba.lib import Solver
    s = Solver()
    yield s
    s.close()


@pytest.mark.parametrize("desc_bytes", [32, 64])
def test_hand_cases(solver, desc_bytes):
    hand = MC.hand(desc_bytes)
    names = sorted(hand)
    ptr, desc = MC.pack([hand[k][0] for k in names], desc_bytes)
    got = solver.desc_medoid(ptr, desc, desc_bytes)
    assert got.dtype == np.int32
    assert dict(zip(names, got.tolist())) == {k: hand[k][1] for k in names}


@pytest.mark.parametrize("desc_bytes", [4, 32, 40, 64])
def test_small_lists_and_the_wave_boundary(solver, desc_bytes):
    lists = MC.small_lists(desc_bytes) + MC.wave_lists(desc_bytes)   # n = 0 .. 5, 63, 64, 65
    ptr, desc = MC.pack(lists, desc_bytes)
    assert solver.desc_medoid(ptr, desc, desc_bytes).tolist() == RM.medoids(ptr, desc, desc_bytes).tolist()


@pytest.mark.parametrize("n", [1, 64, 65])
def test_batch_of_one(solver, n):
    lst = MC._noisy(40 + n, n, 32)
    ptr, desc = MC.pack([lst], 32)
    assert solver.desc_medoid(ptr, desc, 32).tolist() == [RM.medoid(lst)]


def test_empty_batch_and_a_batch_of_empty_lists(solver):
    assert solver.desc_medoid([0], np.zeros((0, 32), np.uint8), 32).tolist() == []
    assert solver.desc_medoid([0, 0, 0], np.zeros((0, 32), np.uint8), 32).tolist() == [-1, -1]


@pytest.mark.parametrize("desc_bytes", [32, 64])
def test_largest_list_and_one_above(solver, desc_bytes):
    big = MC._noisy(5, capi.MEDOID_MAX_N, desc_bytes, flips=60)
    # short lists around it, so that the long list's workgroup is not the only one
    lists = [MC._rand(6, 3, desc_bytes), big, MC._rand(7, 64, desc_bytes)]
    ptr, desc = MC.pack(lists, desc_bytes)
    assert solver.desc_medoid(ptr, desc, desc_bytes).tolist() == RM.medoids(ptr, desc, desc_bytes).tolist()
    over = np.concatenate([big, big[:1]])
    ptr, desc = MC.pack([lists[0], over], desc_bytes)
    with pytest.raises(PlbaError, match=f"{capi.MEDOID_MAX_N + 1} descriptors is more than {capi.MEDOID_MAX_N}"):
        solver.desc_medoid(ptr, desc, desc_bytes)
    # the refusal leaves the context usable
    ptr, desc = MC.pack(lists[:1], desc_bytes)
    assert solver.desc_medoid(ptr, desc, desc_bytes).tolist() == [RM.medoid(lists[0])]


def test_mixed_batch_of_300(solver):
    lists = MC.mixed_batch(32, n_lists=300)
    assert sum(len(l) == 0 for l in lists) >= 10 and sum(len(l) > 64 for l in lists) >= 10
    ptr, desc = MC.pack(lists, 32)
    assert solver.desc_medoid(ptr, desc, 32).tolist() == RM.medoids(ptr, desc, 32).tolist()


def test_invalid_arguments(solver):
    d = np.zeros((4, 32), np.uint8)
    for ptr, db in (([0, 3, 2], 32), ([-1, 2], 32), ([0, 2], 30)):
        with pytest.raises(PlbaError):
            solver.desc_medoid(ptr, d.reshape(-1), db)
