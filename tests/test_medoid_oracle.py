"""plslam_desc_medoid_cpu (the restatement of plba_desc_medoid) against the checker tests/ref_medoid.py,
and the hand cases with their answers written out. Integers: equality. Runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

import medoid_cases as MC
import ref_medoid as RM
from plba import capi, slam_map


@pytest.mark.parametrize("desc_bytes", [32, 64])
@pytest.mark.parametrize("name", sorted(MC.hand()))
def test_hand_cases_have_the_written_answer(name, desc_bytes):
    lst, want = MC.hand(desc_bytes)[name]
    assert RM.medoid(lst) == want
    ptr, desc = MC.pack([lst], desc_bytes)
    assert slam_map.desc_medoid_cpu(ptr, desc, desc_bytes).tolist() == [want]


def test_hand_cases_hold_what_they_are_meant_to():
    h = MC.hand()
    v = RM.row_values(h["four_tie_first_wins"][0])
    assert v.tolist() == [2, 1, 1, 2]                      # a tie for the minimum: the first index wins
    assert RM.row_values(h["five_chain"][0]).tolist() == [3, 2, 2, 2, 3]
    assert set(RM.row_values(h["equidistant"][0]).tolist()) == {2}   # only row 0 is < 99999 and < itself never
    assert set(RM.row_values(h["identical"][0]).tolist()) == {0}
    assert RM.row_values(h["last_is_best"][0]).argmin() == 3
    assert RM.table(MC.hand(64)["max_distance"][0]).max() == 512


@pytest.mark.parametrize("desc_bytes", [4, 32, 40, 64])
def test_small_and_wave_sized_lists_equal_the_checker(desc_bytes):
    lists = MC.small_lists(desc_bytes) + MC.wave_lists(desc_bytes)
    ptr, desc = MC.pack(lists, desc_bytes)
    got = slam_map.desc_medoid_cpu(ptr, desc, desc_bytes)
    assert got.tolist() == RM.medoids(ptr, desc, desc_bytes).tolist()
    assert [g for g, l in zip(got, lists) if len(l) == 0] == [-1, -1]


def test_mixed_batch_equals_the_checker_and_the_mirror_s_own_function():
    lists = MC.mixed_batch(32, n_lists=120)
    ptr, desc = MC.pack(lists, 32)
    got = slam_map.desc_medoid_cpu(ptr, desc, 32)
    assert got.tolist() == RM.medoids(ptr, desc, 32).tolist()
    # median_descriptor() of the package's Python model, which the existing host tests use
    for g, l in list(zip(got, lists))[:40]:
        if len(l):
            assert g == slam_map.median_descriptor(list(l))


def test_invalid_batches_are_refused():
    L = slam_map.load_host()
    ip = C.POINTER(C.c_int32)
    out = np.zeros(4, np.int32)
    for ptr, db in (([0, 2, 1], 32), ([-1, 1], 32), ([0, 1], 30), ([0, 1], 68), ([0, capi.MEDOID_MAX_N + 1], 32)):
        n = max(ptr)
        bv = capi.MedoidBatchView(ptr, np.zeros((max(n, 1), 128), np.uint8), db)
        assert L.plslam_desc_medoid_cpu(None, C.byref(bv.struct), out.ctypes.data_as(ip)) != 0, (ptr, db)
