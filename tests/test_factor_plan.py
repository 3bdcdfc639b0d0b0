"""The factorisation choice of an upload (plan_factor in csrc/plba_plan.hpp), pinned through
plba_factor_plan: no context, no device, so it runs where there is no GPU.

TABLE was recorded from the selection code as it stood BEFORE plan_factor existed (use_cl,
want_bcr, spec_choice and the inline block of do_upload, wrapped by a plba_factor_plan that called
them untouched); plan_factor must reproduce every row. Rows: the (bw, nf) of C1/C1L, C2, C3, C4,
C5, C2R and C3R as plba_structure_stats reports them; bw at the kClMaxBW / band_nt / kBandMax edges;
nf on both sides of the two-sided threshold 2*bw+16; resident = N-1 and N, and resident/N = 1, 2, 4
(the trial-slot cap); sharded, no_bcr and no-triples windows; and every switch that enters the
choice. flags: 1 no_bcr, 2 sharded, 4 has Schur triples. Modes: 0 dense scalar, 1 dense MFMA,
2 band, 3 band two-sided, 4 column-lane, 5 column-lane two-sided, 6 block cyclic reduction.
"""
import ctypes
import os

import pytest

from plba import lib

NO_BCR = 1

# (bw, nf, resident, flags, env) -> (mode, bcr_N, bcr_fused, tw_m, ring, slots, policy, fb_mode, fb_tw_m)
TABLE = [
    (7, 9, 256, 4, {}, (4, 0, 0, 0, 16, 2, 3, -1, 0)),
    (7, 45, 256, 4, {}, (5, 0, 0, 19, 16, 2, 3, -1, 0)),
    (7, 90, 256, 4, {}, (5, 0, 0, 42, 16, 2, 3, -1, 0)),
    (7, 360, 256, 4, {}, (6, 52, 1, 0, 16, 4, 3, 5, 177)),
    (7, 900, 256, 4, {}, (6, 129, 1, 0, 16, 1, 0, 5, 447)),
    (20, 135, 256, 4, {}, (3, 0, 0, 58, 16, 4, 3, -1, 0)),
    (23, 144, 256, 4, {}, (3, 0, 0, 61, 16, 4, 3, -1, 0)),
    (0, 200, 256, 4, {}, (2, 0, 0, 0, 16, 4, 3, -1, 0)),
    (1, 200, 256, 4, {}, (6, 200, 1, 0, 16, 1, 0, 5, 100)),
    (9, 200, 256, 4, {}, (5, 0, 0, 96, 16, 2, 3, -1, 0)),
    (10, 200, 256, 4, {}, (3, 0, 0, 95, 16, 4, 3, -1, 0)),
    (11, 200, 256, 4, {}, (3, 0, 0, 95, 16, 4, 3, -1, 0)),
    (24, 200, 256, 4, {}, (3, 0, 0, 88, 15, 4, 3, -1, 0)),
    (25, 200, 256, 4, {}, (3, 0, 0, 88, 14, 4, 3, -1, 0)),
    (27, 200, 256, 4, {}, (3, 0, 0, 87, 13, 4, 3, -1, 0)),
    (28, 200, 256, 4, {}, (1, 0, 0, 0, 12, 1, 0, -1, 0)),
    (1, 17, 256, 4, {}, (4, 0, 0, 0, 16, 2, 3, -1, 0)),
    (1, 17, 256, 5, {}, (4, 0, 0, 0, 16, 2, 3, -1, 0)),
    (1, 18, 256, 4, {}, (5, 0, 0, 9, 16, 2, 3, -1, 0)),
    (1, 18, 256, 5, {}, (5, 0, 0, 9, 16, 2, 3, -1, 0)),
    (7, 29, 256, 4, {}, (4, 0, 0, 0, 16, 2, 3, -1, 0)),
    (7, 29, 256, 5, {}, (4, 0, 0, 0, 16, 2, 3, -1, 0)),
    (7, 30, 256, 4, {}, (5, 0, 0, 12, 16, 2, 3, -1, 0)),
    (7, 30, 256, 5, {}, (5, 0, 0, 12, 16, 2, 3, -1, 0)),
    (9, 33, 256, 4, {}, (4, 0, 0, 0, 16, 2, 3, -1, 0)),
    (9, 33, 256, 5, {}, (4, 0, 0, 0, 16, 2, 3, -1, 0)),
    (9, 34, 256, 4, {}, (5, 0, 0, 13, 16, 2, 3, -1, 0)),
    (9, 34, 256, 5, {}, (5, 0, 0, 13, 16, 2, 3, -1, 0)),
    (10, 35, 256, 4, {}, (2, 0, 0, 0, 16, 4, 3, -1, 0)),
    (10, 35, 256, 5, {}, (2, 0, 0, 0, 16, 4, 3, -1, 0)),
    (10, 36, 256, 4, {}, (3, 0, 0, 13, 16, 4, 3, -1, 0)),
    (10, 36, 256, 5, {}, (3, 0, 0, 13, 16, 4, 3, -1, 0)),
    (20, 55, 256, 4, {}, (2, 0, 0, 0, 16, 4, 3, -1, 0)),
    (20, 55, 256, 5, {}, (2, 0, 0, 0, 16, 4, 3, -1, 0)),
    (20, 56, 256, 4, {}, (3, 0, 0, 18, 16, 4, 3, -1, 0)),
    (20, 56, 256, 5, {}, (3, 0, 0, 18, 16, 4, 3, -1, 0)),
    (27, 69, 256, 4, {}, (2, 0, 0, 0, 13, 4, 3, -1, 0)),
    (27, 69, 256, 5, {}, (2, 0, 0, 0, 13, 4, 3, -1, 0)),
    (27, 70, 256, 4, {}, (3, 0, 0, 22, 13, 4, 3, -1, 0)),
    (27, 70, 256, 5, {}, (3, 0, 0, 22, 13, 4, 3, -1, 0)),
    (7, 360, 51, 4, {}, (5, 0, 0, 177, 16, 2, 3, -1, 0)),
    (7, 360, 52, 4, {}, (6, 52, 1, 0, 16, 1, 0, 5, 177)),
    (7, 360, 103, 4, {}, (6, 52, 1, 0, 16, 1, 0, 5, 177)),
    (7, 360, 104, 4, {}, (6, 52, 1, 0, 16, 2, 3, 5, 177)),
    (7, 360, 207, 4, {}, (6, 52, 1, 0, 16, 3, 3, 5, 177)),
    (7, 360, 208, 4, {}, (6, 52, 1, 0, 16, 4, 3, 5, 177)),
    (7, 900, 128, 4, {}, (5, 0, 0, 447, 16, 2, 3, -1, 0)),
    (7, 900, 129, 4, {}, (6, 129, 1, 0, 16, 1, 0, 5, 447)),
    (7, 900, 258, 4, {}, (6, 129, 1, 0, 16, 2, 3, 5, 447)),
    (7, 90, 256, 6, {}, (5, 0, 0, 42, 16, 1, 0, -1, 0)),
    (7, 360, 256, 6, {}, (6, 52, 1, 0, 16, 1, 0, 5, 177)),
    (23, 144, 256, 6, {}, (3, 0, 0, 61, 16, 1, 0, -1, 0)),
    (7, 90, 256, 5, {}, (5, 0, 0, 42, 16, 2, 3, -1, 0)),
    (7, 360, 256, 5, {}, (5, 0, 0, 177, 16, 2, 3, -1, 0)),
    (23, 144, 256, 5, {}, (3, 0, 0, 61, 16, 4, 3, -1, 0)),
    (7, 90, 256, 0, {}, (5, 0, 0, 42, 16, 1, 0, -1, 0)),
    (7, 360, 256, 0, {}, (6, 52, 1, 0, 16, 1, 0, 5, 177)),
    (23, 144, 256, 0, {}, (3, 0, 0, 61, 16, 1, 0, -1, 0)),
    (7, 90, 256, 2, {}, (5, 0, 0, 42, 16, 1, 0, -1, 0)),
    (7, 360, 256, 2, {}, (6, 52, 1, 0, 16, 1, 0, 5, 177)),
    (23, 144, 256, 2, {}, (3, 0, 0, 61, 16, 1, 0, -1, 0)),
    (7, 90, 256, 7, {}, (5, 0, 0, 42, 16, 1, 0, -1, 0)),
    (7, 360, 256, 7, {}, (5, 0, 0, 177, 16, 1, 0, -1, 0)),
    (23, 144, 256, 7, {}, (3, 0, 0, 61, 16, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_FACTOR': 'bcr'}, (6, 13, 1, 0, 16, 4, 3, 5, 42)),
    (7, 360, 256, 4, {'PLBA_FACTOR': 'bcr'}, (6, 52, 1, 0, 16, 4, 3, 5, 177)),
    (23, 144, 256, 4, {'PLBA_FACTOR': 'bcr'}, (3, 0, 0, 61, 16, 4, 3, -1, 0)),
    (10, 200, 256, 4, {'PLBA_FACTOR': 'bcr'}, (3, 0, 0, 95, 16, 4, 3, -1, 0)),
    (28, 200, 256, 4, {'PLBA_FACTOR': 'bcr'}, (1, 0, 0, 0, 12, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_FACTOR': 'cl'}, (5, 0, 0, 42, 16, 2, 3, -1, 0)),
    (7, 360, 256, 4, {'PLBA_FACTOR': 'cl'}, (5, 0, 0, 177, 16, 2, 3, -1, 0)),
    (23, 144, 256, 4, {'PLBA_FACTOR': 'cl'}, (3, 0, 0, 61, 16, 4, 3, -1, 0)),
    (10, 200, 256, 4, {'PLBA_FACTOR': 'cl'}, (3, 0, 0, 95, 16, 4, 3, -1, 0)),
    (28, 200, 256, 4, {'PLBA_FACTOR': 'cl'}, (1, 0, 0, 0, 12, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_FACTOR': 'band'}, (3, 0, 0, 42, 16, 4, 3, -1, 0)),
    (7, 360, 256, 4, {'PLBA_FACTOR': 'band'}, (3, 0, 0, 177, 16, 4, 3, -1, 0)),
    (23, 144, 256, 4, {'PLBA_FACTOR': 'band'}, (3, 0, 0, 61, 16, 4, 3, -1, 0)),
    (10, 200, 256, 4, {'PLBA_FACTOR': 'band'}, (3, 0, 0, 95, 16, 4, 3, -1, 0)),
    (28, 200, 256, 4, {'PLBA_FACTOR': 'band'}, (1, 0, 0, 0, 12, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_NO_CL': '1'}, (3, 0, 0, 42, 16, 4, 3, -1, 0)),
    (7, 360, 256, 4, {'PLBA_NO_CL': '1'}, (6, 52, 1, 0, 16, 4, 3, 2, 0)),
    (23, 144, 256, 4, {'PLBA_NO_CL': '1'}, (3, 0, 0, 61, 16, 4, 3, -1, 0)),
    (10, 200, 256, 4, {'PLBA_NO_CL': '1'}, (3, 0, 0, 95, 16, 4, 3, -1, 0)),
    (28, 200, 256, 4, {'PLBA_NO_CL': '1'}, (1, 0, 0, 0, 12, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_NO_TWIST': '1'}, (4, 0, 0, 0, 16, 2, 3, -1, 0)),
    (7, 360, 256, 4, {'PLBA_NO_TWIST': '1'}, (6, 52, 1, 0, 16, 4, 3, 4, 0)),
    (23, 144, 256, 4, {'PLBA_NO_TWIST': '1'}, (2, 0, 0, 0, 16, 4, 3, -1, 0)),
    (10, 200, 256, 4, {'PLBA_NO_TWIST': '1'}, (2, 0, 0, 0, 16, 4, 3, -1, 0)),
    (28, 200, 256, 4, {'PLBA_NO_TWIST': '1'}, (1, 0, 0, 0, 12, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_BCR_SPLIT': '1'}, (5, 0, 0, 42, 16, 2, 3, -1, 0)),
    (7, 360, 256, 4, {'PLBA_BCR_SPLIT': '1'}, (6, 52, 0, 0, 16, 4, 3, 5, 177)),
    (23, 144, 256, 4, {'PLBA_BCR_SPLIT': '1'}, (3, 0, 0, 61, 16, 4, 3, -1, 0)),
    (10, 200, 256, 4, {'PLBA_BCR_SPLIT': '1'}, (3, 0, 0, 95, 16, 4, 3, -1, 0)),
    (28, 200, 256, 4, {'PLBA_BCR_SPLIT': '1'}, (1, 0, 0, 0, 12, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_SPEC': '1'}, (5, 0, 0, 42, 16, 1, 0, -1, 0)),
    (7, 360, 256, 4, {'PLBA_SPEC': '1'}, (6, 52, 1, 0, 16, 1, 0, 5, 177)),
    (23, 144, 256, 4, {'PLBA_SPEC': '1'}, (3, 0, 0, 61, 16, 1, 0, -1, 0)),
    (10, 200, 256, 4, {'PLBA_SPEC': '1'}, (3, 0, 0, 95, 16, 1, 0, -1, 0)),
    (28, 200, 256, 4, {'PLBA_SPEC': '1'}, (1, 0, 0, 0, 12, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_SPEC': '3'}, (5, 0, 0, 42, 16, 3, 3, -1, 0)),
    (7, 360, 256, 4, {'PLBA_SPEC': '3'}, (6, 52, 1, 0, 16, 3, 3, 5, 177)),
    (23, 144, 256, 4, {'PLBA_SPEC': '3'}, (3, 0, 0, 61, 16, 3, 3, -1, 0)),
    (10, 200, 256, 4, {'PLBA_SPEC': '3'}, (3, 0, 0, 95, 16, 3, 3, -1, 0)),
    (28, 200, 256, 4, {'PLBA_SPEC': '3'}, (1, 0, 0, 0, 12, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_SPEC_POLICY': '0'}, (5, 0, 0, 42, 16, 1, 0, -1, 0)),
    (7, 360, 256, 4, {'PLBA_SPEC_POLICY': '0'}, (6, 52, 1, 0, 16, 1, 0, 5, 177)),
    (23, 144, 256, 4, {'PLBA_SPEC_POLICY': '0'}, (3, 0, 0, 61, 16, 1, 0, -1, 0)),
    (10, 200, 256, 4, {'PLBA_SPEC_POLICY': '0'}, (3, 0, 0, 95, 16, 1, 0, -1, 0)),
    (28, 200, 256, 4, {'PLBA_SPEC_POLICY': '0'}, (1, 0, 0, 0, 12, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_SPEC_POLICY': '1'}, (5, 0, 0, 42, 16, 2, 1, -1, 0)),
    (7, 360, 256, 4, {'PLBA_SPEC_POLICY': '1'}, (6, 52, 1, 0, 16, 4, 1, 5, 177)),
    (23, 144, 256, 4, {'PLBA_SPEC_POLICY': '1'}, (3, 0, 0, 61, 16, 4, 1, -1, 0)),
    (10, 200, 256, 4, {'PLBA_SPEC_POLICY': '1'}, (3, 0, 0, 95, 16, 4, 1, -1, 0)),
    (28, 200, 256, 4, {'PLBA_SPEC_POLICY': '1'}, (1, 0, 0, 0, 12, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_SPEC_BCR': '0'}, (5, 0, 0, 42, 16, 2, 3, -1, 0)),
    (7, 360, 256, 4, {'PLBA_SPEC_BCR': '0'}, (6, 52, 1, 0, 16, 1, 0, 5, 177)),
    (23, 144, 256, 4, {'PLBA_SPEC_BCR': '0'}, (3, 0, 0, 61, 16, 4, 3, -1, 0)),
    (10, 200, 256, 4, {'PLBA_SPEC_BCR': '0'}, (3, 0, 0, 95, 16, 4, 3, -1, 0)),
    (28, 200, 256, 4, {'PLBA_SPEC_BCR': '0'}, (1, 0, 0, 0, 12, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_FORCE_DENSE': '1'}, (1, 0, 0, 0, 16, 1, 0, -1, 0)),
    (7, 360, 256, 4, {'PLBA_FORCE_DENSE': '1'}, (1, 0, 0, 0, 16, 1, 0, -1, 0)),
    (23, 144, 256, 4, {'PLBA_FORCE_DENSE': '1'}, (1, 0, 0, 0, 16, 1, 0, -1, 0)),
    (10, 200, 256, 4, {'PLBA_FORCE_DENSE': '1'}, (1, 0, 0, 0, 16, 1, 0, -1, 0)),
    (28, 200, 256, 4, {'PLBA_FORCE_DENSE': '1'}, (1, 0, 0, 0, 12, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_DENSE_SCALAR': '1'}, (5, 0, 0, 42, 16, 2, 3, -1, 0)),
    (7, 360, 256, 4, {'PLBA_DENSE_SCALAR': '1'}, (6, 52, 1, 0, 16, 4, 3, 5, 177)),
    (23, 144, 256, 4, {'PLBA_DENSE_SCALAR': '1'}, (3, 0, 0, 61, 16, 4, 3, -1, 0)),
    (10, 200, 256, 4, {'PLBA_DENSE_SCALAR': '1'}, (3, 0, 0, 95, 16, 4, 3, -1, 0)),
    (28, 200, 256, 4, {'PLBA_DENSE_SCALAR': '1'}, (0, 0, 0, 0, 12, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_DENSE_SCALAR': '1', 'PLBA_FORCE_DENSE': '1'}, (0, 0, 0, 0, 16, 1, 0, -1, 0)),
    (7, 360, 256, 4, {'PLBA_DENSE_SCALAR': '1', 'PLBA_FORCE_DENSE': '1'}, (0, 0, 0, 0, 16, 1, 0, -1, 0)),
    (23, 144, 256, 4, {'PLBA_DENSE_SCALAR': '1', 'PLBA_FORCE_DENSE': '1'}, (0, 0, 0, 0, 16, 1, 0, -1, 0)),
    (10, 200, 256, 4, {'PLBA_DENSE_SCALAR': '1', 'PLBA_FORCE_DENSE': '1'}, (0, 0, 0, 0, 16, 1, 0, -1, 0)),
    (28, 200, 256, 4, {'PLBA_DENSE_SCALAR': '1', 'PLBA_FORCE_DENSE': '1'}, (0, 0, 0, 0, 12, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_BCR_RESIDENT': '60'}, (5, 0, 0, 42, 16, 2, 3, -1, 0)),
    (7, 360, 256, 4, {'PLBA_BCR_RESIDENT': '60'}, (6, 52, 1, 0, 16, 1, 0, 5, 177)),
    (23, 144, 256, 4, {'PLBA_BCR_RESIDENT': '60'}, (3, 0, 0, 61, 16, 4, 3, -1, 0)),
    (10, 200, 256, 4, {'PLBA_BCR_RESIDENT': '60'}, (3, 0, 0, 95, 16, 4, 3, -1, 0)),
    (28, 200, 256, 4, {'PLBA_BCR_RESIDENT': '60'}, (1, 0, 0, 0, 12, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_BCR_SPLIT': '1'}, (6, 13, 0, 0, 16, 4, 3, 5, 42)),
    (7, 360, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_BCR_SPLIT': '1'}, (6, 52, 0, 0, 16, 4, 3, 5, 177)),
    (23, 144, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_BCR_SPLIT': '1'}, (3, 0, 0, 61, 16, 4, 3, -1, 0)),
    (10, 200, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_BCR_SPLIT': '1'}, (3, 0, 0, 95, 16, 4, 3, -1, 0)),
    (28, 200, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_BCR_SPLIT': '1'}, (1, 0, 0, 0, 12, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_NO_CL': '1'}, (6, 13, 1, 0, 16, 4, 3, 2, 0)),
    (7, 360, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_NO_CL': '1'}, (6, 52, 1, 0, 16, 4, 3, 2, 0)),
    (23, 144, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_NO_CL': '1'}, (3, 0, 0, 61, 16, 4, 3, -1, 0)),
    (10, 200, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_NO_CL': '1'}, (3, 0, 0, 95, 16, 4, 3, -1, 0)),
    (28, 200, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_NO_CL': '1'}, (1, 0, 0, 0, 12, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_NO_TWIST': '1'}, (6, 13, 1, 0, 16, 4, 3, 4, 0)),
    (7, 360, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_NO_TWIST': '1'}, (6, 52, 1, 0, 16, 4, 3, 4, 0)),
    (23, 144, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_NO_TWIST': '1'}, (2, 0, 0, 0, 16, 4, 3, -1, 0)),
    (10, 200, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_NO_TWIST': '1'}, (2, 0, 0, 0, 16, 4, 3, -1, 0)),
    (28, 200, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_NO_TWIST': '1'}, (1, 0, 0, 0, 12, 1, 0, -1, 0)),
    (7, 90, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_SPEC_BCR': '0', 'PLBA_BCR_SPLIT': '1'}, (6, 13, 0, 0, 16, 1, 0, 5, 42)),
    (7, 360, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_SPEC_BCR': '0', 'PLBA_BCR_SPLIT': '1'}, (6, 52, 0, 0, 16, 1, 0, 5, 177)),
    (23, 144, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_SPEC_BCR': '0', 'PLBA_BCR_SPLIT': '1'}, (3, 0, 0, 61, 16, 4, 3, -1, 0)),
    (10, 200, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_SPEC_BCR': '0', 'PLBA_BCR_SPLIT': '1'}, (3, 0, 0, 95, 16, 4, 3, -1, 0)),
    (28, 200, 256, 4, {'PLBA_FACTOR': 'bcr', 'PLBA_SPEC_BCR': '0', 'PLBA_BCR_SPLIT': '1'}, (1, 0, 0, 0, 12, 1, 0, -1, 0)),
]


def _plan(monkeypatch, bw, nf, resident, flags, env):
    for k in [k for k in os.environ if k.startswith("PLBA_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = (ctypes.c_int32 * 9)(*([-99] * 9))
    assert lib.load().plba_factor_plan(bw, nf, resident, flags, out, 9) == 0
    return tuple(out)


@pytest.fixture(autouse=True)
def _needs_library():
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("libplba.so not built (run __graft_entry__.build())")


def test_plan_matches_the_recorded_choice(monkeypatch):
    bad = [(row[:5], row[5], got) for row in TABLE if (got := _plan(monkeypatch, *row[:5])) != row[5]]
    assert not bad, bad


def test_c3_by_hand(monkeypatch):
    """C3: bw 7, nf 90, N = 13 super-rows, 5 levels: t_bcr = 5*(2.6*7+4.8) = 115 against
    t_cl = 1.3*97/2 = 63.05 -> column-lane, two-sided, split row (90-7+1)/2 = 42, two trial
    slots, sticky policy (3); no fallback."""
    assert _plan(monkeypatch, 7, 90, 256, 4, {}) == (5, 0, 0, 42, 16, 2, 3, -1, 0)


def test_bcr_fallback_is_the_plan_without_bcr(monkeypatch):
    """A BCR window falls back to the factorisation the same inputs give when BCR is ruled out.
    The one exception is kept from the code this replaced: without the column-lane kernel
    (PLBA_NO_CL=1) the fallback is the one-sweep band kernel (mode 2), never the two-sided one."""
    rows = [r for r in TABLE if r[5][0] == 6]
    assert len(rows) >= 20
    for bw, nf, resident, flags, env, exp in rows:
        other = _plan(monkeypatch, bw, nf, resident, flags | NO_BCR, env)
        assert other[0] != 6
        if env.get("PLBA_NO_CL") == "1":
            assert exp[7:] == (2, 0) and other[0] in (2, 3), (bw, nf, env, exp, other)
        else:
            assert exp[7:] == (other[0], other[3]), (bw, nf, env, exp, other)


def test_unwritten_entries_and_bad_arguments():
    L = lib.load()
    out = (ctypes.c_int32 * 9)(*([-99] * 9))
    assert L.plba_factor_plan(7, 90, 256, 4, out, 4) == 0
    assert tuple(out)[:4] == (5, 0, 0, 42) and tuple(out)[4:] == (-99,) * 5
    assert L.plba_factor_plan(7, 90, 256, 4, None, 9) != 0
    assert L.plba_factor_plan(-1, 90, 256, 4, out, 9) != 0
