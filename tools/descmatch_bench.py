"""GPU box: wall time per call of plba_desc_match (upload, two launches, read-back, synchronise) for
the matching of isLoopClosure over K candidates, (600 points + 150 lines) per keyframe, 2K pairs per
call, K = 1, 8 and 64; next to the single-threaded C++ popcount restatement of the host mirror
(plslam_desc_match_cpu) on the same batch in the same process.

The parent starts one child process per K, each under its own time limit, and stops at the first
one that fails; a child warms the shape up, then times `reps` calls with the host clock around the
call (it ends in a stream synchronise), checks the device result against the CPU one, and prints
one JSON line. Recorded, not gated."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pl-slam-plucker_amd"))

SHAPE = (600, 150)
CHILD_LIMIT_S = 240


def keyframe_pairs(k: int, seed: int = 0):
    """2k pairs: the 32-byte descriptors of an old keyframe against those of the new one; half of the
    rows are true matches (copies with up to 4 flipped bits), the rest random."""
    import numpy as np
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(k):
        for n in SHAPE:
            d2 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            h = n // 2
            flips = ((rng.integers(0, 16, (h, 32)) == 0) * (1 << rng.integers(0, 8, (h, 32)))).astype(np.uint8)
            d1[rng.permutation(n)[:h]] = d2[rng.permutation(n)[:h]] ^ flips   # about 2 flipped bits per row
            pairs.append((d1, d2))
    return pairs


def child(k: int, reps: int) -> None:
    import ctypes as C

    import numpy as np

    from plba import capi
    from plba.lib import Solver
    from plba.slam_map import load_host
    bv = capi.MatchBatchView(keyframe_pairs(k), 0.9, True)
    ip = C.POINTER(C.c_int32)
    m12, cnt = np.zeros(int(bv.off1[-1]), np.int32), np.zeros(2 * k, np.int32)
    m12_cpu, cnt_cpu = np.zeros_like(m12), np.zeros_like(cnt)
    H = load_host()

    def timed(fn, n):
        ms = []
        for _ in range(n):
            t = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t) * 1e3)
        return np.sort(ms)

    def cpu_call():
        assert H.plslam_desc_match_cpu(None, C.byref(bv.struct), m12_cpu.ctypes.data_as(ip), cnt_cpu.ctypes.data_as(ip)) == 0
    cpu_call()
    cpu_ms = timed(cpu_call, max(3, min(20, 160 // k)))
    with Solver() as s:
        def call():
            rc = s.L.plba_desc_match(s.ctx, C.byref(bv.struct), m12.ctypes.data_as(ip), cnt.ctypes.data_as(ip))
            assert rc == 0, rc
        for _ in range(5):   # code object, device block and pinned image
            call()
        ms = timed(call, reps)
    assert np.array_equal(m12, m12_cpu) and np.array_equal(cnt, cnt_cpu)
    print(json.dumps(dict(candidates=k, pairs=2 * k, n_pt=SHAPE[0], n_ln=SHAPE[1], reps=reps, matches=int(cnt.sum()),
                          rows=int(bv.off1[-1]), ms_median=round(float(np.median(ms)), 4),
                          ms_p10=round(float(ms[len(ms) // 10]), 4), ms_p90=round(float(ms[(9 * len(ms)) // 10]), 4),
                          us_per_candidate=round(float(np.median(ms)) * 1e3 / k, 2),
                          cpu_1thread_ms_median=round(float(np.median(cpu_ms)), 3), cpu_reps=len(cpu_ms),
                          equal_to_cpu=True)), flush=True)


def main() -> int:
    if len(sys.argv) >= 3 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 200)
        return 0
    sizes = [int(a) for a in sys.argv[1:]] or [1, 8, 64]
    for k in sizes:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(k)], timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(candidates=k, error=f"time limit of {CHILD_LIMIT_S} s")), flush=True)
            return 1
        if r.returncode != 0:   # nothing more is started on the device after a failure
            print(json.dumps(dict(candidates=k, error=f"exit status {r.returncode}")), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
