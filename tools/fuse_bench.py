"""GPU box: the median descriptors of a landmark fusion, three ways, on 300 fused landmarks whose tracks
have 2 .. 128 observations in all (a observations of the kept landmark, b appended from the erased one):

  per_append   what loopClosureFuseLandmarks does: updateAverageDescDir after each of the b appends, i.e.
               the table and the row sorts for a + 1, a + 2, ..., a + b descriptors
               (plslam_desc_medoid_cpu, single-threaded, on every prefix);
  once_cpu     the same function once per landmark, on the final list, which is all that can be observed;
  device       plba_desc_medoid on the batch of final lists: upload, one launch, read-back, synchronise.

The parent starts one child process under a time limit; the child checks that the three agree, times
each with the host clock and prints one JSON line. Recorded, not gated."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pl-slam-plucker_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_LANDMARKS, MAX_TRACK, DESC_BYTES = 300, 128, 32
CHILD_LIMIT_S = 240


def child(reps: int) -> None:
    import ctypes as C

    import numpy as np

    import medoid_cases as MC
    from plba import capi
    from plba.lib import Solver
    from plba.slam_map import load_host
    H = load_host()
    ip = C.POINTER(C.c_int32)
    rng = np.random.default_rng(1)
    totals = rng.integers(2, MAX_TRACK + 1, N_LANDMARKS)
    kept = [int(rng.integers(1, n)) for n in totals]                      # a; b = n - a >= 1
    lists = [MC._noisy(50 + i, int(n), DESC_BYTES, flips=30) for i, n in enumerate(totals)]
    final = capi.MedoidBatchView(*MC.pack(lists, DESC_BYTES), DESC_BYTES)
    prefixes = [capi.MedoidBatchView(*MC.pack([l[:k] for k in range(a + 1, len(l) + 1)], DESC_BYTES), DESC_BYTES)
                for l, a in zip(lists, kept)]

    def timed(fn, n):
        ms = []
        for _ in range(n):
            t = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t) * 1e3)
        return np.sort(ms)

    out_append = [np.zeros(p.struct.n, np.int32) for p in prefixes]
    out_cpu, out_dev = np.zeros(N_LANDMARKS, np.int32), np.zeros(N_LANDMARKS, np.int32)

    def per_append():
        for p, o in zip(prefixes, out_append):
            assert H.plslam_desc_medoid_cpu(None, C.byref(p.struct), o.ctypes.data_as(ip)) == 0

    def once_cpu():
        assert H.plslam_desc_medoid_cpu(None, C.byref(final.struct), out_cpu.ctypes.data_as(ip)) == 0

    with Solver() as s:
        def device():
            rc = s.L.plba_desc_medoid(s.ctx, C.byref(final.struct), out_dev.ctypes.data_as(ip))
            assert rc == 0, rc
        per_append()
        append_ms = timed(per_append, 3)
        once_cpu()
        cpu_ms = timed(once_cpu, 10)
        for _ in range(5):   # code object, device block and pinned image
            device()
        ms = timed(device, reps)
    assert out_dev.tobytes() == out_cpu.tobytes() and all(o[-1] == v for o, v in zip(out_append, out_cpu))
    print(json.dumps(dict(landmarks=N_LANDMARKS, track=[2, MAX_TRACK], desc_bytes=DESC_BYTES, reps=reps,
                          descriptors=int(totals.sum()), appended=int(sum(n - a for n, a in zip(totals, kept))),
                          per_append_cpu_1thread_ms_median=round(float(np.median(append_ms)), 3),
                          once_cpu_1thread_ms_median=round(float(np.median(cpu_ms)), 3),
                          device_ms_median=round(float(np.median(ms)), 4), device_ms_p10=round(float(ms[len(ms) // 10]), 4),
                          device_ms_p90=round(float(ms[(9 * len(ms)) // 10]), 4), all_equal=True)), flush=True)


def main() -> int:
    if len(sys.argv) >= 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]) if len(sys.argv) > 2 else 200)
        return 0
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:2], timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired:
        print(json.dumps(dict(landmarks=N_LANDMARKS, error=f"time limit of {CHILD_LIMIT_S} s")), flush=True)
        return 1
    if r.returncode != 0:
        print(json.dumps(dict(landmarks=N_LANDMARKS, error=f"exit status {r.returncode}")), flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
