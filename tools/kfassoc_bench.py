"""GPU box: wall time per call of plba_kf_associate (packing, upload, the launches, read-back, synchronise,
the copy to the caller's arrays) on one keyframe pair of 1000 + 1000 points and 200 + 200 lines, and on a
batch of 8 such pairs; next to the single-threaded C++ restatement of the host mirror (plslam_kf_assoc_cpu)
on the same batch in the same process.

The parent starts one child process under a time limit; the child warms each shape up, then times `reps`
calls with the host clock around the call (it ends in a stream synchronise), checks the device result
against the CPU one byte for byte, and prints one JSON line per shape. Recorded, not gated."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pl-slam-plucker_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPE = dict(pt=(1000, 1000), ls=(200, 200))
CHILD_LIMIT_S = 240


def child(reps: int) -> None:
    import ctypes as C

    import numpy as np

    import kfassoc_cases as KC
    from plba import capi
    from plba.lib import Solver
    from plba.slam_map import load_host
    H = load_host()
    prm = capi.kfassoc_params(KC.CAMERA)

    def timed(fn, n):
        ms = []
        for _ in range(n):
            t = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t) * 1e3)
        return np.sort(ms)

    with Solver() as s:
        for pairs in (1, 8):
            ps = [KC.pair(100 + seed, SHAPE["pt"], SHAPE["ls"]) for seed in range(pairs)]
            dev, cpu = capi.KfassocBatchView(ps), capi.KfassocBatchView(ps)

            def cpu_call():
                assert H.plslam_kf_assoc_cpu(None, C.byref(cpu.struct), C.byref(prm), C.byref(cpu.out)) == 0

            def call():
                rc = s.L.plba_kf_associate(s.ctx, C.byref(dev.struct), C.byref(prm), C.byref(dev.out))
                assert rc == 0, rc
            cpu_call()
            cpu_ms = timed(cpu_call, 5)
            for _ in range(5):   # code object, device block and pinned image
                call()
            ms = timed(call, reps)
            assert all(dev.o[k].tobytes() == cpu.o[k].tobytes() for k in dev.o)
            a = dev.results()
            print(json.dumps(dict(points=SHAPE["pt"], lines=SHAPE["ls"], pairs=pairs, reps=reps,
                                  n_matches=[r["n_matches"] for r in a], fallback=[r["fallback"] for r in a],
                                  ms_median=round(float(np.median(ms)), 4), ms_p10=round(float(ms[len(ms) // 10]), 4),
                                  ms_p90=round(float(ms[(9 * len(ms)) // 10]), 4),
                                  cpu_1thread_ms_median=round(float(np.median(cpu_ms)), 3), cpu_reps=len(cpu_ms),
                                  equal_to_cpu=True)), flush=True)


def main() -> int:
    if len(sys.argv) >= 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]) if len(sys.argv) > 2 else 200)
        return 0
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:2], timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired:
        print(json.dumps(dict(SHAPE, error=f"time limit of {CHILD_LIMIT_S} s")), flush=True)
        return 1
    if r.returncode != 0:
        print(json.dumps(dict(SHAPE, error=f"exit status {r.returncode}")), flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
