"""GPU box: wall time per call of plba_lc_relative_pose (upload, one launch, read-back, synchronise)
at (300 points, 100 lines) per candidate for batches of 1, 8 and 64 candidates.

The parent starts one child process per batch size, each under its own time limit, and stops at
the first one that fails; a child warms the shape up, then times `reps` calls with the host clock
around the call (it ends in a stream synchronise) and prints one JSON line. Recorded, not gated."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pl-slam-plucker_amd"))

SHAPE = (300, 100)
CHILD_LIMIT_S = 120


def child(batch: int, reps: int) -> None:
    import ctypes as C

    import numpy as np

    from plba import capi, lcpose
    from plba.lib import Solver
    probs = [lcpose.synth(SHAPE[0], SHAPE[1], seed=100 + i, rot_deg=5.0, trans=0.2, noise_px=1.0, outlier_frac=0.25)
             for i in range(batch)]
    bv = capi.LcposeBatchView(probs)
    p = capi.lcpose_params()
    out = (capi.PlbaLcposeOut * batch)()
    pin, lin = np.zeros(int(bv.pt_off[-1]), np.uint8), np.zeros(int(bv.ln_off[-1]), np.uint8)
    bp = C.POINTER(C.c_uint8)
    with Solver() as s:
        def call():
            rc = s.L.plba_lc_relative_pose(s.ctx, C.byref(bv.struct), C.byref(p), out, pin.ctypes.data_as(bp),
                                           lin.ctypes.data_as(bp))
            assert rc == 0, rc
        for _ in range(5):   # code object, device block and pinned image
            call()
        ms = []
        for _ in range(reps):
            t = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t) * 1e3)
    ms = np.sort(ms)
    print(json.dumps(dict(batch=batch, n_pt=SHAPE[0], n_ln=SHAPE[1], reps=reps, accepted=int(sum(o.accepted for o in out)),
                          passes=[int(out[0].iters_first), int(out[0].iters_ref)],
                          ms_median=round(float(np.median(ms)), 4), ms_p10=round(float(ms[len(ms) // 10]), 4),
                          ms_p90=round(float(ms[(9 * len(ms)) // 10]), 4),
                          us_per_candidate=round(float(np.median(ms)) * 1e3 / batch, 2))), flush=True)


def main() -> int:
    if len(sys.argv) >= 3 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 200)
        return 0
    sizes = [int(a) for a in sys.argv[1:]] or [1, 8, 64]
    for b in sizes:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(b)], timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(batch=b, error=f"time limit of {CHILD_LIMIT_S} s")), flush=True)
            return 1
        if r.returncode != 0:   # nothing more is started on the device after a failure
            print(json.dumps(dict(batch=b, error=f"exit status {r.returncode}")), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
