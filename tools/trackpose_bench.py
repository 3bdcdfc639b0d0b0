"""GPU box: wall time per call of plba_track_pose (upload, one launch, read-back, synchronise) at
(300 points, 100 lines) per frame pair for batches of 1, 8 and 64 problems, against the single-threaded
C++ restatement plslam_track_pose_cpu on the same batch in the same process.

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


def child(batch: int, reps: int, model: int) -> None:
    import ctypes as C

    import numpy as np

    from plba import capi, trackpose
    from plba.lib import Solver
    from plba.slam_map import load_host
    probs = [trackpose.synth(SHAPE[0], SHAPE[1], seed=100 + i, outlier_frac=0.2) for i in range(batch)]
    bv = capi.TrackBatchView(probs)
    p = capi.track_params(line_model=model)
    out = (capi.PlbaTrackOut * batch)()
    out_cpu = (capi.PlbaTrackOut * batch)()
    pin, lin = np.zeros(int(bv.pt_off[-1]), np.uint8), np.zeros(int(bv.ln_off[-1]), np.uint8)
    bp = C.POINTER(C.c_uint8)
    H = load_host()

    def timed(fn, n):
        ms = []
        for _ in range(n):
            t = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t) * 1e3)
        return np.sort(ms)

    with Solver() as s:
        def call():
            rc = s.L.plba_track_pose(s.ctx, C.byref(bv.struct), C.byref(p), out, pin.ctypes.data_as(bp),
                                     lin.ctypes.data_as(bp))
            assert rc == 0, rc

        def call_cpu():
            assert H.plslam_track_pose_cpu(None, C.byref(bv.struct), C.byref(p), out_cpu, None, None) == 0
        for _ in range(5):   # code object, device block and pinned image
            call()
        ms = timed(call, reps)
        call_cpu()
        ms_cpu = timed(call_cpu, max(3, reps // 20))
    same = all(out[i].branch == out_cpu[i].branch and out[i].n_inl_pt == out_cpu[i].n_inl_pt for i in range(batch))
    print(json.dumps(dict(batch=batch, n_pt=SHAPE[0], n_ln=SHAPE[1], line_model=model, reps=reps,
                          ok=int(sum(o.branch == capi.TRACK_OK for o in out)), same_as_cpu=bool(same),
                          passes=[int(out[0].iters_first), int(out[0].iters_ref)],
                          ms_median=round(float(np.median(ms)), 4), ms_p10=round(float(ms[len(ms) // 10]), 4),
                          ms_p90=round(float(ms[(9 * len(ms)) // 10]), 4),
                          us_per_problem=round(float(np.median(ms)) * 1e3 / batch, 2),
                          cpu_ms_median=round(float(np.median(ms_cpu)), 4),
                          cpu_us_per_problem=round(float(np.median(ms_cpu)) * 1e3 / batch, 2))), flush=True)


def main() -> int:
    if len(sys.argv) >= 3 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
        return 0
    sizes = [int(a) for a in sys.argv[1:]] or [1, 8, 64]
    for model in (0, 1):
        for b in sizes:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(b), "200", str(model)],
                                   timeout=CHILD_LIMIT_S)
            except subprocess.TimeoutExpired:
                print(json.dumps(dict(batch=b, error=f"time limit of {CHILD_LIMIT_S} s")), flush=True)
                return 1
            if r.returncode != 0:   # nothing more is started on the device after a failure
                print(json.dumps(dict(batch=b, error=f"exit status {r.returncode}")), flush=True)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
