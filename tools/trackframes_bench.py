"""GPU box: wall time per call of plba_track_frames (one upload, the matcher, the gather, the pose, the
scatter, one read-back, one synchronise) at (300 points, 100 lines) matched per frame pair, among 60 / 20
unmatched rows on each side, for batches of 1, 8 and 64 pairs, against
  - the two-call path on the same context: plba_desc_match, the gather of the matched rows on the host
    (numpy), plba_track_pose; and the two device calls alone on rows gathered beforehand, the floor of
    that path for a caller whose gather costs nothing;
  - the single-threaded C++ restatement plslam_track_frames_cpu,
on the same batch in the same process.

The parent starts one child process per batch size, each under its own time limit, and stops at the first
one that fails; a child warms the shape up, then times `reps` calls with the host clock around the whole
call and prints one JSON line. Recorded, not gated."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pl-slam-plucker_amd"))

SHAPE = (300, 100)
EXTRA = (60, 60, 20, 20)
CHILD_LIMIT_S = 180


def child(batch: int, reps: int, model: int) -> None:
    import ctypes as C

    import numpy as np

    from plba import capi, trackframes, trackpose
    from plba.lib import Solver
    from plba.slam_map import load_host
    pairs = [trackframes.from_problem(trackpose.synth(SHAPE[0], SHAPE[1], seed=100 + i, outlier_frac=0.2), seed=i, extra=EXTRA)
             for i in range(batch)]
    p = capi.frames_params(capi.track_params(line_model=model))
    bv, bv_cpu = capi.FramesBatchView(pairs), capi.FramesBatchView(pairs)
    # the two-call path's own inputs: the descriptor sets of every pair and kind, as plba_desc_match takes them
    sets = [s for q in pairs for s in ((q.prev_pdesc, q.cur_pdesc), (q.prev_ldesc, q.cur_ldesc))]
    mv = capi.MatchBatchView(sets, [p.nnr_pt, p.nnr_ln] * batch, True, 32)
    m12 = np.full(int(mv.off1[-1]), -1, np.int32)
    cnt = np.zeros(2 * batch, np.int32)
    ip, bp = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    out2 = (capi.PlbaTrackOut * batch)()
    H = load_host()

    def timed(fn, n):
        ms = []
        for _ in range(n):
            t = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t) * 1e3)
        return np.sort(ms)

    with Solver() as s:
        def one_call():
            rc = s.L.plba_track_frames(s.ctx, C.byref(bv.struct), C.byref(p), C.byref(bv.out_struct))
            assert rc == 0, rc

        def two_calls():
            rc = s.L.plba_desc_match(s.ctx, C.byref(mv.struct), m12.ctypes.data_as(ip), cnt.ctypes.data_as(ip))
            assert rc == 0, rc
            probs = [trackframes.gather(q, m12[mv.off1[2 * k]:mv.off1[2 * k + 1]], m12[mv.off1[2 * k + 1]:mv.off1[2 * k + 2]])
                     for k, q in enumerate(pairs)]
            tv = capi.TrackBatchView(probs)
            pin, lin = np.zeros(int(tv.pt_off[-1]) + 1, np.uint8), np.zeros(int(tv.ln_off[-1]) + 1, np.uint8)
            rc = s.L.plba_track_pose(s.ctx, C.byref(tv.struct), C.byref(p.track), out2, pin.ctypes.data_as(bp),
                                     lin.ctypes.data_as(bp))
            assert rc == 0, rc

        def two_calls_no_gather():
            """the two device calls alone, on rows gathered beforehand: what a caller with a free gather would pay"""
            rc = s.L.plba_desc_match(s.ctx, C.byref(mv.struct), m12.ctypes.data_as(ip), cnt.ctypes.data_as(ip))
            assert rc == 0, rc
            rc = s.L.plba_track_pose(s.ctx, C.byref(tv0.struct), C.byref(p.track), out2, None, None)
            assert rc == 0, rc

        def cpu():
            assert H.plslam_track_frames_cpu(None, C.byref(bv_cpu.struct), C.byref(p), C.byref(bv_cpu.out_struct)) == 0
        for _ in range(5):   # code objects, device blocks and pinned images
            one_call()
            two_calls()
        tv0 = capi.TrackBatchView([trackframes.gather(q, m12[mv.off1[2 * k]:mv.off1[2 * k + 1]],
                                                      m12[mv.off1[2 * k + 1]:mv.off1[2 * k + 2]]) for k, q in enumerate(pairs)])
        ms1 = timed(one_call, reps)
        ms2 = timed(two_calls, reps)
        ms3 = timed(two_calls_no_gather, reps)
        cpu()
        ms_cpu = timed(cpu, max(3, reps // 20))
    same = all(bytes(bv.out[i]) == bytes(out2[i]) for i in range(batch))
    same_cpu = bool(np.array_equal(bv.pt_m12, bv_cpu.pt_m12) and np.array_equal(bv.ln_m12, bv_cpu.ln_m12) and
                    all(bv.out[i].branch == bv_cpu.out[i].branch and bv.out[i].n_inl_pt == bv_cpu.out[i].n_inl_pt
                        for i in range(batch)))
    med = lambda ms: round(float(np.median(ms)), 4)
    print(json.dumps(dict(batch=batch, n_pt=SHAPE[0], n_ln=SHAPE[1], extra=EXTRA, line_model=model, reps=reps,
                          matched=[int(bv.n_pt[0]), int(bv.n_ln[0])], ok=int(sum(o.branch == capi.TRACK_OK for o in bv.out)),
                          bitwise_same_as_two_calls=bool(same), same_as_cpu=same_cpu,
                          one_call_ms_median=med(ms1), one_call_ms_p10=round(float(ms1[len(ms1) // 10]), 4),
                          one_call_ms_p90=round(float(ms1[(9 * len(ms1)) // 10]), 4),
                          two_calls_ms_median=med(ms2), two_calls_ms_p10=round(float(ms2[len(ms2) // 10]), 4),
                          two_calls_ms_p90=round(float(ms2[(9 * len(ms2)) // 10]), 4),
                          two_calls_no_gather_ms_median=med(ms3), cpu_ms_median=med(ms_cpu),
                          one_call_us_per_pair=round(float(np.median(ms1)) * 1e3 / batch, 2))), flush=True)


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
