"""GPU box: wall time of the map-to-keyframe association on a local map of the C3 scale (about 20000 candidate
points and 4000 candidate lines, a third of them invisible, against 300 unmatched point and 80 unmatched line
features), for 1 keyframe and for a batch of 8, three paths beside each other in one process:

  (a) plslam_match_map_to_kf with the device matchers: the host projection and cells, plba_grid_match, the
      fallback decided on the host, plba_desc_match where it runs. One keyframe per call: 8 keyframes are 8 calls.
  (b) plslam_match_map_to_kf_assoc: the gather and one plba_map_associate call. 8 keyframes are 8 calls.
  (c) plslam_map_assoc_cpu, single-threaded, on the batch that (d) takes.
  (d) plba_map_associate itself on the packed batch of 1 and of 8 keyframes (no map, no gather).

(a) and (b) change the map, so every repetition runs on a fresh host map built outside the clock; what is
timed is the call. The parent starts one child process under a time limit; the child checks (d) against (c)
byte for byte and (a) against (b) in their statistics, and prints one JSON line per shape. Recorded, not gated."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pl-slam-plucker_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPE = dict(pt=(20000, 300), ls=(4000, 80))
CHILD_LIMIT_S = 420


def host_map(kf):
    """A host map whose local landmarks are the keyframe's candidates and whose keyframe 1 has its features."""
    import numpy as np

    import mapassoc_cases as MC
    from plba.slam_map import KF, HostMap, Landmark, SlamMap
    T = np.asarray(kf["T_kf_w"], np.float64).reshape(4, 4)
    kfs = [KF(0, np.eye(4), True, [], []), KF(1, T, True, [-1] * len(kf["pt_pl"]), [-1] * len(kf["ls_spl"]))]

    def lm(idx, pos, width, desc):
        return Landmark(idx=idx, local=True, inlier=True, pos=np.array(pos, np.float64), desc_list=[desc], obs_list=[np.zeros(width)],
                        kf_obs_list=[0], sigma_list=[1.0], dir_list=[np.array([0.0, 0.0, 1.0])] if width == 2 else None)
    X = np.nan_to_num(np.asarray(kf["pt_X"]), nan=1e9)   # the mirror's setters take finite landmarks: far away is invisible too
    L3 = np.nan_to_num(np.asarray(kf["ls_X"]), nan=1e9)
    pts = [lm(i, X[i], 2, kf["pdesc_m"][i]) for i in range(len(X))]
    lns = [lm(i, np.zeros(6), 4, kf["ldesc_m"][i]) for i in range(len(L3))]
    for x in pts + lns:
        x.med_desc = x.desc_list[0]
    m = SlamMap(MC.CAMERA["fx"], MC.CAMERA["fy"], MC.CAMERA["cx"], MC.CAMERA["cy"], keyframes=kfs, points=pts, lines=lns,
                map_points_kf_idx={}, full_graph=np.zeros((2, 2), np.uint32), max_kf_idx=1)
    h = HostMap(m)
    for i, L in enumerate(L3):
        h.set_line_geometry(i, L, np.zeros(3))
    h.set_keyframe_features(1, kf["pdesc_f"], kf["pt_P"], kf["pt_pl"], kf["ldesc_f"], kf["ls_sP"], kf["ls_eP"], kf["ls_le"])
    h.set_keyframe_line_endpoints(1, kf["ls_spl"], kf["ls_epl"])
    h.set_camera(MC.CAMERA["fx"], MC.CAMERA["fy"], MC.CAMERA["cx"], MC.CAMERA["cy"], MC.WIDTH, MC.HEIGHT)
    return h


def child(reps: int) -> None:
    import ctypes as C

    import numpy as np

    import mapassoc_cases as MC
    from plba import capi
    from plba.lib import Solver
    from plba.slam_map import load_host, mapmatch_params
    H = load_host()
    prm = capi.mapassoc_params(MC.CAMERA)

    def med(ms):
        ms = np.sort(ms)
        return dict(median=round(float(np.median(ms)), 4), p10=round(float(ms[len(ms) // 10]), 4),
                    p90=round(float(ms[(9 * len(ms)) // 10]), 4), reps=len(ms))

    def timed(fn, n):
        ms = []
        for _ in range(n):
            t = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t) * 1e3)
        return ms

    with Solver() as s:
        for n_kf in (1, 8):
            kfs = [MC.keyframe(200 + seed, SHAPE["pt"], SHAPE["ls"]) for seed in range(n_kf)]
            dev, cpu = capi.MapassocBatchView(kfs), capi.MapassocBatchView(kfs)

            def cpu_call():
                assert H.plslam_map_assoc_cpu(None, C.byref(cpu.struct), C.byref(prm), C.byref(cpu.out)) == 0

            def call():
                rc = s.L.plba_map_associate(s.ctx, C.byref(dev.struct), C.byref(prm), C.byref(dev.out))
                assert rc == 0, rc
            cpu_call()
            cpu_ms = timed(cpu_call, 3)
            for _ in range(5):   # code object, device block and pinned image
                call()
            dev_ms = timed(call, reps)
            assert all(dev.o[k].tobytes() == cpu.o[k].tobytes() for k in dev.o)
            # the two mirror paths: every repetition on fresh maps, the n_kf calls of a repetition timed together
            n_map = max(3, min(reps, 10))
            legacy_ms, assoc_ms, stats = [], [], None
            for r in range(n_map + 1):   # the first repetition warms both paths up
                hs_a, hs_b = [host_map(k) for k in kfs], [host_map(k) for k in kfs]
                t = time.perf_counter()
                sa = [h.match_map_to_kf(1, None, mapmatch_params()) for h in hs_a]
                ta = (time.perf_counter() - t) * 1e3
                t = time.perf_counter()
                sb = [h.match_map_to_kf_assoc(1, None, prm) for h in hs_b]
                tb = (time.perf_counter() - t) * 1e3
                for a, b in zip(sa, sb):
                    a.pop("match_ms"), b.pop("match_ms")
                assert sa == sb, (sa, sb)
                stats = sb
                for h in hs_a + hs_b:
                    h.close()
                if r:
                    legacy_ms.append(ta), assoc_ms.append(tb)
            res = dev.results()
            print(json.dumps(dict(points=SHAPE["pt"], lines=SHAPE["ls"], keyframes=n_kf,
                                  n_visible=[r["n_visible"] for r in res], n_matches=[r["n_matches"] for r in res],
                                  fallback=[r["fallback"] for r in res], accepted=[x["accepted"] for x in stats],
                                  a_match_map_to_kf_ms=med(legacy_ms), b_match_map_to_kf_assoc_ms=med(assoc_ms),
                                  c_map_assoc_cpu_1thread_ms=med(cpu_ms), d_plba_map_associate_ms=med(dev_ms),
                                  device_equal_to_cpu=True, paths_a_b_same_stats=True)), flush=True)


def main() -> int:
    if len(sys.argv) >= 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]) if len(sys.argv) > 2 else 50)
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
