"""GPU box: wall time per call of plba_grid_match (upload, the launches, read-back, synchronise) on a
local-mapping-sized association in a single call: 3,000 visible map points against 600 unmatched point
features plus 600 map lines against 150 line features, 64 x 48 grid, ws = 3 (matching_f2f_ws), the
left/right check on; next to the single-threaded C++ restatement of the host mirror
(plslam_grid_match_cpu) on the same batch in the same process.

The parent starts one child process under a time limit; the child warms the shape up, then times
`reps` calls with the host clock around the call (it ends in a stream synchronise), checks the device
result against the CPU one, and prints one JSON line. Recorded, not gated."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pl-slam-plucker_amd"))

SHAPE = dict(map_pt=3000, feat_pt=600, map_ln=600, feat_ln=150, ws=3)
CHILD_LIMIT_S = 240
COLS, ROWS, WIDTH, HEIGHT = 64, 48, 1241.0, 376.0   # a KITTI image over the reference's grid


def problems(seed: int = 0):
    """The features of the new keyframe at pixel positions (train side); the visible map landmarks
    (query side): every feature is seen by one landmark within 3 pixels with about 2 flipped bits, the
    other landmarks project anywhere in the image with random descriptors."""
    import numpy as np

    from plba.slam_map import line_cells
    rng = np.random.default_rng(seed)
    iw, ih = COLS / WIDTH, ROWS / HEIGHT
    out = []
    for kind, n1, n2 in ((0, SHAPE["map_pt"], SHAPE["feat_pt"]), (1, SHAPE["map_ln"], SHAPE["feat_ln"])):
        d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
        mid2 = rng.uniform([0, 0], [WIDTH, HEIGHT], (n2, 2))
        half2 = rng.uniform(10, 120, (n2, 1)) * np.stack([np.cos(a := rng.uniform(0, np.pi, n2)), np.sin(a)], axis=1)
        d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
        mid1 = rng.uniform([0, 0], [WIDTH, HEIGHT], (n1, 2))
        half1 = rng.uniform(10, 120, (n1, 1)) * np.stack([np.cos(a := rng.uniform(0, np.pi, n1)), np.sin(a)], axis=1)
        rows = rng.permutation(n1)[:n2]
        flips = ((rng.integers(0, 16, (n2, 32)) == 0) * (1 << rng.integers(0, 8, (n2, 32)))).astype(np.uint8)
        d1[rows] = d2 ^ flips
        mid1[rows] = mid2 + rng.uniform(-3, 3, (n2, 2))
        half1[rows] = half2
        scale = np.array([iw, ih])
        if kind == 0:
            cells2 = [np.array([c], np.int32) for c in (mid2 * scale).astype(np.int32)]
            pb = dict(cell1=(mid1 * scale).astype(np.int32), cell1_end=None, cells2=cells2, dir2=None)
        else:
            s2, e2 = (mid2 - half2) * scale, (mid2 + half2) * scale
            v = e2 - s2
            pb = dict(cell1=((mid1 - half1) * scale).astype(np.int32), cell1_end=((mid1 + half1) * scale).astype(np.int32),
                      cells2=[line_cells(*s, *e) for s, e in zip(s2, e2)], dir2=v / np.linalg.norm(v, axis=1, keepdims=True))
        out.append(dict(pb, kind=kind, ws=SHAPE["ws"], nnr=0.9, line_sim_th=0.75, desc1=d1, desc2=d2))
    return out


def child(reps: int) -> None:
    import ctypes as C

    import numpy as np

    from plba import capi
    from plba.lib import Solver
    from plba.slam_map import load_host
    bv = capi.GridMatchBatchView(problems(), COLS, ROWS, True)
    ip = C.POINTER(C.c_int32)
    m12, cnt = np.zeros(int(bv.off1[-1]), np.int32), np.zeros(2, np.int32)
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
        assert H.plslam_grid_match_cpu(None, C.byref(bv.struct), m12_cpu.ctypes.data_as(ip), cnt_cpu.ctypes.data_as(ip)) == 0
    cpu_call()
    cpu_ms = timed(cpu_call, 20)
    with Solver() as s:
        def call():
            rc = s.L.plba_grid_match(s.ctx, C.byref(bv.struct), m12.ctypes.data_as(ip), cnt.ctypes.data_as(ip))
            assert rc == 0, rc
        for _ in range(5):   # code object, device block and pinned image
            call()
        ms = timed(call, reps)
    assert np.array_equal(m12, m12_cpu) and np.array_equal(cnt, cnt_cpu)
    print(json.dumps(dict(SHAPE, reps=reps, pt_matches=int(cnt[0]), ln_matches=int(cnt[1]),
                          train_cells=int(bv.cell_off2[-1]), ms_median=round(float(np.median(ms)), 4),
                          ms_p10=round(float(ms[len(ms) // 10]), 4), ms_p90=round(float(ms[(9 * len(ms)) // 10]), 4),
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
