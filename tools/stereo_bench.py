"""GPU box: wall time per call of plba_stereo_associate (packing, upload, the launches, read-back,
synchronise, the copy to the caller's arrays) on a realistic frame, about 1000 + 1000 keypoints and
200 + 200 segments of a 1241 x 376 image, and on a batch of 8 such frames; next to the single-threaded
C++ restatement of the host mirror (plslam_stereo_cpu) on the same batch in the same process.

The parent starts one child process under a time limit; the child warms each shape up, then times
`reps` calls with the host clock around the call (it ends in a stream synchronise), checks the device
result against the CPU one byte for byte, and prints one JSON line per shape. Recorded, not gated."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pl-slam-plucker_amd"))

SHAPE = dict(pt_l=1000, pt_r=1000, ls_l=200, ls_r=200)
CHILD_LIMIT_S = 240
CAMERA = dict(width=1241, height=376, fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, b=0.537, pluker=1)


def frame(seed: int):
    """Nine tenths of the left features have a partner on the right: a disparity of 2 to 80 px, half a pixel
    of vertical noise, a few flipped descriptor bits; the rest of both sides is random."""
    import numpy as np
    rng = np.random.default_rng(seed)
    W, H = CAMERA["width"], CAMERA["height"]

    def flip(d):
        bits = np.unpackbits(d, axis=1)
        for row in bits:
            row[rng.permutation(256)[:int(rng.integers(1, 6))]] ^= 1
        return np.packbits(bits, axis=1)
    n, k = SHAPE["pt_l"], int(0.9 * min(SHAPE["pt_l"], SHAPE["pt_r"]))
    pl = np.stack([rng.uniform(90, W - 5, n), rng.uniform(5, H - 5, n)], axis=1)
    dl = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pr = np.stack([rng.uniform(0, W, SHAPE["pt_r"]), rng.uniform(0, H, SHAPE["pt_r"])], axis=1)
    dr = rng.integers(0, 256, (SHAPE["pt_r"], 32), dtype=np.uint8)
    pr[:k] = pl[:k] - np.stack([rng.uniform(2, 80, k), rng.uniform(-0.5, 0.5, k)], axis=1)
    dr[:k] = flip(dl[:k])
    n, k = SHAPE["ls_l"], int(0.9 * min(SHAPE["ls_l"], SHAPE["ls_r"]))

    def segs(m):
        s = np.stack([rng.uniform(90, W - 5, m), rng.uniform(5, H - 5, m)], axis=1)
        ang, length = rng.uniform(0.3, np.pi - 0.3, m) * rng.choice([-1, 1], m), rng.uniform(30, 200, m)
        e = s + length[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        return np.concatenate([s, np.clip(e, [0, 0], [W, H])], axis=1)
    ll, lr = segs(n), segs(SHAPE["ls_r"])
    ldl, ldr = rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 256, (SHAPE["ls_r"], 32), dtype=np.uint8)
    d = rng.uniform(2, 60, k)
    lr[:k] = ll[:k] - np.stack([d, np.zeros(k), d * rng.uniform(0.85, 1.15, k), np.zeros(k)], axis=1)
    ldr[:k] = flip(ldl[:k])
    p, q = rng.permutation(SHAPE["pt_r"]), rng.permutation(SHAPE["ls_r"])
    return dict(pt_l=pl.astype(np.float32), pdesc_l=dl, pt_r=pr[p].astype(np.float32), pdesc_r=dr[p],
                ls_l=ll.astype(np.float32), ldesc_l=ldl, ls_r=lr[q].astype(np.float32), ldesc_r=ldr[q])


def child(reps: int) -> None:
    import ctypes as C

    import numpy as np

    from plba import capi
    from plba.lib import Solver
    from plba.slam_map import load_host
    H = load_host()
    prm = capi.stereo_params(CAMERA)

    def timed(fn, n):
        ms = []
        for _ in range(n):
            t = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t) * 1e3)
        return np.sort(ms)

    with Solver() as s:
        for frames in (1, 8):
            fs = [frame(seed) for seed in range(frames)]
            dev, cpu = capi.StereoBatchView(fs), capi.StereoBatchView(fs)

            def cpu_call():
                assert H.plslam_stereo_cpu(None, C.byref(cpu.struct), C.byref(prm), C.byref(cpu.out)) == 0

            def call():
                rc = s.L.plba_stereo_associate(s.ctx, C.byref(dev.struct), C.byref(prm), C.byref(dev.out))
                assert rc == 0, rc
            cpu_call()
            cpu_ms = timed(cpu_call, 10)
            for _ in range(5):   # code object, device block and pinned image
                call()
            ms = timed(call, reps)
            a, b = dev.results(True), cpu.results(True)
            assert all(x[k].tobytes() == y[k].tobytes() if hasattr(x[k], "tobytes") else x[k] == y[k]
                       for x, y in zip(a, b) for k in x)
            print(json.dumps(dict(SHAPE, frames=frames, reps=reps, n_pt=[r["n_pt"] for r in a], n_ls=[r["n_ls"] for r in a],
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
