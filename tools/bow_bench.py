"""GPU box: wall time per plba_bow_insert (upload, three launches, read-back, synchronise) for a
keyframe of 600 point descriptors (slot 0) and 150 line descriptors (slot 1) against a synthetic
k = 10, L = 5 vocabulary (111,111 nodes), at database sizes 100, 1,000 and 4,000; next to the
single-threaded C++ restatement of the host mirror (plslam_bow_cpu) on the same input in the same
process, the results checked equal as bytes.

The parent starts one child process per database size, each under its own time limit, and stops at
the first one that fails; a child fills both databases, then times `reps` inserts with the host
clock around the call (it ends in a stream synchronise) and prints one JSON line. The database
grows by one vector per timed insert (reps is small against its size). Recorded, not gated. The
baseline is this project's own restatement, not DBoW2: it walks sorted arrays where DBoW2 walks
std::maps."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pl-slam-plucker_amd"))

SHAPE = (600, 150)
K, LEVELS = 10, 5
CHILD_LIMIT_S = 400


def vocabulary(seed: int):
    """A full k-ary tree, breadth first, random 32-byte node descriptors, idf-like leaf weights."""
    import numpy as np
    rng = np.random.default_rng(seed)
    counts = [K ** lv for lv in range(LEVELS + 1)]
    n = sum(counts)
    first = np.cumsum([0] + counts)           # first node of each level
    n_inner = int(first[LEVELS])
    child_off = np.zeros(n + 1, np.int32)
    child_off[1:n_inner + 1] = K * np.arange(1, n_inner + 1)
    child_off[n_inner + 1:] = K * n_inner
    children = np.arange(1, n, dtype=np.int32)   # node i's children are K*i+1 .. K*i+K
    word_id = np.full(n, -1, np.int32)
    word_id[n_inner:] = np.arange(n - n_inner, dtype=np.int32)
    weight = np.zeros(n)
    weight[n_inner:] = rng.uniform(0.5, 8.0, n - n_inner)
    return dict(child_off=child_off, children=children, node_desc=rng.integers(0, 256, (n, 32), dtype=np.uint8),
                word_id=word_id, weight=weight, n_words=n - n_inner, desc_bytes=32)


def child(n_db: int, reps: int) -> None:
    import numpy as np

    from plba.lib import Solver
    from plba.slam_map import BowCpu
    rng = np.random.default_rng(n_db)
    vocs = [vocabulary(1), vocabulary(2)]
    total = n_db + reps + 5
    desc = [[rng.integers(0, 256, (SHAPE[s], 32), dtype=np.uint8) for _ in range(min(total, 64))] for s in (0, 1)]
    cpu = BowCpu()
    with Solver() as g:
        for s in (0, 1):
            cpu.set_vocab(s, vocs[s])
            g.bow_set_vocab(s, vocs[s])
        ms = {"gpu": [], "cpu": []}
        for kf in range(total):
            t_gpu = t_cpu = 0.0
            for s in (0, 1):
                d = desc[s][kf % len(desc[s])]
                t = time.perf_counter()
                a = g.bow_insert(s, kf, d)
                t_gpu += time.perf_counter() - t
                t = time.perf_counter()
                b = cpu.insert(s, kf, d)
                t_cpu += time.perf_counter() - t
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (kf, s)
            if kf >= n_db + 5:   # the inserts past the fill and five warm-up calls at this size
                ms["gpu"].append(t_gpu * 1e3)
                ms["cpu"].append(t_cpu * 1e3)
    gm, cm = np.sort(ms["gpu"]), np.sort(ms["cpu"])
    print(json.dumps(dict(db_size=n_db, n_pt=SHAPE[0], n_ln=SHAPE[1], vocabulary=f"k={K} L={LEVELS}", reps=reps,
                          gpu_ms_median=round(float(np.median(gm)), 4), gpu_ms_p10=round(float(gm[len(gm) // 10]), 4),
                          gpu_ms_p90=round(float(gm[(9 * len(gm)) // 10]), 4),
                          cpu_1thread_ms_median=round(float(np.median(cm)), 4),
                          ratio_cpu_over_gpu=round(float(np.median(cm) / np.median(gm)), 2), equal_to_cpu=True)), flush=True)


def main() -> int:
    if len(sys.argv) >= 3 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 50)
        return 0
    sizes = [int(a) for a in sys.argv[1:]] or [100, 1000, 4000]
    for n_db in sizes:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n_db)], timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(db_size=n_db, error=f"time limit of {CHILD_LIMIT_S} s")), flush=True)
            return 1
        if r.returncode != 0:   # nothing more is started on the device after a failure
            print(json.dumps(dict(db_size=n_db, error=f"exit status {r.returncode}")), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
