"""Endpoint-line local BA (plba_hlm_lba, variant PLBA_HLM_LBA_ENDPOINTS) timed per linearisation
beside the GBA variant on the same synthetic window, in one process, interleaved.

usage (GPU box): python tools/lba_endpoints_timing.py [--config C3] [--repeats 30] [--max-iters 6]
                                                      [--gba-lib PATH]
--gba-lib: a second libplba.so (e.g. built from the parent commit) that runs the GBA leg, so the
comparison is against code that predates the variant; default: the same library.
Prints one JSON line: medians and quartiles of solve_ms / linearizations over the repeats."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pl-slam-plucker_amd"))

import numpy as np  # noqa: E402

from plba import capi, lib, synth  # noqa: E402
from plba.hlm import gba_window, lba_window  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C3")
ap.add_argument("--repeats", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--max-iters", type=int, default=6)
ap.add_argument("--gba-lib", default=None)
a = ap.parse_args()


def solver_from(path):
    lib._lib = None                      # one library handle per Solver (lib.load caches the last one)
    lib.load(path)
    return lib.Solver()


g = synth.generate(a.config)
legs = {"gba": (solver_from(a.gba_lib), gba_window(g), capi.gba_params(max_iters=a.max_iters)),
        "lba_endpoints": (solver_from(None), lba_window(g), capi.lba_params(max_iters=a.max_iters))}
per_lin = {k: [] for k in legs}
info = {}
for k, (s, win, p) in legs.items():
    s.upload(win.graph)
    st = s.structure_stats()
    info[k] = dict(nf=int(st["nf"]), bw=int(st["bw"]), column_lane=int(st["column_lane"]), twisted=int(st["twisted"]))
for it in range(a.warmup + a.repeats):
    for k, (s, win, p) in legs.items():   # interleaved: drift hits both legs alike
        out = s.hlm_lba(win, p, with_trace=False)
        info[k]["linearizations"] = out["linearizations"]
        if it >= a.warmup:
            per_lin[k].append(out["solve_ms"] / max(out["linearizations"], 1))
res = {"config": a.config, "repeats": a.repeats, "max_iters": a.max_iters, "gba_lib": a.gba_lib or "same"}
for k, v in per_lin.items():
    q1, med, q3 = np.percentile(v, [25, 50, 75])
    res[k] = dict(info[k], ms_per_linearization_median=float(med), q1=float(q1), q3=float(q3), min=float(min(v)),
                  max=float(max(v)))
res["lba_over_gba"] = res["lba_endpoints"]["ms_per_linearization_median"] / res["gba"]["ms_per_linearization_median"]
print(json.dumps(res), flush=True)
for s, _, _ in legs.values():
    s.close()
