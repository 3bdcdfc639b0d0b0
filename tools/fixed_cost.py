"""Fixed per-solve cost of the benchmark's LBA loop from a rocprofv3 kernel trace: everything one
`reset -> plba_lba_plucker` puts on the stream outside its working step graphs.

For every solve of the trace with the usual number of steps (the first five, warm-up, dropped):
  span      first reset operation .. last operation of the solve (k_refresh, or the control / trace
            copies where they follow it)
  steps     first kernel of the first step .. last kernel of the last working step
  fixed     span - steps, split into reset | prologue (control upload, k_line_pluker, up to the first
            step kernel) | trailing no-op steps | epilogue (after the last step kernel: refresh,
            copies and the idle gaps between them)
  between   last operation of a solve .. first reset operation of the next (host: the final wait
            returning, the caller's loop)
Medians over the solves, in microseconds. Copies that the runtime does with its DMA engines are not
kernels and show only as gaps.
usage: python tools/fixed_cost.py <kernel_trace.csv> [--dump N]   (--dump: list the operations of N solves)"""
import collections
import csv
import statistics as st
import sys

STEP = ("k_linearize", "k_iter_reduce", "k_iter_init", "k_edge_schur", "k_rcs_", "k_pose_update", "k_lm_solve",
        "k_decide", "k_dense_")
BLIT = ("__amd_rocclr_fillBuffer", "__amd_rocclr_copyBuffer")
NOOP_KERNEL_US = 8.0  # no kernel of a step above this: every one of them left at its guard


def short(n):
    return n.split("(")[0].replace("void ", "").replace("plba::", "").split("<")[0]


def main():
    rows = [(int(r["Start_Timestamp"]) / 1e3, int(r["End_Timestamp"]) / 1e3, short(r["Kernel_Name"]))
            for r in csv.DictReader(open(sys.argv[1]))]
    rows.sort()
    dump = int(sys.argv[sys.argv.index("--dump") + 1]) if "--dump" in sys.argv else 0
    names = [r[2] for r in rows]
    one_kernel = "k_reset_estimates" in names
    is_step = lambda n: n.startswith(STEP)
    is_blit = lambda n: n.startswith(BLIT)
    # a solve starts at its reset: the reset kernel, or the run of blits that ends at k_line_pluker
    starts = []
    for p, n in enumerate(names):
        if n != "k_line_pluker":
            continue
        q = p
        if one_kernel:
            while q > 0 and names[q] != "k_reset_estimates" and not is_step(names[q - 1]) and p - q < 4:
                q -= 1
            if names[q] != "k_reset_estimates":
                continue
        else:
            while q > 0 and is_blit(names[q - 1]):
                q -= 1
        starts.append((q, p))
    solves = []
    for (q, p), nxt in zip(starts, starts[1:] + [(len(rows), None)]):
        ops = rows[q:nxt[0]]
        # the solve's own operations end with the refresh and the copies right behind it
        last = max((i for i, o in enumerate(ops) if o[2] == "k_refresh"), default=None)
        if last is None:
            continue
        if one_kernel:
            while last + 1 < len(ops) and is_blit(ops[last + 1][2]):
                last += 1
        solves.append((ops[:last + 1], p - q, rows[nxt[0]][0] if nxt[1] is not None else None))
    if not solves:
        sys.exit("no solve found in the trace")

    def split(ops, pl):
        first = next(i for i, o in enumerate(ops) if is_step(o[2]))
        lasts = max(i for i, o in enumerate(ops) if is_step(o[2]))
        steps, cur = [], []
        for o in ops[first:lasts + 1]:
            if o[2] == "k_linearize" and cur:
                steps.append(cur)
                cur = []
            cur.append(o)
        steps.append(cur)
        work = [s for s in steps if max(o[1] - o[0] for o in s) >= NOOP_KERNEL_US]
        # reset = the operations before the prologue (parent: the blit just before k_line_pluker is the
        # control upload when the runtime did it with a kernel)
        n_reset = pl if one_kernel else pl - (1 if pl >= 1 and ops[pl - 1][2].startswith(BLIT[1]) and
                                              pl >= 2 and ops[pl - 2][2].startswith(BLIT[0]) else 0)
        n_reset = max(n_reset if not one_kernel else 1, 1)
        tail = ops[lasts + 1:]
        d = collections.OrderedDict()
        d["span"] = ops[-1][1] - ops[0][0]
        d["steps"] = work[-1][-1][1] - ops[first][0]
        d["reset"] = ops[n_reset - 1][1] - ops[0][0]
        d["prologue"] = ops[first][0] - ops[n_reset - 1][1]
        d["noop_steps"] = ops[lasts][1] - work[-1][-1][1]
        d["epilogue"] = ops[-1][1] - ops[lasts][1]
        d["epilogue_busy"] = sum(o[1] - o[0] for o in tail)
        d["epilogue_idle"] = d["epilogue"] - d["epilogue_busy"]
        d["fixed"] = d["span"] - d["steps"]
        cnt = collections.Counter("fill" if o[2].startswith(BLIT[0]) else "copy" if o[2].startswith(BLIT[1]) else o[2]
                                  for o in ops if not is_step(o[2]))
        return d, len(steps), len(work), cnt

    parsed = [(split(ops, pl), ops, nxt) for ops, pl, nxt in solves]
    modal = collections.Counter(p[0][1] for p in parsed).most_common(1)[0][0]
    keep = [p for p in parsed if p[0][1] == modal][5:]
    if not keep:
        sys.exit("fewer than six solves of %d steps in the trace" % modal)
    for (d, ns, nw, cnt), ops, nxt in keep[:dump]:
        print("--- solve: %d steps, %d working" % (ns, nw))
        t0 = ops[0][0]
        for o in ops:
            if not is_step(o[2]) or o[2] == "k_linearize":
                print("  %10.2f %8.2f  %s" % (o[0] - t0, o[1] - o[0], o[2]))
    if dump:
        return
    (d0, ns, nw, cnt0), _, _ = keep[0]
    print("solves analysed %d (of %d in the trace), %d steps each, %d working" % (len(keep), len(parsed), ns, nw))
    print("operations outside the step graphs, per solve: " + ", ".join("%s %d" % kv for kv in sorted(cnt0.items())))
    med = lambda k: st.median(p[0][0][k] for p in keep)
    for k in d0:
        print("%-14s %9.2f us" % (k, med(k)))
    btw = [nxt - ops[-1][1] for _, ops, nxt in keep if nxt is not None]
    per = [nxt - ops[0][0] for _, ops, nxt in keep if nxt is not None]
    print("%-14s %9.2f us" % ("between", st.median(btw)))
    print("%-14s %9.2f us" % ("period", st.median(per)))
    print("fixed / span  %6.2f %%   (fixed + between) / period  %6.2f %%"
          % (100 * med("fixed") / med("span"), 100 * (med("fixed") + st.median(btw)) / st.median(per)))


if __name__ == "__main__":
    main()
