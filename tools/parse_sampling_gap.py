"""device idle time around the contrastive sampling of a step, from a rocprofv3 --kernel-trace CSV of bench.py:
    python tools/parse_sampling_gap.py <kernel_trace.csv> <timed_steps> [out.json]
Per InfoNCE forward launch (one per semi-supervised step; the LAST <timed_steps> are bench.py's timed ones):
  before_us   end of the last phase-1 / bank-append kernel -> start of the InfoNCE forward with every kernel that ran in
              between taken out (host path: mirror, index draws, upload, grouping, job table; device path: the plan launch)
  after_us    end of the InfoNCE forward -> start of the next kernel of any stream (autograd start-up + backward launch)
  idle_us     time in [end of phase 1 / append, start of the first kernel of >= LONG_US after the InfoNCE forward] during
              which NO kernel ran on any stream: the loss heads' backward launches included
gap_us = before_us + after_us: the window of the two events less the InfoNCE forward's own duration."""
import csv
import json
import statistics
import sys

PRE = ("k_bank_append", "k_bank_enqueue", "k_bank_advance", "k_phase1_tail", "k_proto_stream", "k_contra_classify")
LONG_US = 200.0


def _idle(rows, t0, t1):
    """ns of [t0, t1] covered by no kernel"""
    cur, idle = t0, 0
    for s, e, _ in rows:
        if e <= t0 or s >= t1:
            continue
        if s > cur:
            idle += s - cur
        cur = max(cur, e)
    return idle + max(0, t1 - cur)


def main(trace, steps, out=None):
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(trace)))
    recs = []
    for k, (s, e, name) in enumerate(rows):
        if "k_infonce" not in name or "reduce" in name:
            continue
        pre = [r for r in rows[max(0, k - 40):k] if r[2].startswith(PRE) or any(p in r[2] for p in PRE)]
        if not pre:
            continue
        p_end = max(r[1] for r in pre)
        between = [r for r in rows[max(0, k - 40):k] if r[0] >= p_end]
        nxt = next((r for r in rows[k + 1:] if r[0] >= e), None)
        lng = next((r for r in rows[k + 1:] if r[0] >= e and (r[1] - r[0]) >= LONG_US * 1e3), None)
        if nxt is None or lng is None:
            continue
        before = (s - p_end) - sum(r[1] - r[0] for r in between)
        recs.append(dict(before_us=before / 1e3, infonce_us=(e - s) / 1e3, after_us=(nxt[0] - e) / 1e3,
                         gap_us=(before + nxt[0] - e) / 1e3, idle_us=_idle(rows, p_end, lng[0]) / 1e3,
                         window_us=(lng[0] - p_end) / 1e3, kernels_between=[r[2].split("(")[0] for r in between],
                         next_kernel=nxt[2].split("(")[0], first_long_kernel=lng[2].split("(")[0]))
    timed = recs[-int(steps):]
    med = lambda key: statistics.median(r[key] for r in timed) if timed else None
    res = dict(infonce_launches_in_trace=len(recs), timed_steps=len(timed), long_us=LONG_US,
               median=dict((k, med(k)) for k in ("before_us", "infonce_us", "after_us", "gap_us", "idle_us", "window_us")),
               steps=timed)
    print(json.dumps(res["median"]))
    if out:
        json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main(*sys.argv[1:])
