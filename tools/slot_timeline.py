#!/usr/bin/env python3
"""How the pipeline slots' big kernels share the chip: a summary of a rocprofv3 kernel trace of bench.py.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py --gpus 1 --steps 60 --warmup 5
    python tools/slot_timeline.py DIR [--steps 60] [--cus 256] [--out summary.json]

(kernel trace only, no counters; DIR is searched for *kernel_trace.csv.)  A recurrence workgroup (lstm_rec*) and a workgroup of a
persistent grid (gemm_f16p_ws_kernel, head_fused_kernel) each hold a CU to themselves, so the grids tell how many CUs are held.  The
timed part is taken as the last 4 x steps recurrence launches (one per layer and step; nothing of the library runs after the timed
steps of a plain bench.py run).  Reported for it:
  dispatch_delay_us   per recurrence launch, its start minus the end of the previous kernel on its own stream (median, p90): a
                      recurrence that waits for another slot's persistent grid to drain shows a large fraction of a projection here
  rec_beside_other_proj_share   share of wall time in which a recurrence of one stream runs beside a projection of another
  recs_only_share     share of wall time in which two or more recurrences run and no projection does
  mean_cus_held       time average of the workgroups of the running recurrences and persistent grids (at most --cus)
  held_off            the start stamp of a kernel is its dispatch, not its first workgroup on a CU, so a recurrence that waits for CUs
                      shows as a longer launch: launches that start while another stream's projection runs against the others, the
                      slope of the launch duration over what that projection had left, and the same split for the projections
Streams are told apart by Stream_Id where the trace carries more than one, by Queue_Id otherwise."""
import argparse
import csv
import glob
import json
import os
import sys

LAYERS = 4


def kind_of(name):
    if "lstm_rec" in name:
        return "rec"
    if "gemm_f16p_ws_kernel" in name:
        return "proj"
    if "head_fused_kernel" in name:
        return "head"
    return "other"


def read_rows(path):
    """The library's kernels of one kernel_trace.csv: dicts of stream, kind, start, end (ns) and workgroups, by start time."""
    raw = list(csv.DictReader(open(path)))
    key = "Stream_Id" if len({r.get("Stream_Id") for r in raw}) > 1 else "Queue_Id"
    rows = []
    for r in raw:
        name = r["Kernel_Name"]
        if "uvad::" not in name:
            continue
        wgs = 1
        for ax in "XYZ":
            g, w = int(r.get(f"Grid_Size_{ax}") or 1), int(r.get(f"Workgroup_Size_{ax}") or 1)
            wgs *= max(1, g // max(w, 1))
        rows.append({"stream": r[key], "kind": kind_of(name), "name": name, "start": int(r["Start_Timestamp"]),
                     "end": int(r["End_Timestamp"]), "wgs": wgs})
    rows.sort(key=lambda r: r["start"])
    return rows, key


def quantile(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))] if xs else None


def summarize(rows, steps, cus):
    recs = [r for r in rows if r["kind"] == "rec"]
    if not recs:
        raise SystemExit("no recurrence launches in the trace")
    first = recs[-min(len(recs), LAYERS * steps)]
    t0, t1 = first["start"], max(r["end"] for r in rows)
    # dispatch delay: against the previous kernel of the same stream (whatever it is: a projection, the exact-kernel twin, ...)
    last_end, delays = {}, []
    for r in rows:
        if r["kind"] == "rec" and r["start"] >= t0 and r["stream"] in last_end:
            delays.append((r["start"] - last_end[r["stream"]]) / 1e3)
        last_end[r["stream"]] = max(r["end"], last_end.get(r["stream"], 0))
    # sweep over the starts and ends of the kernels that hold whole CUs
    ev = []
    for i, r in enumerate(rows):
        if r["kind"] != "other" and r["end"] > t0:
            ev.append((max(r["start"], t0), 1, i))
            ev.append((r["end"], 0, i))
    ev.sort()
    live = set()
    beside = recs_only = cu_ns = 0
    prev = t0
    for t, on, i in ev:
        dt = t - prev
        if dt > 0 and live:
            rs = {rows[j]["stream"] for j in live if rows[j]["kind"] == "rec"}
            ps = {rows[j]["stream"] for j in live if rows[j]["kind"] == "proj"}
            if any(a != b for a in rs for b in ps):
                beside += dt
            if not ps and sum(1 for j in live if rows[j]["kind"] == "rec") >= 2:
                recs_only += dt
            cu_ns += dt * min(cus, sum(rows[j]["wgs"] for j in live))
        prev = t
        if on:
            live.add(i)
        else:
            live.discard(i)
    # A kernel's start stamp is taken when its dispatch begins, not when its first workgroup gets a CU: a recurrence held off by a
    # persistent grid shows as a LONGER launch, by what was left of that grid.  So: each recurrence launch against the time the
    # longest-running projection of another stream still had to go at its start.
    projs = [r for r in rows if r["kind"] == "proj" and r["end"] > t0]
    left, rdur = [], []
    for r in recs:
        if r["start"] >= t0:
            left.append(max([p["end"] - r["start"] for p in projs if p["stream"] != r["stream"] and p["start"] <= r["start"] < p["end"]], default=0) / 1e3)
            rdur.append((r["end"] - r["start"]) / 1e3)
    under = [d for d, l in zip(rdur, left) if l > 0]
    clear = [d for d, l in zip(rdur, left) if l == 0]
    n, sx, sy = len(left), sum(left), sum(rdur)
    sxx, sxy = sum(x * x for x in left), sum(x * y for x, y in zip(left, rdur))
    slope = (n * sxy - sx * sy) / (n * sxx - sx * sx) if n * sxx - sx * sx > 0 else None
    # ... and the projections that queue behind each other for the chip
    pp = [p for p in projs if any(q is not p and q["stream"] != p["stream"] and q["start"] <= p["start"] < q["end"] for q in projs)]
    pdur = lambda ps: quantile([(p["end"] - p["start"]) / 1e3 for p in ps], 0.5)
    held_off = {"recurrences_started_under_another_streams_projection_share": len(under) / max(n, 1),
                "recurrence_us_median_when_so": quantile(under, 0.5), "recurrence_us_median_otherwise": quantile(clear, 0.5),
                "recurrence_us_per_us_of_projection_left": slope,
                "projections_started_under_another_streams_projection_share": len(pp) / max(len(projs), 1),
                "projection_us_median_when_so": pdur(pp), "projection_us_median_otherwise": pdur([p for p in projs if p not in pp])}
    wall = t1 - t0
    dur = lambda k: [(r["end"] - r["start"]) / 1e3 for r in rows if r["kind"] == k and r["start"] >= t0]
    return {
        "window_ms": wall / 1e6, "streams": len({r["stream"] for r in rows if r["start"] >= t0}),
        "recurrence_launches": len(delays), "steps_in_window": len([r for r in recs if r["start"] >= t0]) / LAYERS,
        "ms_per_step": wall / 1e6 / (len([r for r in recs if r["start"] >= t0]) / LAYERS),
        "dispatch_delay_us": {"median": quantile(delays, 0.5), "p90": quantile(delays, 0.9)},
        "rec_beside_other_proj_share": beside / wall, "recs_only_share": recs_only / wall, "mean_cus_held": cu_ns / wall,
        "recurrence_us": {"median": quantile(dur("rec"), 0.5), "p90": quantile(dur("rec"), 0.9)},
        "projection_us": {"median": quantile(dur("proj"), 0.5), "p90": quantile(dur("proj"), 0.9)},
        "held_off": held_off,
        "projection_grids": sorted({r["wgs"] for r in rows if r["kind"] == "proj" and r["start"] >= t0}),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("trace", help="kernel_trace.csv, or a directory that holds one")
    ap.add_argument("--steps", type=int, default=60, help="timed steps of the traced bench.py run")
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--out", default=None, help="also write the summary to this JSON file")
    a = ap.parse_args()
    path = a.trace
    if os.path.isdir(path):
        found = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
        if not found:
            raise SystemExit(f"no *kernel_trace.csv under {path}")
        path = max(found, key=os.path.getsize)   # (bench.py's own process; helper processes trace next to nothing)
    rows, key = read_rows(path)
    out = summarize(rows, a.steps, a.cus)
    out["streams_told_apart_by"] = key
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    sys.exit(main())
