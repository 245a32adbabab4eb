#!/usr/bin/env python3
"""Which hardware queue each of the library's streams landed on, and what that costs the pipeline, from one
rocprofv3 --kernel-trace CSV of a pipelined run (bench.py):

    python tools/queue_trace.py kernel_trace.csv [--last 20 --drop-tail 3]

Reports (profiles/r22_*):
  - per stream: its queue id, its kernels by name and count -- streams that share a queue id serialise;
  - over the steady part of the run (from the start of the first to the end of the last of --last accumulations, the
    final --drop-tail ones left out: the pipeline drains there; set-up and warm-up, with their host-side gaps, come
    before): the time during which 0, 1, 2 and more k_accumulate kernels are resident;
  - per k_accumulate: the gap between its start and the end of the last kernel before it on the same QUEUE, split by
    whether that kernel came from the accumulation's own stream or from another stream of the queue.
"""
import argparse
import collections
import csv
import statistics


def role(names):
    if any("k_accumulate" in n for n in names):
        return "main"
    if any("k_digits" in n or "k_convert_points" in n for n in names):
        return "pre"
    if any("k_reduce_segments" in n or "k_merge_large" in n for n in names):
        return "tail"
    return "other"


def short(name):
    name = name.split("(")[0].split("::")[-1]
    return name.split("<")[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--last", type=int, default=20, help="accumulations of the steady part")
    ap.add_argument("--drop-tail", type=int, default=3, help="final accumulations left out (the pipeline drains)")
    args = ap.parse_args()
    rows = []
    with open(args.csv) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), int(r["Queue_Id"]), int(r["Stream_Id"]),
                         r["Kernel_Name"]))
    rows.sort()
    acc = [r for r in rows if "k_accumulate" in r[4]]
    if not acc:
        raise SystemExit("no k_accumulate in the trace")
    acc.sort(key=lambda r: r[0])
    steady = acc[:len(acc) - args.drop_tail][-args.last:]
    t0 = steady[0][0]
    t1 = max(r[1] for r in steady)
    lib = [r for r in rows if "curdle::" in r[4] and r[1] >= acc[0][0] and r[0] <= t1]

    by_stream = collections.defaultdict(lambda: {"q": set(), "names": collections.Counter()})
    for s, e, q, st, n in lib:
        by_stream[st]["q"].add(q)
        by_stream[st]["names"][short(n)] += 1
    print("stream  queue  role  kernels")
    per_queue = collections.defaultdict(list)
    for st in sorted(by_stream):
        b = by_stream[st]
        rl = role(b["names"])
        for q in b["q"]:
            per_queue[q].append(f"{rl}:{st}")
        print(f"{st:6d}  {','.join(map(str, sorted(b['q']))):>5}  {rl:5} " +
              " ".join(f"{k}x{v}" for k, v in b["names"].most_common()))
    print("queue -> streams: " + "; ".join(f"{q}: {' '.join(v)}" for q, v in sorted(per_queue.items())))
    busy = [r for r in by_stream.values() if role(r["names"]) != "other"]
    print(f"busy streams {len(busy)} on {len(set().union(*[r['q'] for r in busy]))} queue ids")

    # residency of k_accumulate
    ev = []
    for s, e, *_ in acc:
        s, e = max(s, t0), min(e, t1)
        if e > s:
            ev += [(s, 1), (e, -1)]
    ev.sort()
    level, last, hist = 0, t0, collections.Counter()
    for t, d in ev:
        hist[level] += t - last
        last = t
        level += d
    hist[level] += t1 - last
    span = t1 - t0
    n_acc = len(steady)
    print(f"steady span {span / 1e6:.3f} ms, {n_acc} accumulations, {span / 1e6 / max(1, n_acc):.3f} ms per accumulation")
    for k in sorted(hist):
        print(f"  {k} k_accumulate resident: {hist[k] / 1e6:8.3f} ms  {100.0 * hist[k] / span:5.1f} %")
    fewer = sum(v for k, v in hist.items() if k < 2)
    print(f"  fewer than two resident: {fewer / 1e6:.3f} ms, {fewer / 1e6 / max(1, n_acc):.3f} ms per accumulation")
    print(f"  k_accumulate duration: median {statistics.median((e - s) / 1e6 for s, e, *_ in acc):.3f} ms")

    # gap between an accumulation's start and the end of the kernel before it on the same queue
    by_queue = collections.defaultdict(list)
    for r in rows:
        by_queue[r[2]].append(r)
    gaps = {"own": [], "other": []}
    behind = collections.Counter()
    for q, rs in by_queue.items():
        rs.sort(key=lambda r: r[1])
        for a in (r for r in rs if "k_accumulate" in r[4] and t0 <= r[0] <= t1):
            prev = [r for r in rs if r[1] <= a[0] + 1000 and r is not a]
            if not prev:
                continue
            p = prev[-1]
            kind = "own" if p[3] == a[3] else "other"
            gaps[kind].append((a[0] - p[1]) / 1e6)
            if kind == "other":
                behind[short(p[4])] += 1
    for kind, g in gaps.items():
        if g:
            tight = sum(1 for x in g if x < 0.02)
            print(f"accumulations whose queue predecessor is of {kind} stream: {len(g)}; gap median {statistics.median(g):.3f} ms, "
                  f"max {max(g):.3f}; started within 0.02 ms of it: {tight}")
    if behind:
        print("  predecessors from another stream: " + " ".join(f"{k}x{v}" for k, v in behind.most_common()))


if __name__ == "__main__":
    main()
