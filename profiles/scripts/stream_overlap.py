"""How much two streams' kernels overlapped, from a rocprofv3 --kernel-trace csv (no GPU needed).

Usage: stream_overlap.py <dir or kernel_trace.csv> [--top N] [--json OUT]

Kernels are grouped into the bench's categories by name (graph / message / node_dense+heads products / nodewise / stepper / other)
and into streams by the trace's Stream_Id (Queue_Id where the trace has no stream column).  The two streams that carry the
most kernel time are taken as the pair.  Printed:
  * wall = last end - first start, busy = time with at least one kernel in flight, sum = summed kernel time;
  * both = time during which kernels of BOTH streams of the pair were in flight, as a share of busy;
  * per category: its kernel time and the share of it spent while a kernel of the OTHER stream was in flight;
  * the kernel pairs (a on one stream, b on the other) that overlapped longest.
A one-stream trace reports both = 0."""
import argparse
import collections
import csv
import glob
import json
import os

CATS = (("message", ("adf_message_kernel",)),
        ("graph", ("adf_topk", "adf_count", "adf_fill", "adf_sort_edges", "adf_validate", "DeviceScan", "adf_inc_", "DeviceSelect",
                   "adf_embed")),
        ("products", ("adf_gemm16", "adf_gemm_", "gemm16")),
        ("nodewise", ("layernorm", "rowmag", "rowmax", "adf_nodewise", "adf_scatter_rows", "adf_gather_rows", "adf_head", "adf_gate")),
        ("stepper", ("adf_step_", "adf_tr_", "adf_split_", "adf_init_placement")))


def category(name):
    for cat, keys in CATS:
        if any(k in name for k in keys):
            return cat
    return "other"


def short(name):
    return name.split("(")[0].replace("void ", "")[:70]


def load(path):
    files = [path] if os.path.isfile(path) else glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            stream = r.get("Stream_Id") or r.get("Queue_Id") or "0"
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), stream, r["Kernel_Name"]))
    rows.sort()
    return rows


def analyse(rows, top=12):
    per_stream = collections.Counter()
    for s, e, st, _ in rows:
        per_stream[st] += e - s
    pair = [st for st, _ in per_stream.most_common(2)]
    events = []   # (time, +1/-1, stream index, row index)
    for i, (s, e, st, _) in enumerate(rows):
        k = pair.index(st) if st in pair else 2
        events.append((s, 1, k, i))
        events.append((e, -1, k, i))
    events.sort(key=lambda ev: (ev[0], ev[1]))
    live = [set(), set(), set()]
    busy = both = 0
    cat_time = collections.Counter()
    cat_overlapped = collections.Counter()
    pairs = collections.Counter()
    last = events[0][0] if events else 0
    for t, d, k, i in events:
        dt = t - last
        if dt > 0:
            if live[0] or live[1] or live[2]:
                busy += dt
            if live[0] and live[1]:
                both += dt
                for a in live[0]:
                    for b in live[1]:
                        pairs[(short(rows[a][3]), short(rows[b][3]))] += dt
            for k2 in (0, 1):
                for a in live[k2]:
                    c = category(rows[a][3])
                    cat_time[c] += dt
                    if live[1 - k2]:
                        cat_overlapped[c] += dt
            for a in live[2]:
                cat_time[category(rows[a][3])] += dt
        last = t
        (live[k].add if d > 0 else live[k].discard)(i)
    wall = (max(r[1] for r in rows) - min(r[0] for r in rows)) if rows else 0
    total = sum(e - s for s, e, _, _ in rows)
    return {
        "kernels": len(rows), "streams": {st: round(v / 1e6, 2) for st, v in per_stream.most_common()}, "pair": pair,
        "wall_ms": round(wall / 1e6, 2), "busy_ms": round(busy / 1e6, 2), "sum_kernel_ms": round(total / 1e6, 2),
        "both_ms": round(both / 1e6, 2), "both_share_of_busy": round(both / busy, 4) if busy else 0.0,
        "categories": {c: {"kernel_ms": round(cat_time[c] / 1e6, 2),
                           "share_beside_other_stream": round(cat_overlapped[c] / cat_time[c], 4) if cat_time[c] else 0.0}
                       for c in sorted(cat_time, key=lambda c: -cat_time[c])},
        "top_pairs_ms": [[a, b, round(v / 1e6, 2)] for (a, b), v in pairs.most_common(top)],
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("path")
    ap.add_argument("--top", type=int, default=12)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    res = analyse(load(args.path), args.top)
    print(f"{res['kernels']} kernels on streams {res['streams']} (ms of kernel time); pair = {res['pair']}")
    print(f"wall {res['wall_ms']} ms, busy {res['busy_ms']} ms, summed kernel time {res['sum_kernel_ms']} ms")
    print(f"both streams in flight: {res['both_ms']} ms = {100 * res['both_share_of_busy']:.1f} % of busy")
    for c, v in res["categories"].items():
        print(f"  {c:10s} {v['kernel_ms']:10.2f} ms, {100 * v['share_beside_other_stream']:5.1f} % of it beside the other stream")
    for a, b, ms in res["top_pairs_ms"]:
        print(f"  {ms:9.2f} ms  {a}  ||  {b}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
