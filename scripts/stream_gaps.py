"""Where a pipeline frame's device time is EMPTY: from a rocprofv3 --kernel-trace CSV of bench.py (no counters in that run), the time per frame in which no
kernel runs on any stream, attributed to what the host was doing — waiting for the sky pre-pass's count, polling the round loop (a gap between two rounds'
kernels), switching to the drain pool, reducing — plus launches and summed launch time per kernel and frame.

    python3 scripts/stream_gaps.py <kernel_trace.csv> [frames to skip at the start, default 1: the counting pass]

A frame ends with its stream_reduce.  A gap belongs to the frame it lies in; the time between a frame's reduce and the next frame's first kernel is the
caller's (bench.py's step), reported apart."""
import collections
import csv
import re
import sys


def short(name):
    m = re.search(r"(sky_\w+|stream_\w+|fused_render|accum_\w+)", name)
    return m.group(1) if m else name[:40]


def main():
    path = sys.argv[1]
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    rows = []
    for r in csv.DictReader(open(path)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), r.get("Stream_Id") or r.get("Queue_Id") or "0"))
    rows.sort()
    frames, cur = [], []
    for k in rows:
        cur.append(k)
        if k[2] in ("stream_reduce", "stream_reduce_split"):
            frames.append(cur); cur = []
    frames = frames[skip:]
    if not frames:
        print("no frame found"); return
    tot = collections.Counter(); launches = collections.Counter(); busy_ms = collections.Counter()
    span_ms = 0.0; between = []
    prev_end = None
    for f in frames:
        t0, t1 = f[0][0], max(k[1] for k in f)
        if prev_end is not None:
            between.append((t0 - prev_end) * 1e-6)
        prev_end = t1
        span_ms += (t1 - t0) * 1e-6
        for k in f:
            launches[k[2]] += 1; busy_ms[k[2]] += (k[1] - k[0]) * 1e-6
        # union of the kernels' intervals; a gap is named after the kernel that ended last before it and the one that starts after it
        end, last = f[0][1], f[0][2]
        for s, e, name, _ in f[1:]:
            if s > end:
                gap = (s - end) * 1e-6
                if last.startswith("sky_"):
                    what = "pre-pass (the host waits for the count of pixels to walk)"
                elif name.startswith("stream_compact") or last.startswith("stream_compact"):
                    what = "drain switch"
                elif name.startswith("stream_reduce") or name == "stream_sum_counters":
                    what = "before the reduce (last poll)"
                elif name.startswith("sky_") or name == "stream_init":
                    what = "frame start"
                else:
                    what = "between rounds (poll)"
                tot[what] += gap; tot["_n " + what] += 1
            if e > end:
                end, last = e, name
    n = len(frames)
    print(f"{n} frame(s); first kernel to end of reduce {span_ms / n:.3f} ms per frame; between frames (the caller) {sum(between) / max(1, len(between)):.3f} ms")
    empty = sum(v for k, v in tot.items() if not k.startswith("_n "))
    print(f"no kernel on any stream: {empty / n:.3f} ms per frame = {100 * empty / span_ms:.2f} % of the frame")
    for k, v in sorted(tot.items()):
        if not k.startswith("_n "):
            print(f"  {k:58s} {v / n:8.3f} ms per frame in {tot['_n ' + k] / n:.1f} gaps")
    print("kernel                         launches/frame   ms/frame   ms/launch")
    for k, c in sorted(launches.items(), key=lambda kv: -busy_ms[kv[0]]):
        print(f"  {k:28s} {c / n:10.1f} {busy_ms[k] / n:12.3f} {busy_ms[k] / c:10.4f}")
    streams = sorted({k[3] for f in frames for k in f})
    for sid in streams:   # a stream's own idle time inside the frames: what the other stream's kernels may or may not cover
        b = sum((k[1] - k[0]) for f in frames for k in f if k[3] == sid) * 1e-6
        print(f"  stream/queue {sid}: {b / n:.3f} ms of kernels per frame")


if __name__ == "__main__":
    main()
