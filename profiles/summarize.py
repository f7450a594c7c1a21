#!/usr/bin/env python3
"""Summarize a rocprofv3 result DB (--kernel-trace [-o name]) into the
per-kernel table committed under profiles/.

Usage: python profiles/summarize.py <results.db>
       python profiles/summarize.py --table <results.db> <ticks> [title]
       python profiles/summarize.py --timeline <results.db> <tick> [title]
The second form prints the launches / total ms / avg us table of the
*_kernels.txt files, with per-tick dispatch count and kernel time over
<ticks> ticks (timed + warmup).  The third prints the *_timeline.txt files:
every dispatch of one q3 tick period with begin / end relative to the tick's
flatmap, and the medians over the steady-state periods of the distances that
tell which chain bounds the step: tail(t) end -> flatmap(t+1) begin (the
stream the tail runs on), sort end -> head copy end (the device's part of
the host loop) and head copy end -> flatmap(t+1) begin (the host's part).
"""
import sqlite3
import sys


def summarize(path):
    db = sqlite3.connect(path)
    cur = db.cursor()
    sfx = [r[0] for r in cur.execute(
        "SELECT name FROM sqlite_master WHERE name LIKE 'rocpd_kernel_dispatch%'"
    )][0].replace('rocpd_kernel_dispatch_', '')
    q = f"""SELECT ks.display_name, COUNT(*) n,
                   SUM(kd.end-kd.start)/1e6 ms, AVG(kd.end-kd.start)/1e3 avg
            FROM rocpd_kernel_dispatch_{sfx} kd
            JOIN rocpd_info_kernel_symbol_{sfx} ks ON kd.kernel_id = ks.id
            GROUP BY ks.display_name ORDER BY ms DESC"""
    lines = []
    tot = 0.0
    for name, n, ms, avg in cur.execute(q).fetchall():
        tot += ms
        lines.append(f"{name.split('(')[0][:52]:52s} n={n:6d} "
                     f"total={ms:9.3f}ms avg={avg:9.3f}us")
    rows = cur.execute(
        f"SELECT start,end FROM rocpd_kernel_dispatch_{sfx} ORDER BY start"
    ).fetchall()
    span = (rows[-1][1] - rows[0][0]) / 1e6
    gaps = sum(max(0, rows[i + 1][0] - rows[i][1])
               for i in range(len(rows) - 1)) / 1e6
    lines.append(f"TOTAL kernel time {tot:.2f} ms; dispatch span {span:.2f} ms; "
                 f"inter-dispatch gaps {gaps:.2f} ms; {len(rows)} dispatches")
    return "\n".join(lines)


def table(path, ticks, title=""):
    db = sqlite3.connect(path)
    cur = db.cursor()
    sfx = [r[0] for r in cur.execute(
        "SELECT name FROM sqlite_master WHERE name LIKE 'rocpd_kernel_dispatch%'"
    )][0].replace('rocpd_kernel_dispatch_', '')
    rows = cur.execute(
        f"""SELECT ks.display_name, COUNT(*) n,
                   SUM(kd.end-kd.start)/1e6 ms, AVG(kd.end-kd.start)/1e3 avg
            FROM rocpd_kernel_dispatch_{sfx} kd
            JOIN rocpd_info_kernel_symbol_{sfx} ks ON kd.kernel_id = ks.id
            GROUP BY ks.display_name ORDER BY ms DESC""").fetchall()
    tot = sum(r[2] for r in rows)
    nd = sum(r[1] for r in rows)
    lines = []
    if title:
        lines.append(title)
    lines.append(f"total kernel time {tot:.1f} ms over {nd} dispatches "
                 f"(~{tot / ticks * 1e3:.0f} us/tick GPU, "
                 f"{nd / ticks:.1f} dispatches/tick over {ticks} ticks)")
    lines.append("")
    lines.append("launches   total ms   avg us  kernel")
    for name, n, ms, avg in rows:
        if ms < 0.025:
            continue
        lines.append(f"{n:8d} {ms:10.2f} {avg:8.1f}  {name}")
    return "\n".join(lines)


def _short(name):
    name = name.split("(")[0].replace("void ", "")
    return name.replace("__amd_rocclr_", "rocclr:")


def timeline(path, tick_no, title=""):
    """One steady-state q3 tick period from the per-dispatch timestamps: every
    dispatch from the tick_no-th k_flatmap's begin to the next one's, in us
    relative to that begin, with the queue it ran on; then, over all full
    periods from tick 10 on, the medians of the three distances that say which
    chain bounds the step."""
    db = sqlite3.connect(path)
    cur = db.cursor()
    sfx = [r[0] for r in cur.execute(
        "SELECT name FROM sqlite_master WHERE name LIKE 'rocpd_kernel_dispatch%'"
    )][0].replace('rocpd_kernel_dispatch_', '')
    cols = [r[1] for r in cur.execute(
        f"PRAGMA table_info(rocpd_kernel_dispatch_{sfx})")]
    qcol = "kd.queue_id" if "queue_id" in cols else "0"
    rows = cur.execute(
        f"""SELECT ks.display_name, kd.start, kd.end, {qcol}
            FROM rocpd_kernel_dispatch_{sfx} kd
            JOIN rocpd_info_kernel_symbol_{sfx} ks ON kd.kernel_id = ks.id
            ORDER BY kd.start""").fetchall()
    rows = [(_short(n), s, e, q) for n, s, e, q in rows]
    starts = [i for i, r in enumerate(rows) if r[0] == "k_flatmap"]
    lines = [title] if title else []

    def period(t):
        return rows[starts[t]:starts[t + 1] + 1]

    t0 = rows[starts[tick_no]][1]
    lines.append(f"tick {tick_no}: begin / end / length in us from its "
                 f"k_flatmap's begin; queue")
    for n, s, e, q in period(tick_no):
        lines.append(f"{(s - t0) / 1e3:9.2f} {(e - t0) / 1e3:9.2f} "
                     f"{(e - s) / 1e3:7.2f}  q{q}  {n}")

    def med(xs):
        xs = sorted(xs)
        return xs[len(xs) // 2] if xs else float("nan")

    per, next_fm, head_after_sort, merge_len, host_part = [], [], [], [], []
    for t in range(10, len(starts) - 1):
        p = period(t)
        names = [r[0] for r in p[:-1]]
        if "k_join_tail_small" not in names or \
                "k_sort_cons_small<long>" not in names:
            continue
        tail = p[names.index("k_join_tail_small")]
        sort = p[names.index("k_sort_cons_small<long>")]
        merge = [r for r in p[:-1] if r[0].startswith(("k_acc_fold",
                                                       "k_merge_mid_fused"))]
        copies = [r for r in p[:-1] if r[0] == "rocclr:copyBuffer"]
        if not merge or not copies:
            continue
        # the head copy follows the fold on the fold's own queue
        head = [r for r in copies
                if r[1] >= merge[0][2] and r[3] == merge[0][3]]
        if not head:
            continue
        per.append((p[-1][1] - p[0][1]) / 1e3)
        next_fm.append((p[-1][1] - tail[2]) / 1e3)
        head_after_sort.append((head[0][2] - sort[2]) / 1e3)
        merge_len.append((merge[0][2] - merge[0][1]) / 1e3)
        host_part.append((p[-1][1] - head[0][2]) / 1e3)
    lines.append("")
    lines.append(f"medians over {len(per)} periods (tick 10 on):")
    lines.append(f"  period, flatmap(t) begin -> flatmap(t+1) begin  "
                 f"{med(per):7.2f} us")
    lines.append(f"  tail(t) end -> flatmap(t+1) begin               "
                 f"{med(next_fm):7.2f} us")
    lines.append(f"    (flatmap(t+1) began before tail(t) ended in "
                 f"{sum(x < 0 for x in next_fm)} of {len(next_fm)} periods)")
    lines.append(f"  sort end -> head copy end (fold/merge + copy)   "
                 f"{med(head_after_sort):7.2f} us")
    lines.append(f"  head copy end -> flatmap(t+1) begin (host part) "
                 f"{med(host_part):7.2f} us")
    lines.append(f"  accumulator fold / merge kernel                 "
                 f"{med(merge_len):7.2f} us")
    return "\n".join(lines)


if __name__ == "__main__":
    if sys.argv[1] == "--table":
        print(table(sys.argv[2], int(sys.argv[3]), " ".join(sys.argv[4:])))
    elif sys.argv[1] == "--timeline":
        print(timeline(sys.argv[2], int(sys.argv[3]), " ".join(sys.argv[4:])))
    else:
        print(summarize(sys.argv[1]))
