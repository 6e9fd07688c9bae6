"""What the scripts/*_time.py share: the repository root on sys.path, two timers and the kernel table of a traced run.

    from timing import ROOT, kernel_table, sync_time, timed
"""
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sync_time(fn):
    """-> (device-synchronised wall seconds of one fn(), its result)."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def timed(fn, reps):
    """One warm-up, then -> (median, minimum, maximum of `reps` device-synchronised wall seconds, the last result)."""
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts), r


def kernel_table(script, args, caption, rows, limit=300, family=None):
    """`script` with `args` once more, as a fresh process under `rocprofv3 --kernel-trace --stats` with `limit` seconds -> the lines of its
    kernel table: the `rows` longest kernels.  caption: what the run does, then the format of the kernel count and the seconds of kernel
    time.  family = (noun, prefix): a last line sums the kernels whose name holds the prefix."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(script)] + args
        p = subprocess.run(cmd, capture_output=True, text=True)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not found:
            return ["# no kernel table: rocprofv3 exit %s, %d stats files" % (p.returncode, len(found))]
        table = list(csv.DictReader(open(found[0])))
    total = sum(float(r["TotalDurationNs"]) for r in table)
    out = ["# rocprofv3 --kernel-trace --stats, a run of its own: " + caption % (len(table), total * 1e-9),
           "# %-72s %8s %12s %10s %7s" % ("kernel", "calls", "total ms", "avg us", "%")]
    for r in sorted(table, key=lambda r: -float(r["TotalDurationNs"]))[:rows]:
        out.append("  %-72s %8d %12.3f %10.2f %7.2f" % (r["Name"].split("(")[0][-72:], int(r["Calls"]), float(r["TotalDurationNs"]) * 1e-6,
                                                       float(r["TotalDurationNs"]) / int(r["Calls"]) * 1e-3, 100.0 * float(r["TotalDurationNs"]) / total))
    if family is not None:
        own = [r for r in table if family[1] in r["Name"]]
        out.append("# the %s kernels (%s*): %d launches, %.3f ms in all" % (family[0], family[1], sum(int(r["Calls"]) for r in own),
                                                                          sum(float(r["TotalDurationNs"]) for r in own) * 1e-6))
    return out
