"""Reduce the Welch-primitive profile runs (tools/time_psd.py under rocprofv3) to one row per workload:

    python tools/psd_pmc_table.py DIR [--trim]
    (DIR: time_psd.json, trace/*/*_kernel_stats.csv, pmc_<counter>/*/*_counter_collection.csv)

Fetched bytes = 2 x FETCH_SIZE KiB per psd_kernel dispatch (median over the timed loop), divided by the algorithmic bytes
(the input); kernel times from the trace.  The factor 2: on gfx950 FETCH_SIZE tallies the 128-byte requests of a wide
(16 bytes per lane) streaming read at 64 bytes each (tools/reduce_pmc.py, profiles/r07).  The raw counter is
printed beside it as the check: the kernel reads every byte of an input twice the size of the 256 MiB last-level cache
at least once, so a raw ratio near 0.5 cannot be the traffic and the doubled figure is.
The kernel of a workload is found by its signal type, components per sample and log2 n_fft; the LDS image's type (float64
by default, float32 under option psd_f32_image) is whatever the run used.
--trim rewrites every counter file to the psd dispatches of the timed loops (the last 20 per kernel), summed over the
counter's instances, and the kernel statistics to the psd kernels: what the repository keeps."""
import csv
import glob
import json
import os
import re
import statistics
import sys

# workload -> (signal scalar, components per sample, log2 n_fft) of psd_kernel<SI, T, NC, LOG2N>
KERNEL_OF = {"C256": ("float", 2, 8), "C1024": ("float", 2, 10), "C4096": ("float", 2, 12), "F1024": ("float", 1, 10),
             "D1024": ("double", 1, 10)}
KEEP = 20


def kernel_of(wl, names):
    """The psd_kernel instantiation of workload wl among the kernel names of a run (None if it did not run)."""
    si, nc, log2n = KERNEL_OF[wl]
    pat = re.compile(r"psd_kernel<%s, (float|double), %d, %d>" % (si, nc, log2n))
    hits = sorted(n for n in names if pat.search(n))
    if len(hits) > 1:
        raise SystemExit("%s: more than one LDS image type in one run: %s" % (wl, hits))
    return hits[0] if hits else None


def dispatches(f):
    """{(kernel, counter): {dispatch id: value summed over instances}} of one counter file, psd kernels only."""
    per = {}
    for r in csv.DictReader(open(f)):
        if "psd_" not in r["Kernel_Name"]:
            continue
        d = per.setdefault((r["Kernel_Name"], r["Counter_Name"]), {})
        d[int(r["Dispatch_Id"])] = d.get(int(r["Dispatch_Id"]), 0.0) + float(r["Counter_Value"])
    return {k: dict(sorted(v.items())[-KEEP:]) for k, v in per.items()}


def main(d, trim):
    recs = {json.loads(line)["workload"]: json.loads(line) for line in open(os.path.join(d, "time_psd.json"))}
    c = {}
    for f in glob.glob(os.path.join(d, "pmc_*", "*", "*_counter_collection.csv")):
        per = dispatches(f)
        if trim:
            with open(f, "w", newline="") as out:
                w = csv.writer(out)
                w.writerow(["Kernel_Name", "Counter_Name", "Dispatch_Id", "Counter_Value"])
                for (kn, cn), v in sorted(per.items()):
                    for did, val in v.items():
                        w.writerow([kn, cn, did, val])
        c.update({k: statistics.median(v.values()) for k, v in per.items()})
    stats = {}
    for f in glob.glob(os.path.join(d, "trace", "*", "*_kernel_stats.csv")):
        rows = [r for r in csv.DictReader(open(f)) if "psd_" in r["Name"]]
        for r in rows:
            stats[r["Name"]] = float(r["AverageNs"]) / 1e6
        if trim and rows:
            with open(f, "w", newline="") as out:
                w = csv.DictWriter(out, fieldnames=list(rows[0].keys()))
                w.writeheader()
                w.writerows(rows)
    red = next((v for k, v in stats.items() if "psd_reduce_kernel" in k), float("nan"))
    print("%-6s %-36s %9s %9s %9s %8s %9s %9s %10s %8s" % ("", "kernel", "trace ms", "reduce ms", "event ms", "TB/s", "fetch GB", "alg GB", "fetch/alg",
                                                            "raw/alg"))
    for wl, rec in recs.items():
        kn = kernel_of(wl, stats)
        kc = kernel_of(wl, [k for (k, cn) in c if cn == "FETCH_SIZE"])
        raw = c.get((kc, "FETCH_SIZE"), float("nan")) * 1024
        fetch = 2 * raw
        ms = stats.get(kn, float("nan"))
        short = re.search(r"psd_kernel<[^>]*>", kn or kc or "").group(0) if (kn or kc) else "(not run)"
        print("%-6s %-36s %9.4f %9.4f %9.4f %8.3f %9.3f %9.3f %10.3f %8.3f" % (wl, short, ms, red, rec["ms"], rec["alg_bytes"] / rec["ms"] / 1e9,
                                                                           fetch / 1e9, rec["alg_bytes"] / 1e9, fetch / rec["alg_bytes"],
                                                                           raw / rec["alg_bytes"]))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(args[0] if args else ".", "--trim" in sys.argv)
