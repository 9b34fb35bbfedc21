"""Reduce the Farrow profile runs (tools/time_farrow.py under rocprofv3) to one row per workload:

    python tools/farrow_pmc_table.py DIR     (DIR: time_farrow.json, trace/*/*_kernel_stats.csv, pmc_<first counter>/*/*_counter_collection.csv)

HBM traffic = 2 x FETCH_SIZE + WRITE_SIZE (FETCH_SIZE reports half the bytes of a wide streaming read on gfx950), per dispatch
(median over the run), divided by the algorithmic bytes esz_in n + esz_out N; SQ_INSTS_VALU per output; kernel time from the trace."""
import csv
import glob
import json
import os
import statistics
import sys

KERNEL_OF = {"W1": "farrow_kernel<float, float, double, 2, 3>", "W2": "farrow_kernel<float, float, double, 1, 3>",
             "W3": "farrow_kernel<double, double, double, 1, 3>"}


def counters(d):
    per = {}
    for f in glob.glob(os.path.join(d, "pmc_*", "*", "*_counter_collection.csv")):
        for r in csv.DictReader(open(f)):
            per.setdefault((r["Kernel_Name"], r["Counter_Name"]), {}).setdefault(r["Dispatch_Id"], 0.0)
            per[(r["Kernel_Name"], r["Counter_Name"])][r["Dispatch_Id"]] += float(r["Counter_Value"])
    return {k: statistics.median(v.values()) for k, v in per.items()}


def main(d):
    recs = {json.loads(line)["workload"]: json.loads(line) for line in open(os.path.join(d, "time_farrow.json"))}
    stats = {}
    for f in glob.glob(os.path.join(d, "trace", "*", "*_kernel_stats.csv")):
        for r in csv.DictReader(open(f)):
            stats[r["Name"]] = float(r["AverageNs"]) / 1e6
    c = counters(d)
    print("%-3s %-45s %9s %9s %8s %9s %9s %10s %8s" % ("", "kernel", "trace ms", "event ms", "TB/s", "HBM GB", "alg GB", "HBM/alg", "VALU/out"))
    for w, rec in sorted(recs.items()):
        kn = next((k for k in stats if KERNEL_OF[w] in k), None)
        get = lambda name: next((v for (k, cn), v in c.items() if cn == name and KERNEL_OF[w] in k), float("nan"))  # noqa: E731
        hbm = (2 * get("FETCH_SIZE") + get("WRITE_SIZE")) * 1024
        valu = get("SQ_INSTS_VALU") * 64 / rec["n_out"]   # SQ_INSTS_VALU counts wave instructions
        ms = stats.get(kn, float("nan"))
        print("%-3s %-45s %9.4f %9.4f %8.3f %9.3f %9.3f %10.3f %8.1f" % (w, KERNEL_OF[w], ms, rec["ms"], rec["alg_bytes"] / ms / 1e9,
                                                                    hbm / 1e9, rec["alg_bytes"] / 1e9, hbm / rec["alg_bytes"], valu))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else ".")
