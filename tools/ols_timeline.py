"""Developer aid: when does each workgroup of the headline overlap-save launch start, walk its tiles and end?
   make -C scikit-dsp-comm_amd/csrc timeline          # libskdsp_timeline.so: fir_ols.hip with -DSKDSP_OLS_TIMELINE_BUILD
   python tools/ols_timeline.py [--out profiles/r18/timeline_fir1024.json] [--log2n 26] [--walks 0,1] [--stamps]
Thread 0 of every workgroup of ols_tile_kernel stamps wall_clock64 (100 MHz) at entry, behind the table barrier, behind the issue of each
tile's stores and at exit.  One SETTLED launch per walk (150 launches in front of it) of multirate_FIR.filter, 1024 taps, complex64, 2^log2n samples;
the JSON holds, per walk, one column per field over the workgroups: blockIdx, XCD (blockIdx % 8), start / tables / end (us behind the launch's
first entry) and the tiles walked (--stamps: also every tile's stamp and index); the summary that profiles/r18/README.md quotes, which is
computed from the per-tile stamps, goes to stdout."""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scikit-dsp-comm_amd"))
os.environ.setdefault("SKDSP_LIB", os.path.join(ROOT, "scikit-dsp-comm_amd", "sk_dsp_comm_amd", "libskdsp_timeline.so"))
import numpy as np
import bench
from sk_dsp_comm_amd import _ffi

TICK_US = 0.01   # wall_clock64: 100 MHz
HEAD, STEPS = 4, 64

def arg(name, default):
    if name in sys.argv:
        return sys.argv[sys.argv.index(name) + 1]
    return default

def one_walk(walk, k, xd, yd, buf, nwg):
    lib = _ffi.load()
    words = HEAD + 2 * STEPS
    with _ffi.option("ols_walk", walk):
        lib.skdsp_ols_timeline_arm(ctypes.c_void_p(None), 0)
        for _ in range(150): k.filter_dev(xd, yd)
        _ffi.sync()
        buf.write(np.zeros(buf.nbytes, np.uint8))
        lib.skdsp_ols_timeline_arm(ctypes.c_void_p(buf.ptr), STEPS)
        k.filter_dev(xd, yd)
        _ffi.sync()
        lib.skdsp_ols_timeline_arm(ctypes.c_void_p(None), 0)
    rec = buf.read().view(np.uint64).reshape(nwg, words)
    rec = rec[rec[:, 0] != 0]   # the launch's grid may be smaller than the buffer
    t0 = int(rec[:, 0].min())
    us = lambda v: round((int(v) - t0) * TICK_US, 2)
    wgs = []
    for b, r in enumerate(rec):
        steps = min(int(r[3]), STEPS)
        wgs.append({"block": b, "xcd": b % 8, "start": us(r[0]), "tables": us(r[1]), "end": us(r[2]), "tiles": int(r[3]),
                    "stamps": [us(r[HEAD + 2 * i]) for i in range(steps)], "tile_index": [int(r[HEAD + 2 * i + 1]) for i in range(steps)]})
    return wgs

def pct(a, q): return float(np.percentile(np.asarray(a, float), q))

def summary(walk, wgs):
    out = []
    start = [w["start"] for w in wgs]; end = [w["end"] for w in wgs]; tiles = [w["tiles"] for w in wgs]
    out.append("walk %d (%s): %d workgroups, %d tiles, launch %.1f us from the first entry to the last exit" % (walk, "claimed" if walk else "dealt", len(wgs), sum(tiles), max(end)))
    out.append("  start (us behind the first entry): median %.2f  p90 %.2f  p99 %.2f  max %.2f" % (pct(start, 50), pct(start, 90), pct(start, 99), max(start)))
    out.append("  table barrier behind entry: median %.2f  max %.2f us" % (pct([w["tables"] - w["start"] for w in wgs], 50), max(w["tables"] - w["start"] for w in wgs)))
    out.append("  exit: first %.1f  median %.1f  last %.1f us  (last - first %.1f us; mean idle behind a workgroup's exit %.1f us = %.1f %% of the launch)"
               % (min(end), pct(end, 50), max(end), max(end) - min(end), max(end) - float(np.mean(end)), 100 * (max(end) - float(np.mean(end))) / max(end)))
    out.append("  tiles per workgroup: min %d  median %d  max %d" % (min(tiles), int(pct(tiles, 50)), max(tiles)))
    # per-tile time: the difference of consecutive stamps (the first tile from the table barrier: it holds the first load's latency)
    per = {}    # (xcd, round) -> list
    mean_wg = []
    for w in wgs:
        d = np.diff([w["tables"]] + w["stamps"])
        if d.size > 1: mean_wg.append(float(np.mean(d[1:])))
        for i, v in enumerate(d): per.setdefault((w["xcd"], i), []).append(float(v))
    out.append("  a workgroup's mean time per tile (first tile left out): min %.2f  p10 %.2f  median %.2f  p90 %.2f  max %.2f us  (max / min %.3f)"
               % (min(mean_wg), pct(mean_wg, 10), pct(mean_wg, 50), pct(mean_wg, 90), max(mean_wg), max(mean_wg) / min(mean_wg)))
    out.append("  per-tile time by XCD (rounds 1 on), mean (sd) us: " + "  ".join(
        "%d: %.2f (%.2f)" % (x, np.mean(sum((v for (xx, r), v in per.items() if xx == x and r > 0), [])), np.std(sum((v for (xx, r), v in per.items() if xx == x and r > 0), []))) for x in range(8)))
    rounds = sorted({r for (_, r) in per})
    out.append("  per-tile time by round, mean (sd) [n]: " + "  ".join(
        "%d: %.2f (%.2f) [%d]" % (r, np.mean(sum((v for (x, rr), v in per.items() if rr == r), [])), np.std(sum((v for (x, rr), v in per.items() if rr == r), [])), len(sum((v for (x, rr), v in per.items() if rr == r), []))) for r in rounds))
    return out

def main():
    log2n = int(arg("--log2n", "26"))
    walks = [int(v) for v in arg("--walks", "0,1").split(",")]
    out_path = arg("--out", os.path.join(ROOT, "profiles", "r18", "timeline_fir1024.json"))
    _ffi.init(0)
    lib = _ffi.load()
    if not hasattr(lib, "skdsp_ols_timeline_arm"):
        raise SystemExit("%s is not a timeline build (make -C scikit-dsp-comm_amd/csrc timeline)" % _ffi.lib_path())
    lib.skdsp_ols_timeline_arm.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.skdsp_ols_timeline_arm.restype = None
    n = 1 << log2n
    k = _ffi.FirKernel(bench.firwin_lowpass(1024, 0.2), _ffi.C64)
    xd = _ffi.DeviceArray(n, np.complex64, headroom=1024).fill_noise(1)
    yd = _ffi.DeviceArray(n, np.complex64)
    nwg = 2 * _ffi.device_info()["compute_units"]   # (the launch's grid is at most this)
    buf = _ffi.DeviceBytes(nwg * (HEAD + 2 * STEPS) * 8)
    doc = {"workload": "multirate_FIR.filter, 1024 taps, complex64, 2^%d samples" % log2n, "unit": "us behind the launch's first workgroup entry (wall_clock64, 100 MHz)",
           "device": _ffi.device_info()["name"], "walks": {}}
    keys = ["block", "xcd", "start", "tables", "end", "tiles"] + (["stamps", "tile_index"] if "--stamps" in sys.argv else [])
    for walk in walks:
        wgs = one_walk(walk, k, xd, yd, buf, nwg)
        doc["walks"][str(walk)] = {key: [w[key] for w in wgs] for key in keys}   # one column per field, workgroups in blockIdx order
        print("\n".join(summary(walk, wgs)), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(key) + ": " + json.dumps(v, separators=(",", ":")) for key, v in doc.items() if key != "walks"))
        for walk, cols in doc["walks"].items():   # (one line per column: the file diffs and reads by field)
            f.write(",\n" + json.dumps("walk_%s" % walk) + ": {\n" + ",\n".join(json.dumps(key) + ": " + json.dumps(v, separators=(",", ":")) for key, v in cols.items()) + "\n}")
        f.write("\n}\n")
    print("wrote", out_path, file=sys.stderr)

main()
