"""The LDS chain of one kernel of an assembly listing: every ds_read / ds_write run, s_waitcnt lgkmcnt(N) and s_barrier of the
kernel's tile loop, in order, with the number of vector-ALU instructions between them -- what shows whether a table read sits
between two exchange writes and is waited for with lgkmcnt(0).
    hipcc -S --cuda-device-only --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -Iinclude csrc/fir_ols.hip -o fir_ols.s
    python tools/ols_lds_chain.py fir_ols.s 'ols_tile_kernel<false, false, false, false>' [--brief]
The tile loop is taken to be the longest backward branch of the function.  Last line: totals of the loop."""
import re, subprocess, sys

def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))

def function_lines(path, want):
    lines = open(path).read().split("\n")
    starts = [(i, m.group(1)) for i, l in enumerate(lines) for m in [re.match(r"^(_Z\w+):\s*(;.*)?$", l)] if m]
    names = demangle([s for _, s in starts])
    for i, s in starts:
        if want in names[s]:
            j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
            return names[s], lines[i:j]
    raise SystemExit("no kernel matching %r" % want)

def tile_loop(body):
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\w+):", l)] if m}
    best = (0, 0, 0)
    for i, l in enumerate(body):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\w+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i and i - labels[m.group(1)] > best[0]:
            best = (i - labels[m.group(1)], labels[m.group(1)], i)
    return body[best[1]:best[2] + 1]

def main():
    path, want = sys.argv[1], sys.argv[2]
    brief = "--brief" in sys.argv
    name, body = function_lines(path, want)
    loop = tile_loop(body)
    ev, valu, tot = [], 0, {"valu": 0, "packed": 0, "ds_read": 0, "ds_write": 0, "lgkm_waits": 0, "lgkm0_waits": 0, "barriers": 0, "scratch": 0, "lgkm0_between_writes": 0}
    def flush():
        nonlocal valu
        if valu:
            ev.append("valu x%d" % valu)
            valu = 0
    last_ds = None   # last LDS instruction seen: "w" / "r"; a lgkmcnt(0) wait seen since a write
    wait0_since_write = False
    for l in loop:
        s = l.strip()
        if not s or s.startswith((";", ".")):
            continue
        op = s.split()[0]
        if op.startswith("v_"):
            valu += 1; tot["valu"] += 1
            if op.startswith("v_pk_"): tot["packed"] += 1
            continue
        if op.startswith("ds_"):
            flush()
            kind = "r" if ("read" in op or "load" in op) else "w"
            tot["ds_read" if kind == "r" else "ds_write"] += 1
            if kind == "w":
                if last_ds == "w" and wait0_since_write: tot["lgkm0_between_writes"] += 1
                wait0_since_write = False
            last_ds = kind if kind == "w" or last_ds != "w" else last_ds   # (a read between two writes does not end the write run)
            ev.append(op + (" " + s.split()[1].rstrip(",") if kind == "r" else ""))
        elif op == "s_waitcnt" and "lgkmcnt" in s:
            flush()
            n = int(re.search(r"lgkmcnt\((\d+)\)", s).group(1))
            tot["lgkm_waits"] += 1
            if n == 0:
                tot["lgkm0_waits"] += 1; wait0_since_write = True
            ev.append("WAIT lgkmcnt(%d)" % n)
        elif op.startswith("scratch_"):
            flush(); tot["scratch"] += 1; ev.append(op)
        elif op == "s_barrier":
            flush(); tot["barriers"] += 1; last_ds = None; ev.append("---- s_barrier ----")
    flush()
    print(name, "tile loop: %d lines" % len(loop))
    if not brief:
        run, prev = 0, None   # collapse repeats
        for e in ev + [None]:
            if e == prev: run += 1; continue
            if prev is not None: print("  " + prev + (" (x%d)" % run if run > 1 else ""))
            prev, run = e, 1
    print(" ".join("%s=%d" % kv for kv in tot.items()))

if __name__ == "__main__":
    main()
