"""Timing of the block-code kernels (csrc/blockcode.hip) on 2^28 code bits (one byte each) per call:

  H3 H7 H10 H13 H16   FECHamming(j): decode_dev and encode_dev -- the lane form (j = 3), the wave form (7, 10), the group form (13, 16)
  C7                  FECCyclic('10100001'): decode_dev (the same kernel over other tables)

    python tools/time_blockcode.py [H3 H7 H10 H13 H16 C7] [--reps K] [--json PATH]

Per workload, device events around each of K launches after a warm-up, median of the repeats: ms, decoded (encoded: source) Gbit/s,
and the stream's bytes (n + k per block) over the time, in GB/s and as a fraction of the device-copy rate measured in the same run the
way bench.py --full measures it (hipMemcpyAsync device-to-device of 2^28 bytes, bytes read + bytes written).  The kernels move bytes
and do little else, so the copy is the yardstick, not the HBM peak.  Beside them the reference's own rate for that code where
tests/golden/g20_conventions.json recorded one (one CPU core).  The bits are uniform noise: the work per block does not depend on
them.  One JSON line per workload, stamped with the hashes of the kernel's sources."""
import ctypes
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scikit-dsp-comm_amd"))

import numpy as np  # noqa: E402

from sk_dsp_comm_amd import _ffi, fec_block as fb  # noqa: E402

WORKLOADS = {"H3": 3, "H7": 7, "H10": 10, "H13": 13, "H16": 16, "C7": '10100001'}
CODE_BITS = 1 << 28


def source_hashes():
    out = {}
    for name in ("blockcode.hip", "blockcode_core.hpp"):
        with open(os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc", name), "rb") as f:
            out[name] = hashlib.sha256(f.read()).hexdigest()[:16]
    return out


def median_ms(launch, reps):
    launch()
    _ffi.sync()
    ms = []
    for _ in range(reps):
        _ffi.timer_start()
        launch()
        ms.append(_ffi.timer_stop())
    return statistics.median(ms), ms


def device_copy_gbps(src, dst, nbytes, reps=20):
    cp = _ffi.load().skdsp_memcpy_d2d
    for _ in range(5):
        _ffi.check(cp(ctypes.c_void_p(dst), ctypes.c_void_p(src), nbytes))
    _ffi.sync()
    _ffi.timer_start()
    for _ in range(reps):
        _ffi.check(cp(ctypes.c_void_p(dst), ctypes.c_void_p(src), nbytes))
    return 2 * nbytes / (_ffi.timer_stop() / reps) / 1e6


def main(argv):
    names = [a for a in argv if a in WORKLOADS] or list(WORKLOADS)
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 7
    out_path = argv[argv.index("--json") + 1] if "--json" in argv else None
    with open(os.path.join(ROOT, "tests", "golden", "g20_conventions.json")) as f:
        ref_rate = json.load(f)["ref_bits_per_s"]
    _ffi.init(0)
    rng = np.random.default_rng(11)
    bits = rng.integers(0, 2, CODE_BITS, dtype=np.uint8)
    din, dout = _ffi.DeviceBytes(CODE_BITS), _ffi.DeviceBytes(CODE_BITS)
    din.write(bits)
    copy = device_copy_gbps(din.ptr, dout.ptr, CODE_BITS)
    stamp = source_hashes()
    lines = []
    for name in names:
        spec = WORKLOADS[name]
        code = fb.FECHamming(spec) if isinstance(spec, int) else fb.FECCyclic(spec)
        kern = code._kernel()
        nblocks = CODE_BITS // code.n
        calls = [("decode", lambda: kern.decode_dev(din.ptr, nblocks, dout.ptr))]
        if isinstance(spec, int):
            calls.append(("encode", lambda: kern.encode_dev(din.ptr, nblocks, dout.ptr)))
        for fn, launch in calls:
            _ffi.debug_path()
            ms, rounds = median_ms(launch, reps)
            path = sorted(set(_ffi.debug_path()))
            stream_bytes = (code.n + code.k) * nblocks
            key = ("ham%d" % spec) if isinstance(spec, int) else "cyc" + spec
            rec = {"workload": name, "fn": fn, "j": code.j, "n": code.n, "k": code.k, "nblocks": nblocks, "ms": round(ms, 4),
                   "source_gbit_s": round(code.k * nblocks / ms / 1e6, 2), "stream_GBps": round(stream_bytes / ms / 1e6, 1),
                   "device_copy_GBps": round(copy, 1), "frac_of_device_copy": round(stream_bytes / ms / 1e6 / copy, 3),
                   "ref_bits_per_s": ref_rate.get(key) if fn == "decode" else None, "ms_rounds": [round(v, 4) for v in rounds], "path": path,
                   "source_sha256": stamp}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del kern, code
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
