"""Timing of the device-resident FEC chain (csrc/convcode.hip around csrc/viterbi.hip): K = 7, rate 1/2 punctured to 3/4 by ('110', '101'),
soft decisions at levels 0 / 7 in the decoder's int16 device format, decision depth 35.

  rows     4096 frames x 16384 bits: encode -> puncture -> (levels) -> depuncture to int16 -> viterbi_decoder_rows -> count
  stream   one row of 2^26 bits: the same stages without the decoder (it is sequential along a stream: a long stream reaches it cut into
           frames, which is the rows shape)

    python tools/time_fecchain.py [rows stream] [--reps K] [--json PATH]

All data stays on the device; per stage, device events around each of K launches after a warm-up, median of the repeats: ms, the bytes
the stage reads plus the bytes it writes over that time in GB/s and as a fraction of the device-copy rate measured in the same run the way
bench.py --full measures it (hipMemcpyAsync device-to-device of 2^28 bytes, bytes read + bytes written), and the stage's share of the
chain's total.  The line "outer" sums the four stages around the decoder.  The levels step (bits -> int16 0 / 7) stands for the caller's
channel and is not timed: it runs on the host once, before the timed stages.  The count of the rows shape must come out as 0 errors (a
check of the data path, not of a time).  One JSON line per stage, stamped with the hashes of the kernels' sources."""
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scikit-dsp-comm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from sk_dsp_comm_amd import _ffi, fec_conv as fc  # noqa: E402
from time_blockcode import device_copy_gbps, median_ms  # noqa: E402

SHAPES = {"rows": (4096, 16384), "stream": (1, 1 << 26)}
G, DEPTH, PATTERN = ('1111001', '1011011'), 35, ('110', '101')


def source_hashes():
    out = {}
    for name in ("convcode.hip", "convcode_core.hpp", "viterbi.hip", "viterbi_core.hpp"):
        with open(os.path.join(ROOT, "scikit-dsp-comm_amd", "csrc", name), "rb") as f:
            out[name] = hashlib.sha256(f.read()).hexdigest()[:16]
    return out


def run_shape(name, nrow, n, reps, copy, stamp):
    cc = fc.FECConv(G, DEPTH)
    enc, vit = cc._encoder(), cc._kernel()
    n_code = 2 * n
    n_sent = _ffi.puncture_out_len(n_code, PATTERN)
    n_back = _ffi.puncture_out_len(n_sent, PATTERN, True)
    n_dec = n_back // 2 - (DEPTH - 1)
    decode = name == "rows"
    rng = np.random.default_rng(12)
    d_bits, d_code, d_sent = _ffi.DeviceBytes(nrow * n), _ffi.DeviceBytes(nrow * n_code), _ffi.DeviceBytes(nrow * n_sent)
    d_soft, d_back = _ffi.DeviceBytes(2 * nrow * n_sent), _ffi.DeviceBytes(2 * nrow * n_back)
    d_dec, d_cnt = _ffi.DeviceBytes(max(nrow * n_dec, 1)), _ffi.DeviceBytes(8 * nrow)
    d_bits.write(rng.integers(0, 2, nrow * n, dtype=np.uint8))
    stages = [
        ("encode", "convenc", lambda: enc.encode_rows_dev(d_bits.ptr, n, nrow, 0, 0, d_code.ptr, 0), nrow * (n + n_code)),
        ("puncture", "puncture", lambda: _ffi.puncture_rows_dev(d_code.ptr, n_code, nrow, 1, PATTERN, d_sent.ptr), nrow * (n_code + n_sent)),
        ("depuncture", "depuncture", lambda: _ffi.depuncture_rows_dev(d_soft.ptr, n_sent, nrow, np.int16, PATTERN, 3.5, d_back.ptr), 2 * nrow * (n_sent + n_back)),
    ]
    if decode:
        stages.append(("decode", "viterbi", lambda: vit.decode_rows_dev(d_back.ptr, n_back, nrow, vit.SOFT, 3, d_dec.ptr), nrow * (2 * n_back + n_dec)))
        stages.append(("count", "bitcount", lambda: _ffi.bit_count_rows_dev(d_bits.ptr, n, d_dec.ptr, n_dec, n_dec, nrow, False, d_cnt.ptr), nrow * (2 * n_dec + 8)))
    else:      # the stream against its own code bits' first stream: a count over n bytes, whatever it finds
        stages.append(("count", "bitcount", lambda: _ffi.bit_count_rows_dev(d_bits.ptr, n, d_code.ptr, n_code, n, nrow, False, d_cnt.ptr), nrow * (2 * n + 8)))
    recs = []
    for stage, engine, launch, nbytes in stages:
        if stage == "depuncture":      # the caller's channel: punctured bits -> int16 levels 0 / 7, on the host, once, untimed
            d_soft.write((7 * d_sent.read().astype(np.int16)).view(np.uint8))
        _ffi.debug_path()
        ms, rounds = median_ms(launch, reps)
        path = sorted(set(_ffi.debug_path()))
        recs.append({"shape": name, "nrow": nrow, "bits_per_row": n, "stage": stage, "ms": round(ms, 4), "bytes": nbytes, "GBps": round(nbytes / ms / 1e6, 1),
                     "device_copy_GBps": round(copy, 1), "frac_of_device_copy": round(nbytes / ms / 1e6 / copy, 3), "source_gbit_s": round(nrow * n / ms / 1e6, 2),
                     "ms_rounds": [round(v, 4) for v in rounds], "path": path, "engine": engine, "source_sha256": stamp})
    total = sum(r["ms"] for r in recs)
    for r in recs:
        r["share_of_chain"] = round(r["ms"] / total, 4)
    outer = sum(r["ms"] for r in recs if r["stage"] != "decode")
    summary = {"shape": name, "nrow": nrow, "bits_per_row": n, "stage": "outer", "ms": round(outer, 4), "chain_ms": round(total, 4),
               "share_of_chain": round(outer / total, 4), "decoder_in_chain": decode, "source_sha256": stamp}
    if decode:
        summary["bit_errors"] = int(d_cnt.read().view(np.int64).sum())
    for d in (d_bits, d_code, d_sent, d_soft, d_back, d_dec, d_cnt):
        d.free()
    return recs + [summary]


def main(argv):
    names = [a for a in argv if a in SHAPES] or list(SHAPES)
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 7
    out_path = argv[argv.index("--json") + 1] if "--json" in argv else None
    _ffi.init(0)
    src, dst = _ffi.DeviceBytes(1 << 28), _ffi.DeviceBytes(1 << 28)
    copy = device_copy_gbps(src.ptr, dst.ptr, 1 << 28)
    src.free()
    dst.free()
    stamp = source_hashes()
    lines = []
    for name in names:
        for rec in run_shape(name, SHAPES[name][0], SHAPES[name][1], reps, copy, stamp):
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
