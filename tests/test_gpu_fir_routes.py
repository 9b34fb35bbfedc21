"""The FIR routing decision and its results against the record of the commit that last held the decision inside csrc/fir_api.hip
(tests/fir_routes/mi355x.txt, written by tools/record_fir_routes.py; its header names that commit): every call of the table is made
again -- same taps, same input, same options -- and must return the same code, run the same engines (skdsp_debug_path) and write
the same bytes (zlib.crc32; the FIR engines have no data-dependent summation order).  tests/host/fir_route_emul.cpp checks the
same table against csrc/fir_route.hpp on the host.  The CRCs of the rows that run fir_ols64 / fir_ols64_up were recorded again, by the same
run_row, when those kernels' twiddle powers changed (csrc/fir_ols64.hip: twiddle_powers); their return codes and engines are the first record's.

Every row up to 2^17 + 3 samples is replayed; of the rows with 2^25 outputs (the cost model's rounds term needs them), the two
smallest per signal class and engine list, so that a class takes seconds."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_fir_routes as rec   # noqa: E402
from sk_dsp_comm_amd import _ffi  # noqa: E402

pytestmark = pytest.mark.gpu

TABLE = os.path.join(ROOT, "tests", "fir_routes", "mi355x.txt")
LARGE_PER_ENGINE = 2


def _table():
    with open(TABLE) as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip()]
    header = dict(kv.split("=", 1) for kv in lines[0].lstrip("# ").split())
    return int(header["cus"]), [rec.parse_row(ln) for ln in lines[1:]]


def _rows_of(cls, records):
    """The class's rows to replay: all up to N_MID samples, and per engine list the LARGE_PER_ENGINE cheapest of the longer ones."""
    mine = [r for r in records if (r[0][0], r[0][1]) == cls]
    keep = [r for r in mine if r[0][6] <= rec.N_MID]
    large = {}
    for r in mine:
        if r[0][6] > rec.N_MID:
            large.setdefault(",".join(r[2]), []).append(r)
    for same in large.values():
        same.sort(key=lambda r: r[0][6] + rec.n_out_of(r[0][4], r[0][5], r[0][6]))
        keep += same[:LARGE_PER_ENGINE]
    return keep


@pytest.mark.parametrize("cls", rec.CLASSES, ids=rec.CLASS_NAMES)
def test_fir_calls_run_the_recorded_engines_and_write_the_recorded_bytes(cls):
    cus, records = _table()
    _ffi.init()
    have = _ffi.device_info()["compute_units"]
    if have != cus:
        pytest.skip("the table was recorded on %d compute units (the cost model reads the count); this device has %d" % (cus, have))
    records = _rows_of(cls, records)
    assert records, "no rows of this class in %s" % TABLE
    run = rec.runner_for([r[0] for r in records])
    wrong = []
    for row, rc, engines, crc in records:
        got_rc, got_engines, got_crc = run.run_row(row)
        if got_rc != rc or got_engines != engines or (rc == 0 and crc is not None and got_crc != crc):
            wrong.append("%s: now %s" % (rec.format_row(row, rc, engines, crc), rec.format_row(row, got_rc, got_engines, got_crc).split(" ", 10)[10]))
    assert not wrong, "%d of %d rows differ from the record:\n%s" % (len(wrong), len(records), "\n".join(wrong[:40]))
