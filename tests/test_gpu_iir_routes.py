"""The IIR routing decision and its results against the record of the commit that last held the decision spread over csrc/iir_api.hip,
csrc/iir_scan.hip and csrc/iir_par.hip (tests/iir_routes/mi355x.txt, written by tools/record_iir_routes.py; its header names that
commit): every call of the table is made again -- same cascade, same input, same options -- and must return the same code, run the
same engines (skdsp_debug_path) and write the same bytes (zlib.crc32; two recordings of that commit agreed on every row, and a row
whose CRC column holds `-` is compared on code and engines only).  tests/host/iir_route_emul.cpp checks the same table against
csrc/iir_route.hpp on the host.

Every row of up to 3 * 4097 samples is replayed; of the longer rows (the single-pass rule and the 128-sample chunks of the two-pass
scan need millions of samples), the two shortest per signal dtype and engine list, so that a dtype takes seconds."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_iir_routes as rec   # noqa: E402
from sk_dsp_comm_amd import _ffi  # noqa: E402

pytestmark = pytest.mark.gpu

TABLE = os.path.join(ROOT, "tests", "iir_routes", "mi355x.txt")
N_ALL = 3 * 4097
LARGE_PER_ENGINE = 2


def _table():
    with open(TABLE) as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip()]
    header = dict(kv.split("=", 1) for kv in lines[0].lstrip("# ").split())
    return int(header["cus"]), [rec.parse_row(ln) for ln in lines[1:] if not ln.startswith("#")]


def _rows_of(dtype, records):
    """The dtype's rows to replay: all up to N_ALL samples, and per engine list the LARGE_PER_ENGINE shortest of the longer ones."""
    mine = [r for r in records if r[0][0] == dtype]
    keep = [r for r in mine if r[0][4] <= N_ALL]
    large = {}
    for r in mine:
        if r[0][4] > N_ALL:
            large.setdefault(",".join(r[2]), []).append(r)
    for same in large.values():
        same.sort(key=lambda r: r[0][4])
        keep += same[:LARGE_PER_ENGINE]
    return keep


@pytest.mark.parametrize("dtype", rec.DTYPES, ids=rec.DTYPE_NAMES)
def test_iir_calls_run_the_recorded_engines_and_write_the_recorded_bytes(dtype):
    cus, records = _table()
    _ffi.init()
    have = _ffi.device_info()["compute_units"]
    if have != cus:
        pytest.skip("the table was recorded on %d compute units (the single-pass rule reads the count); this device has %d" % (cus, have))
    records = _rows_of(dtype, records)
    assert records, "no rows of this dtype in %s" % TABLE
    run = rec.Runner([r[0] for r in records])
    wrong = []
    for row, rc, engines, crc in records:
        got_rc, got_engines, got_crc = run.run_row(row)
        if got_rc != rc or got_engines != engines or (rc == 0 and crc is not None and got_crc != crc):
            wrong.append("%s: now %s" % (rec.format_row(row, rc, engines, crc), rec.format_row(row, got_rc, got_engines, got_crc).split(" ", 6)[6]))
    assert not wrong, "%d of %d rows differ from the record:\n%s" % (len(wrong), len(records), "\n".join(wrong[:40]))
