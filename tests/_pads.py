"""Pad values for the device memory in front of and behind an input window (tests/test_gpu_input_footprint.py, tests/test_gpu_fuzz.py)."""
import numpy as np


def loud(count, dt, first=0):
    """`count` elements of `dt` for positions first .. first + count - 1 of a buffer: finite, ~2^20 (2^19 .. 1.5 x 2^20), sign and
    magnitude varying from element to element, in both parts of a complex sample; no RNG draws.  A call reads its own window only, so
    they must not show in any result; zeros there would hide a loader that reads past its window."""
    def part(idx):
        mag = 2.0 ** 20 * (0.5 + ((idx * 37) % 101) / 101.0)
        return np.where((idx * 7 + idx // 5) % 3 == 0, -mag, mag)
    idx = np.arange(first, first + count, dtype=np.int64)
    v = part(idx)
    if np.dtype(dt).kind == "c":
        v = v - 1j * part(idx + 53)
    return v.astype(dt)
