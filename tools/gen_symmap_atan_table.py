#!/usr/bin/env python3
"""Prints the double-double constants of csrc/symmap_core.hpp's atan2_rn: k pi / 16, cos and sin of it for k = 0 ... 4, pi / 2 and pi, each as
(hi, lo) with hi = the nearest float64 and lo = the nearest float64 of the rest (mpmath, 60 digits), and the octant thresholds tan((2k + 1) pi / 32).

    python tools/gen_symmap_atan_table.py
"""
import mpmath as mp

mp.mp.dps = 60


def dd(v):
    hi = float(v)
    lo = float(v - mp.mpf(hi))
    return "%s, %s" % (hi.hex(), lo.hex())


for k in range(5):
    a = k * mp.pi / 16
    print("    {%s, %s, %s}," % (dd(a), dd(mp.cos(a)), dd(mp.sin(a))))
print("pio2: %s" % dd(mp.pi / 2))
print("pi:   %s" % dd(mp.pi))
print("tan thresholds: " + ", ".join(float(mp.tan((2 * k + 1) * mp.pi / 32)).hex() for k in range(4)))
