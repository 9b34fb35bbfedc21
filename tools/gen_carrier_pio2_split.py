#!/usr/bin/env python3
"""The three-word split of pi / 2 that csrc/carrier_core.hpp's sincos_rad reduces its argument with (Cody and Waite): P1 and P2 carry 49 bits each, so
k P1 and k P2 are exact for every multiple k <= 16, P3 is the rest rounded to a double.  Printed as C hex-float literals; exact rational arithmetic
on a 60-digit value of pi, no dependencies."""
from fractions import Fraction

PI = Fraction("3.14159265358979323846264338327950288419716939937510582097494")


def chop(v, bits):
    """v truncated to `bits` significant bits, as a Fraction"""
    e = 0
    while v >= 2 ** (e + 1):
        e += 1
    while v < 2 ** e:
        e -= 1
    q = Fraction(2) ** (e - bits + 1)
    return (v // q) * q


def main():
    v = PI / 2
    p1 = chop(v, 49)
    p2 = chop(v - p1, 49)
    p3 = float(v - p1 - p2)
    for name, w in (("P1", float(p1)), ("P2", float(p2)), ("P3", p3)):
        assert name == "P3" or Fraction(w) == (p1 if name == "P1" else p2)
        print("%s = %s" % (name, w.hex()))
    print("2/pi = %s" % float(1 / v).hex())
    print("residual = %.3e" % float(v - p1 - p2 - Fraction(p3)))


if __name__ == "__main__":
    main()
