#!/usr/bin/env python3
"""Regenerates the sRGB encode thresholds of the colour contract (include/imagestitch.h, "colour profiles"):
    T[c] = ceil(65535 * s((c - 0.5) / 255)),  c = 1 .. 255,   s(x) = x / 12.92 for x <= 0.04045, else ((x + 0.055) / 1.055) ** 2.4
The output code of a linear value o in 0 .. 65535 is the number of c with T[c] <= o.  Prints the literal that
imagestitching_amd/csrc/ist_icc.h and tests/icc_reference.py carry (T[0] = 0 is a placeholder), and checks the property the
kernel's coarse table rests on: no two thresholds fall into one bucket of 16 linear values.

    python tools/gen_icc_encode_table.py
"""
import math


def srgb_to_linear(x):
    return x / 12.92 if x <= 0.04045 else math.pow((x + 0.055) / 1.055, 2.4)


def thresholds():
    return [0] + [int(math.ceil(65535.0 * srgb_to_linear((c - 0.5) / 255.0))) for c in range(1, 256)]


def main():
    t = thresholds()
    assert all(b > a for a, b in zip(t[1:], t[2:])) and t[1] > 0 and t[255] <= 65535
    assert len({v >> 4 for v in t[1:]}) == 255, "two thresholds share a bucket of 16"
    print("// narrowest step: %d" % min(b - a for a, b in zip(t[1:], t[2:])))
    for i in range(0, 256, 16):
        print("  " + ", ".join("%5d" % v for v in t[i:i + 16]) + ",")


if __name__ == "__main__":
    main()
