#!/usr/bin/env python3
"""The offline search behind the constants of tests/jpeg_encode_cases.py (DIRECTED and NOISE_688): CPU only, some ten seconds.

    python tools/search_jpeg_encode_cases.py [--tries N]

For every layout and kind of table it re-draws the +-3 noise of the directed last MCU until the eight 1 bits of coefficient 63 fall on
a byte ('0xFF last whole byte of a batch' for kind 'seam', 'unpadded last byte is 0xFF' for kind 'end'), and it picks 688 wide noise rows
that reach the three regimes white noise does reach.  It prints the constants and how many inputs each took."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import jpeg_encode_cases as JC            # noqa: E402
from tests.test_gpu_jpeg_encode import noise          # noqa: E402

TARGET = {"seam": "0xFF last whole byte of a batch", "end": "unpadded last byte is 0xFF"}
BY_NOISE = ("batch ends on a byte", "0xFF completed from carried bits", "padded last byte is 0xFF")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tries", type=int, default=20000)
    ap.add_argument("--amp", type=int, default=39)
    a = ap.parse_args()
    for layout in ("444", "420"):
        h = 16 if layout == "420" else 8
        base = noise(688, h, seed=21)
        for kind, target in TARGET.items():
            for tables in ("std", "optimal"):
                for seed in range(a.tries):
                    if target in JC.regimes(JC.directed(base, layout, kind, a.amp, seed), 100, layout, tables):
                        print('    ("%s", "%s", "%s", %d, %d),      # input %d of the search' % (layout, tables, kind, a.amp, seed, seed + 1), flush=True)
                        break
                    JC._coded.clear()
                else:
                    print("# %s %s %s: not reached in %d inputs" % (layout, tables, kind, a.tries), flush=True)
        need = {(t, r) for t in ("std", "optimal") for r in BY_NOISE}
        seeds = []
        for seed in range(a.tries):
            if not need:
                break
            c = noise(688, h, seed=seed)
            got = {(t, r) for t in ("std", "optimal") for r in JC.regimes(c, 100, layout, t)} & need
            JC._coded.clear()
            if got:
                seeds.append(seed)
                need -= got
        print('NOISE_688 "%s": %r      # missing: %r' % (layout, tuple(seeds), sorted(need)), flush=True)


if __name__ == "__main__":
    main()
