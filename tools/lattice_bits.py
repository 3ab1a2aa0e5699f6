#!/usr/bin/env python3
"""Bit lengths of the lattice-reduced scalar pairs (c0, c1) for random
challenges k < l, per item and per 64-lane wave (the largest of the wave's
128 scalars sets how many Straus windows the wave runs: csrc/hsv_verify_hc.hpp
straus_vt).  Uses the host build of the kernel core (tests/native/core_host,
built by tests/test_kernel_host.py into build/core_host).

Then the 2-bit columns of the joint point pass (straus_joint): columns per
item, cols = max(cols(|c0|), cols(c1)), and the mean columns a 64-lane wave
runs (its largest item's), for the symmetric digits {-2 .. 1} and for the
record's {-1 .. 2} (recode_cols), in index order and, for the latter, dealt:
64-item batches cut from the items sorted by clamped column count, longest
first, as hsv_verify_hp_kernel takes them from the class lists.

python tools/lattice_bits.py [N [BOUND_BITS]]      (BOUND_BITS: 133; the comb path's is 138)
"""
import collections
import os
import random
import subprocess
import sys

L = 2**252 + 27742317777372353535851937790883648493
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cols(c, reach):
    """Columns of 2 bits a scalar needs when m columns reach reach(m):
    4^m / 3 for digits in {-2 .. 1}, 2 * 4^m / 3 for {-1 .. 2}."""
    m = 0
    while not reach(c, m):
        m += 1
    return m


def sym(c, m):      # chunk - 2: c + 2 (4^m - 1) / 3 < 4^m
    return 3 * c < 4 ** m + 2


def pos(c, m):      # chunk - 1: c + (4^m - 1) / 3 < 4^m
    return 3 * c < 2 * 4 ** m + 1


def column_report(pairs):
    def waves(need):
        w = [max(need[i:i + 64]) for i in range(0, len(need) - 63, 64)]
        return sum(w) / len(w), collections.Counter(w)
    for name, reach in (("digits {-2..1}", sym), ("digits {-1..2}", pos)):
        need = [max(cols(c0, reach), cols(c1, reach)) for c0, c1 in pairs]
        hist = collections.Counter(need)
        mean, wh = waves(need)
        print(f"{name}: columns per item ->",
              {k: "%.1f%%" % (100.0 * v / len(need)) for k, v in sorted(hist.items())})
        print(f"{name}: index order, mean columns a wave runs %.2f" % mean,
              {k: "%.0f%%" % (100.0 * v / sum(wh.values())) for k, v in sorted(wh.items())})
        if reach is pos:
            dealt = sorted((min(max(x, 62), 67) for x in need), reverse=True)
            # a batch runs its largest item's true count; within a clamped class the counts are equal
            # except above 67 and below 62, where the wave-uniform skip still finds the true one
            true = sorted(need, reverse=True)
            print(f"{name}: dealt by class (62 .. 67), mean columns a wave runs %.2f" % waves(true)[0],
                  "classes ->", dict(sorted(collections.Counter(dealt).items())))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
    bound = sys.argv[2:3]
    rnd = random.Random(3)
    ks = [rnd.randrange(L) for _ in range(n)]
    out = subprocess.run([os.path.join(ROOT, "build", "core_host"), "--lattice"] + bound,
                         input="\n".join(f"{k:064x}" for k in ks) + "\n",
                         capture_output=True, text=True, check=True).stdout.split()
    per_item, bits, pairs = collections.Counter(), [], []
    for i in range(n):
        ok, c0, c1 = int(out[4 * i]), int(out[4 * i + 2], 16), int(out[4 * i + 3], 16)
        if not ok:
            per_item["fallback"] += 1
            continue
        b = max(c0.bit_length(), c1.bit_length())
        per_item[b] += 1
        bits.append(b)
        pairs.append((c0, c1))
    print("items: max(bits(c0), bits(c1)) ->", dict(sorted((k, v) for k, v in per_item.items() if k != "fallback")),
          "fallback:", per_item["fallback"])
    waves = collections.Counter(max(bits[i:i + 64]) for i in range(0, len(bits) - 63, 64))
    tot = sum(waves.values())
    print("waves of 64: largest bit length ->", dict(sorted(waves.items())))
    print("share of waves with every scalar < 2^131 (top 4-bit window zero): %.3f"
          % (sum(v for k, v in waves.items() if k <= 131) / tot))
    column_report(pairs)


if __name__ == "__main__":
    main()
