"""What factors would an end-to-end float32-grade criterion need?  Prints K_rms and K_max (tests/block_accuracy_cases.py: chain_K) of every plan of the
block-kernel accuracy cases — CPU only, about two minutes — and the totals.  README.md in this directory holds the figures of the last run.

    python profiles/accuracy/chain_factors.py [floor in ulps, default 1]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for d in ("tests", "oracle", ""):
    sys.path.insert(0, os.path.join(ROOT, d))

import block_accuracy_cases as BC          # noqa: E402
import oracle as O                         # noqa: E402


def main():
    floor = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    O.build()
    top = [0.0, "", 0.0, ""]
    for case in BC.all_cases():
        k = BC.chain_K(case, O, floor)
        print("CHAIN_K %-40s K_rms=%.3f K_max=%.3f" % (case.id, k[0], k[2]), flush=True)
        for i in (0, 2):
            if k[i] > top[i]:
                top[i], top[i + 1] = k[i], k[i + 1]
    print("TOTAL floor=%g ulp  K_rms=%.3f [%s]  K_max=%.3f [%s]" % (floor, top[0], top[1], top[2], top[3]))
    print("twice K, rounded up to the next half: %.1f and %.1f" % (-(-4 * top[0] // 1) / 2, -(-4 * top[2] // 1) / 2))


if __name__ == "__main__":
    main()
