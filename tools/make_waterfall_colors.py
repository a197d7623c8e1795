"""Writes tests/golden/waterfall_colors.npz: the four colour schemes of FDC.WaterfallMsgTagging (python/WaterfallMsgTagging.py:276-312,
cr_colorscheme) and their frame colours, built as the scheme definitions specify them: numpy.linspace(a, b, n, dtype=uint8) pieces
(float64 points truncated to uint8), constant pieces, channels R, G, B of 1024 colours.  Run once; the fixture is committed.

    python tools/make_waterfall_colors.py [out.npz]
"""
import os
import sys

import numpy as np

N = 1024


def lsp(a, b, n):
    return np.linspace(a, b, n, dtype=np.uint8)


def const(v, n):
    return np.full(n, v, np.uint8)


def scheme(k):
    q, h = N // 4, N // 2
    if k == 1:      # black-rainbow
        r = np.concatenate((lsp(0, 75, q), lsp(75, 0, q), const(0, q), lsp(0, 255, q)))
        g = np.concatenate((const(0, q), const(0, q), lsp(0, 255, q), const(255, q)))
        b = np.concatenate((lsp(0, 130, q), lsp(130, 255, q), lsp(255, 0, q), const(0, q)))
        frame = (255, 255, 255)
    elif k == 2:    # black-red-yellow
        r = np.concatenate((lsp(0, 255, h), const(255, h)))
        g = np.concatenate((const(0, h), lsp(0, 255, h)))
        b = const(0, N)
        frame = (255, 255, 255)
    elif k == 3:    # black-white
        r = g = b = lsp(0, 255, N)
        frame = (0, 255, 0)
    else:           # black-blue-cyan-white
        r = const(0, N)
        g = np.concatenate((const(0, h), lsp(0, 255, h)))
        b = np.concatenate((lsp(0, 255, h), const(255, h)))
        frame = (255, 255, 255)
    return np.stack([r, g, b], axis=1).astype(np.uint8), np.array(frame, np.uint8)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden",
                                                             "waterfall_colors.npz")
    arrs = {}
    for k in range(4):
        arrs["cols%d" % k], arrs["frame%d" % k] = scheme(k)
    np.savez_compressed(out, **arrs)
    print("wrote", os.path.normpath(out))


if __name__ == "__main__":
    main()
