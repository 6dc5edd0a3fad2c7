#!/usr/bin/env python
"""Answers of the three host queries of the 1x1 convolutions over one grid of launch shapes, as JSON.

    python tools/conv1x1_host_grid.py path/to/libaid_hip.so COMMIT out.json

tests/golden/conv1x1_host_grid.json is this script's output for the library of the commit named in its "commit" field;
tests/test_host_logic.py recomputes every row from the library under test.  (Pure host functions: no GPU.)

A row is one (Cin, Cout, F) with the answers for every T of TS: aid_conv2d_pack_dims once, aid_conv2d_dot_partials_1x1 per T, and per T the
answers of aid_conv2d_x2_supported for the six Cin1 of cin1s(Cin) as bits (bit i: Cin1 = cin1s(Cin)[i]).
"""
import ctypes
import json
import sys

from wino_r_host_grid import LEVELS

B = 4                                                    # the queries answer per sample: one batch
TS = (8, 12, 16, 32, 48, 64, 96, 128, 256, 512, 1024, 2048)
FS = tuple(dict.fromkeys((1, 2, 6, 9, 16) + tuple(F for _, F, _, _ in LEVELS)))
COUTS = (32, 40, 64, 96, 128, 192, 256, 288)
CINS = (16, 32, 40, 64, 96, 128, 144, 192, 256, 352, 512)
COLUMNS = ["Cin", "Cout", "F", "Cin_pad", "Cout_pad", "dot_partials_1x1[T in TS]", "x2_supported[T in TS], bit i: Cin1 = cin1s(Cin)[i]"]


def cin1s(cin):
    return (16, 64, cin // 2, cin - 16, cin, 24)


def shapes():
    """(Cin, Cout, F) of the grid, in a fixed order, without repeats: the network's own 1x1 layers (channels C, 2C, 8, 2 at each level's F), then
    every Cin x Cout x F of the lists above."""
    out = [(ci, co, F) for C, F, _, _ in LEVELS for ci in (C, 2 * C, 8, 2) for co in (C, 2 * C, 8, 2)]
    out += [(ci, co, F) for ci in CINS for co in COUTS for F in FS]
    return list(dict.fromkeys(out))


def row(L, cin, cout, F):
    cip, cop = ctypes.c_int(0), ctypes.c_int(0)
    L.aid_conv2d_pack_dims(cin, cout, ctypes.byref(cip), ctypes.byref(cop))
    return [cin, cout, F, cip.value, cop.value, [L.aid_conv2d_dot_partials_1x1(B, cin, cout, F, T) for T in TS],
            [sum(L.aid_conv2d_x2_supported(cin, c1, cout, F, T) << i for i, c1 in enumerate(cin1s(cin))) for T in TS]]


def table(L):
    return [row(L, *s) for s in shapes()]


if __name__ == "__main__":
    lib, commit, out = sys.argv[1:4]
    rows = table(ctypes.CDLL(lib))
    with open(out, "w") as f:
        f.write('{"commit": %s,\n "B": %d,\n "TS": %s,\n "columns": %s,\n "rows": [\n' % (json.dumps(commit), B, json.dumps(list(TS)), json.dumps(COLUMNS)))
        f.write(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n ]}\n")
    print(len(rows), "rows x", len(TS), "T ->", out)
