#!/usr/bin/env python
"""Answers of the seven host queries of the row-shared Winograd kernels over one grid of launch shapes, as JSON.

    python tools/wino_r_host_grid.py path/to/libaid_hip.so COMMIT out.json

tests/golden/wino_r_host_grid.json is this script's output for the library of the commit named in its "commit" field;
tests/test_host_logic.py recomputes every row from the library under test.  (Pure host functions: no GPU.)
"""
import ctypes
import json
import sys

LEVELS = [(64, 64, 2048, 2), (96, 128, 1024, 3), (96, 192, 512, 4), (128, 256, 256, 5), (128, 320, 128, 6), (256, 384, 64, 7), (256, 448, 32, 7)]
BATCHES = (1, 2, 3, 4, 8)
COLUMNS = ["B", "Cin", "Cout", "F", "T", "dilF", "wino_form", "wino8_supported", "wino_input_ok", "wino_split_ws_bytes",
           "fin_supported[x_wino=0,1,2]", "stat_partials[x_wino=0,1,2]", "dot_partials[x_wino=0,1,2]"]


def shapes():
    """(Cin, Cout, F, T, dilF) of the grid, in a fixed order, without repeats."""
    out = []
    for C, F, T, nd in LEVELS:
        for k in range(nd):
            out.append((C, C, F, T, 1 << k))
            out += [(C, C, F, t, 1 << k) for t in (16, 32, 48, 96)]
            if k:
                out.append((C, C, F + 1, T, 1 << k))                        # F not divisible by the dilation
    for cout in (2, 64, 96, 128, 192, 256):
        for cin in (2, 62, 64):
            out += [(cin, cout, 64, 1024, 1), (cin, cout, 448, 32, 4), (cin, cout, 56, 64, 2), (cin, cout, 112, 16, 8)]
    # the declining shapes test_winograd_form_choice_is_a_function_of_the_launch_shape names
    out += [(256, 256, 384, 64, 64), (256, 256, 64, 16, 1), (2, 64, 64, 1024, 1), (64, 2, 64, 1024, 1), (96, 96, 20, 256, 4), (128, 128, 320, 128, 1), (128, 128, 256, 256, 2)]
    return list(dict.fromkeys(out))


def bind(path):
    L = ctypes.CDLL(path)
    L.aid_conv2d_wino_split_ws_bytes.restype = ctypes.c_int64
    return L


def row(L, B, cin, cout, F, T, d):
    return [B, cin, cout, F, T, d, L.aid_conv2d_wino_form(B, cin, cout, F, T, d), L.aid_conv2d_wino8_supported(cin, cout, F, T, d),
            L.aid_conv2d_wino_input_ok(B, cin, cout, F, T, d), L.aid_conv2d_wino_split_ws_bytes(B, cin, cout, F, T, d),
            [L.aid_conv2d_fin_supported(B, cin, cout, F, T, d, x) for x in (0, 1, 2)],
            [L.aid_conv2d_stat_partials(B, cin, cout, F, T, d, x) for x in (0, 1, 2)],
            [L.aid_conv2d_dot_partials(B, cin, cout, F, T, d, x) for x in (0, 1, 2)]]


def table(L):
    return [row(L, B, *s) for s in shapes() for B in BATCHES]


if __name__ == "__main__":
    lib, commit, out = sys.argv[1:4]
    rows = table(bind(lib))
    with open(out, "w") as f:
        f.write('{"commit": %s,\n "columns": %s,\n "rows": [\n' % (json.dumps(commit), json.dumps(COLUMNS)))
        f.write(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n ]}\n")
    print(len(rows), "rows ->", out)
