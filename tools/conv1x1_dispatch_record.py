#!/usr/bin/env python
"""Which kernel aid_conv2d notes (aid_last_kernel) for a list of small 1x1 launches, as JSON.  Needs one MI355X.

    python tools/conv1x1_dispatch_record.py COMMIT out.json        (AID_EXPERIMENT=1 AID_LIB_PATH=... selects the library of COMMIT)

tests/golden/conv1x1_dispatch.json is this script's output for the library of the commit named in its "commit" field;
tests/test_gpu_kernels.py::test_conv1x1_dispatch_is_as_recorded launches every case again and compares.  The launch itself is the test's (_c11_launch).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = ["B", "Cin", "Cout", "F", "T", "act", "in_scale", "epi", "res", "dot", "Cin1", "ws", "kernel", "what the case is for"]
CASES = [
    # register-streamed kernel: the three instances, every option key (act 8 | in_scale 4 | epi 2 | res 1) it has, and one it has not
    (1, 96, 96, 6, 32, 0, 0, 0, 0, 0, 0, 0, "rs <3,128>, key 0; a tile spans two rows"),
    (2, 256, 96, 2, 96, 0, 0, 0, 1, 0, 0, 0, "rs <3,256>, key 1"),
    (2, 64, 64, 8, 64, 0, 0, 1, 0, 1, 0, 0, "rs <2,128>, key 2, dot partials"),
    (1, 96, 96, 6, 32, 0, 0, 1, 1, 0, 0, 0, "rs key 3"),
    (2, 64, 64, 8, 64, 0, 1, 0, 0, 0, 0, 0, "rs key 4"),
    (1, 128, 96, 4, 48, 0, 1, 0, 1, 0, 0, 0, "rs key 5, T not a power of two"),
    (1, 96, 96, 6, 32, 0, 1, 1, 0, 1, 0, 0, "rs key 6, dot partials"),
    (2, 64, 64, 8, 64, 1, 1, 0, 0, 0, 0, 0, "rs key 12"),
    (2, 256, 96, 2, 96, 1, 1, 0, 1, 0, 0, 0, "rs key 13"),
    (1, 96, 96, 6, 32, 1, 1, 1, 0, 0, 0, 0, "key 14 has no rs instance: tiled 96-row tile"),
    (2, 64, 64, 8, 64, 0, 1, 0, 1, 0, 0, 0, "rs <2,128>, key 5"),
    (2, 64, 64, 8, 64, 1, 1, 0, 1, 0, 0, 0, "rs <2,128>, key 13"),
    (1, 96, 96, 6, 32, 0, 0, 0, 1, 0, 0, 0, "rs <3,128>, key 1"),
    (1, 96, 96, 6, 32, 0, 0, 1, 0, 1, 0, 0, "rs <3,128>, key 2, dot partials"),
    (2, 256, 96, 2, 96, 0, 0, 0, 0, 0, 0, 0, "rs <3,256>, key 0"),
    (2, 256, 96, 2, 96, 0, 1, 0, 1, 0, 0, 0, "rs <3,256>, key 5"),
    (1, 192, 96, 4, 32, 0, 0, 0, 1, 0, 64, 0, "rs with the K axis in two tensors"),
    (2, 64, 64, 8, 64, 0, 0, 0, 0, 0, 0, 0, "rs <2,128>, key 0"),
    (2, 64, 64, 8, 64, 0, 0, 0, 1, 0, 0, 0, "rs <2,128>, key 1"),
    (2, 64, 64, 8, 64, 0, 0, 1, 1, 0, 0, 0, "rs <2,128>, key 3"),
    (2, 64, 64, 8, 64, 0, 1, 1, 0, 0, 0, 0, "rs <2,128>, key 6"),
    (1, 96, 96, 6, 32, 0, 1, 0, 0, 0, 0, 0, "rs <3,128>, key 4"),
    (1, 96, 96, 6, 32, 1, 1, 0, 0, 0, 0, 0, "rs <3,128>, key 12"),
    (1, 96, 96, 6, 32, 1, 1, 0, 1, 0, 0, 0, "rs <3,128>, key 13"),
    (2, 256, 96, 2, 96, 0, 0, 1, 0, 0, 0, 0, "rs <3,256>, key 2"),
    (2, 256, 96, 2, 96, 0, 0, 1, 1, 0, 0, 0, "rs <3,256>, key 3"),
    (2, 256, 96, 2, 96, 0, 1, 0, 0, 0, 0, 0, "rs <3,256>, key 4"),
    (2, 256, 96, 2, 96, 0, 1, 1, 0, 0, 0, 0, "rs <3,256>, key 6"),
    (2, 256, 96, 2, 96, 1, 1, 0, 0, 0, 0, 0, "rs <3,256>, key 12"),
    # direct-to-LDS tiles
    (2, 128, 128, 8, 64, 0, 0, 0, 1, 0, 0, 0, "dma 128-wide"),
    (2, 128, 128, 8, 64, 0, 0, 1, 0, 1, 0, 0, "dma 128-wide, dot partials"),
    (2, 128, 64, 8, 64, 0, 0, 0, 0, 0, 0, 0, "dma 64-wide (64 output channels, K > 64)"),
    (1, 256, 192, 8, 128, 0, 1, 0, 1, 0, 0, 0, "dma 64-wide, Cout 192 = three tiles, in_scale"),
    (2, 288, 96, 16, 64, 0, 0, 0, 1, 0, 0, 0, "dma 96-wide (K > 256)"),
    (1, 48, 96, 4, 64, 0, 0, 0, 0, 0, 16, 0, "dma 96-wide with the K axis in two tensors (K % 32 != 0)"),
    (2, 128, 128, 16, 16, 0, 1, 0, 0, 0, 0, 0, "dma ROWS = 16 with in_scale, F % 16 == 0"),
    (4, 64, 128, 40, 16, 0, 1, 0, 0, 0, 0, 0, "dma ROWS = 16 with in_scale, F % 16 != 0: declined to the streaming kernel <2,4>"),
    (2, 128, 128, 8, 16, 0, 1, 0, 0, 0, 0, 0, "... and with K > 96 to the tiled kernel"),
    # qk GEMMs (F = 1), K = 512 / 768
    (1, 512, 1024, 1, 32, 0, 0, 0, 1, 0, 0, 1, "skinny nt = 1"),
    (1, 512, 1024, 1, 64, 0, 0, 0, 0, 0, 0, 1, "skinny nt = 2"),
    (3, 512, 640, 1, 32, 0, 0, 0, 1, 0, 0, 1, "skinny nt = 3"),
    (2, 512, 1024, 1, 64, 0, 0, 0, 0, 0, 0, 1, "skinny nt = 4"),
    (4, 768, 384, 1, 64, 0, 0, 0, 1, 0, 0, 1, "dma GEMM + split-K"),
    (4, 768, 384, 1, 64, 0, 0, 0, 1, 0, 0, 0, "the same without scratch: single pass"),
    # streaming kernel (K % 16 != 0)
    (2, 40, 64, 8, 128, 0, 0, 0, 1, 0, 0, 0, "stream <2,4>"),
    (2, 40, 96, 8, 128, 0, 1, 0, 0, 0, 0, 0, "stream <1,4>"),
    (4, 40, 128, 9, 64, 0, 0, 0, 1, 0, 0, 0, "stream <4,2>, F*T = 576"),
    (4, 40, 96, 9, 64, 0, 0, 1, 0, 0, 0, 0, "stream <3,2>"),
    (4, 40, 64, 9, 64, 0, 1, 0, 1, 0, 0, 0, "stream <2,2>"),
    (4, 40, 32, 9, 64, 0, 0, 0, 0, 0, 0, 0, "stream <1,2>"),
    # tiled fallback
    (1, 64, 128, 4, 64, 1, 1, 0, 0, 0, 0, 0, "tiled 32-row tile (few tiles)"),
    (3, 64, 128, 32, 256, 1, 1, 0, 0, 0, 0, 0, "tiled 64-row tile (96 tiles x one 128-slice)"),
    (3, 64, 256, 32, 256, 1, 1, 0, 1, 0, 0, 0, "tiled 128-row tile (96 tiles x two 128-slices = 192)"),
    (1, 64, 40, 4, 64, 1, 1, 0, 1, 0, 0, 0, "tiled 64-row tile, Cout in 33..64: masked rows"),
    (1, 64, 96, 4, 64, 1, 0, 0, 0, 0, 0, 0, "tiled 96-row tile: act without in_scale"),
    (1, 8, 64, 4, 64, 1, 1, 0, 0, 0, 0, 0, "tiled, K = 8 (8-channel chunks), 64-row tile"),
    (1, 8, 32, 4, 64, 1, 1, 0, 0, 0, 0, 0, "tiled, K = 8, 32-row tile"),
    (1, 8, 96, 4, 64, 1, 1, 0, 1, 0, 0, 0, "tiled, K = 8, 96-row tile"),
    (3, 8, 256, 32, 256, 1, 1, 0, 0, 0, 0, 0, "tiled, K = 8, 128-row tile"),
    (1, 264, 128, 1, 64, 0, 0, 0, 1, 0, 0, 1, "tiled + split-K: a GEMM with K % 16 != 0"),
    (1, 320, 640, 1, 128, 0, 0, 0, 0, 0, 0, 1, "test_conv2d's \"larger K\" case: N = 128 columns, the skinny GEMM takes it"),
]

if __name__ == "__main__":
    commit, out = sys.argv[1:3]
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import test_gpu_kernels as T
    from audio_inpainting_diffusion_amd import _lib
    _lib.lib()
    rows = []
    for c in CASES:
        name, yc, ref, intact = T._c11_launch(_lib, c[:12])
        print(c[:12], name, "rel-L2 %.2e" % T.rel_l2(yc, ref), "intact" if intact else "WROTE OUTSIDE", flush=True)
        rows.append(list(c[:12]) + [name, c[12]])
    with open(out, "w") as f:
        f.write('{"commit": %s,\n "columns": %s,\n "cases": [\n' % (json.dumps(commit), json.dumps(COLUMNS)))
        f.write(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n ]}\n")
    print(len(rows), "cases ->", out)
