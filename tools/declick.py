#!/usr/bin/env python
"""Declick a folder of recordings (audio_inpainting_diffusion_amd/declick.py through harness.declick_detect / harness.declick_long): find the
clicks and short dropouts of every file on the GPU and restore them with the inpainter.

    tools/declick.py IN_DIR OUT_DIR [--detect-only] [--json OUT] [--block 2048] [--order 16] [--threshold 8] [--pad 16] [--min-run 8]
                     [--max-run 1024] [--ridge 1e-6] [--sigma-floor 1e-6] [--max-fraction 0.2]
                     [--checkpoint CKPT --preset maestro22k --steps 36 --seed 0 --max-batch 8] [--allow-unpinned-cqt]

The 16-bit mono wav files of IN_DIR are read with harness.read_wav; files of one rate only (named otherwise).  For every file the mask goes
to OUT_DIR/masks/NAME.wav (a non-zero sample = observed, what ``tools/evaluate.py --task inpainting --mask-dir`` reads) and one row to the
report: samples, masked samples and their fraction, gaps, the longest gap.  --detect-only stops there and needs no model.  Otherwise
--checkpoint names trained weights for the network of --preset (config.make_args), and the restored files go to OUT_DIR/NAME.wav
(harness.write_audio_file): the files of all lengths share the batches of one pooled restoration, file i with seed --seed + i.
--json writes the rows and the settings.  Needs the GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SETTINGS = (("block", int), ("order", int), ("threshold", float), ("pad", int), ("min_run", int), ("max_run", int), ("ridge", float),
            ("sigma_floor", float), ("max_fraction", float))


def read_folder(folder):
    """(names, 1-D float32 tensors, rate) of the wav files of ``folder``; an empty folder, an empty file and mixed rates are refused by name"""
    from audio_inpainting_diffusion_amd import harness
    if not os.path.isdir(folder):
        raise SystemExit(f"declick: {folder} is not a folder")
    names = sorted(f for f in os.listdir(folder) if f.lower().endswith(".wav"))
    if not names:
        raise SystemExit(f"declick: no wav file in {folder}")
    files, rate = [], None
    for n in names:
        x, fs = harness.read_wav(os.path.join(folder, n))
        if x.numel() == 0:
            raise SystemExit(f"declick: {n}: no samples")
        if rate is not None and fs != rate:
            raise SystemExit(f"declick: {n}: sampled at {fs} Hz, the files before it at {rate} Hz (one rate per run)")
        rate = fs
        files.append(x.reshape(-1))
    return names, files, rate


def table(rows):
    width = max(len("file"), max(len(r["name"]) for r in rows))
    lines = ["file".ljust(width) + "   samples    masked  fraction   gaps  longest"]
    for r in rows:
        lines.append(r["name"].ljust(width) + " %9d %9d %9.5f %6d %8d" % (r["samples"], r["n_flagged"], r["fraction"], r["n_gaps"], r["longest_gap"]))
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("in_dir")
    ap.add_argument("out_dir")
    ap.add_argument("--detect-only", action="store_true")
    ap.add_argument("--json")
    for name, kind in SETTINGS:
        ap.add_argument("--" + name.replace("_", "-"), type=kind, default=None)
    ap.add_argument("--checkpoint")
    ap.add_argument("--preset", default="maestro22k")
    ap.add_argument("--steps", type=int, default=36)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-batch", type=int, default=8)
    ap.add_argument("--allow-unpinned-cqt", action="store_true")
    a = ap.parse_args(argv)
    if not a.detect_only and not a.checkpoint:
        raise SystemExit("declick: restoring needs --checkpoint (trained weights); --detect-only writes the masks and the report without a model")
    import torch
    from audio_inpainting_diffusion_amd import declick, harness
    settings = {name: getattr(a, name) for name, _ in SETTINGS if getattr(a, name) is not None}
    names, files, rate = read_folder(a.in_dir)
    if a.detect_only:
        cfg = declick.make_settings(**settings)
        masks, reports = harness.declick_detect(files, "cuda", None, cfg._asdict())
        restored = None
    else:
        from audio_inpainting_diffusion_amd.config import make_args
        from audio_inpainting_diffusion_amd.edm import EDM
        from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
        from audio_inpainting_diffusion_amd.sampler import Sampler
        args = make_args(a.preset, T=a.steps)
        if int(args.exp.sample_rate) != int(rate):
            raise SystemExit(f"declick: the files are sampled at {rate} Hz, the network of --preset {a.preset} works at {args.exp.sample_rate} Hz")
        net = Unet_CQT_oct_with_attention(args, torch.device("cuda"))
        harness.load_checkpoint(net, a.checkpoint, allow_unpinned_cqt=a.allow_unpinned_cqt)
        smp = Sampler(model=net, diff_params=EDM(args), args=args)
        cfg = declick.settings_of(args, **settings)
        restored, reports = harness.declick_long(smp, files, seeds=[a.seed + i for i in range(len(files))], max_batch=a.max_batch, pool=True, **settings)
        masks = [r.mask for r in reports]
    rows = []
    for n, f, m, r in zip(names, files, masks, reports):
        stem = os.path.splitext(n)[0]
        harness.write_audio_file(m * 0.5, rate, stem, os.path.join(a.out_dir, "masks"))
        if restored is not None:
            harness.write_audio_file(restored[len(rows)], rate, stem, a.out_dir)
        rows.append({"name": n, "samples": f.numel(), "n_flagged": int(r.n_flagged), "fraction": int(r.n_flagged) / f.numel(), "n_gaps": int(r.n_gaps),
                     "longest_gap": int(r.longest_gap)})
    print(table(rows))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"settings": dict(cfg._asdict(), sample_rate=rate, detect_only=a.detect_only), "rows": rows}, f, indent=1, allow_nan=False)
            f.write("\n")
    return rows


if __name__ == "__main__":
    main()
