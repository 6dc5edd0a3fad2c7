#!/usr/bin/env python
"""Objective metrics of a folder of restored recordings against a folder of references (audio_inpainting_diffusion_amd/metrics.py through
harness.evaluate_long): log-spectral distance, SNR, SI-SDR and the largest sample error per file, their mean and median over the folder.

    tools/evaluate.py REF_DIR EST_DIR [--task TASK ...] [--n-fft 2048] [--hop 512] [--band LO_HZ HI_HZ] [--json OUT]

The 16-bit mono wav files of EST_DIR (what harness.write_audio_file writes) are paired BY NAME with those of REF_DIR and read with
harness.read_wav.  A name without a partner, a pair whose sampling rates or lengths differ, and a folder of mixed rates are refused, by name.
--task says what the files are judged on (metrics.region_of):
    inpainting   --mask-dir DIR          wav files of the same names, a non-zero sample = observed: the gaps are evaluated
    declipping   --degraded-dir DIR --clip-value C     the clipped recordings: the samples with |y| >= C are evaluated
    bwe          --cutoff-hz F           every sample; lsd over the band (F, rate / 2)
    spectrogram_inpainting | pr | compsens | all (the default)     every sample, every bin
--band overrides the band of the task.  Prints the table and the summary; --json writes rows, summary and settings.  Needs the GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COLUMNS = (("lsd", "lsd", "%9.4f"), ("snr_db", "snr dB", "%9.3f"), ("si_sdr_db", "si-sdr dB", "%9.3f"), ("max_abs_err", "max err", "%9.2e"),
           ("n_samples", "samples", "%9.0f"), ("n_frames", "frames", "%7.0f"))


def wav_names(folder):
    if not os.path.isdir(folder):
        raise SystemExit(f"evaluate: {folder} is not a folder")
    return sorted(f for f in os.listdir(folder) if f.lower().endswith(".wav"))


def read_pairs(ref_dir, est_dir):
    """(names, references, estimates, rate): 1-D float32 tensors paired by file name; every mismatch is refused by name"""
    from audio_inpainting_diffusion_amd import harness
    names, other = wav_names(est_dir), set(wav_names(ref_dir))
    if not names:
        raise SystemExit(f"evaluate: no wav file in {est_dir}")
    lone = sorted(set(names) ^ other)
    if lone:
        raise SystemExit(f"evaluate: without a partner of the same name in the other folder: {', '.join(lone)}")
    refs, ests, rate = [], [], None
    for n in names:
        (r, fr), (e, fe) = harness.read_wav(os.path.join(ref_dir, n)), harness.read_wav(os.path.join(est_dir, n))
        if fr != fe:
            raise SystemExit(f"evaluate: {n}: the reference is sampled at {fr} Hz, the estimate at {fe} Hz")
        if r.numel() != e.numel():
            raise SystemExit(f"evaluate: {n}: the reference has {r.numel()} samples, the estimate {e.numel()}")
        if r.numel() == 0:
            raise SystemExit(f"evaluate: {n}: no samples")
        if rate is not None and fr != rate:
            raise SystemExit(f"evaluate: {n}: sampled at {fr} Hz, the files before it at {rate} Hz (one rate per run)")
        rate = fr
        refs.append(r.reshape(-1))
        ests.append(e.reshape(-1))
    return names, refs, ests, rate


def read_side(folder, names, refs, rate, what):
    """the wav of every name in ``folder`` (masks, degraded recordings), with the checks of read_pairs"""
    from audio_inpainting_diffusion_amd import harness
    out = []
    for n, r in zip(names, refs):
        fn = os.path.join(folder, n)
        if not os.path.isfile(fn):
            raise SystemExit(f"evaluate: {n}: no {what} in {folder}")
        x, fs = harness.read_wav(fn)
        if fs != rate or x.numel() != r.numel():
            raise SystemExit(f"evaluate: {n}: the {what} has {x.numel()} samples at {fs} Hz, the reference {r.numel()} at {rate} Hz")
        out.append(x.reshape(-1))
    return out


def table(names, rows, summary):
    width = max(len("median"), max(len(n) for n in names))
    lines = [" " * width + "".join(" %*s" % (len(fmt % 0), head) for _, head, fmt in COLUMNS)]
    for n, row in zip(names, rows):
        lines.append(n.ljust(width) + "".join(" " + fmt % row[k] for k, _, fmt in COLUMNS))
    for stat in ("mean", "median"):
        lines.append(stat.ljust(width) + "".join(" " + (fmt % summary[k][stat] if k in summary else " " * len(fmt % 0)) for k, _, fmt in COLUMNS))
    bad = {k: summary[k]["n_not_finite"] for k, _, _ in COLUMNS if k in summary and summary[k]["n_not_finite"]}
    lines.append(f"{summary['n_files']} files; mean and median over the files where the metric is finite" +
                 ("" if not bad else "; not finite: " + ", ".join(f"{k} in {v}" for k, v in bad.items())))
    return "\n".join(lines)


def plain(v):
    """strict JSON has no inf / nan: they are written as strings"""
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    return repr(v) if isinstance(v, float) and v - v != 0 else v


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("ref_dir")
    ap.add_argument("est_dir")
    ap.add_argument("--task", default="all", choices=("all", "inpainting", "declipping", "bwe", "spectrogram_inpainting", "pr", "compsens"))
    ap.add_argument("--mask-dir")
    ap.add_argument("--degraded-dir")
    ap.add_argument("--clip-value", type=float)
    ap.add_argument("--cutoff-hz", type=float)
    ap.add_argument("--n-fft", type=int, default=2048)
    ap.add_argument("--hop", type=int, default=512)
    ap.add_argument("--band", type=float, nargs=2, metavar=("LO_HZ", "HI_HZ"))
    ap.add_argument("--floor", type=float, default=1e-10)
    ap.add_argument("--json")
    a = ap.parse_args(argv)
    from audio_inpainting_diffusion_amd import harness, metrics
    names, refs, ests, rate = read_pairs(a.ref_dir, a.est_dir)
    regions, band = None, None
    if a.task == "inpainting":
        if not a.mask_dir:
            raise SystemExit("evaluate: --task inpainting needs --mask-dir")
        regions = [metrics.region_of("inpainting", mask=(m != 0).float())[0] for m in read_side(a.mask_dir, names, refs, rate, "mask")]
    elif a.task == "declipping":
        if not a.degraded_dir or a.clip_value is None:
            raise SystemExit("evaluate: --task declipping needs --degraded-dir and --clip-value")
        regions = [metrics.region_of("declipping", y=y, clip_value=a.clip_value)[0].reshape(-1)
                   for y in read_side(a.degraded_dir, names, refs, rate, "clipped recording")]
    elif a.task == "bwe":
        if a.cutoff_hz is None:
            raise SystemExit("evaluate: --task bwe needs --cutoff-hz")
        band = metrics.region_of("bwe", cutoff_hz=a.cutoff_hz, sample_rate=rate)[1]
    elif a.task != "all":
        regions, band = metrics.region_of(a.task)
    band = tuple(a.band) if a.band else band
    rows, summary = harness.evaluate_long(refs, ests, regions, sample_rate=rate, n_fft=a.n_fft, hop=a.hop, band=band, floor=a.floor)
    print(table(names, rows, summary))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(plain({"settings": {"task": a.task, "sample_rate": rate, "n_fft": a.n_fft, "hop": a.hop, "band": band, "floor": a.floor},
                       "rows": [dict(row, name=n) for n, row in zip(names, rows)], "summary": summary}), f, indent=1, allow_nan=False)
            f.write("\n")
    return rows, summary


if __name__ == "__main__":
    main()
