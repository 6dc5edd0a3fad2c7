#!/usr/bin/env python
"""Segments of twice the shipped length (L = 368368, 16.7 s at 22.05 kHz: attention T = 256 / 128 / 64 on levels 4 / 5 / 6) on the chunked time
attention of csrc/aid_attn_long.hip.  Three parts, chosen with --parts, one JSON line in all (and --out):

 kernel : aid_time_attention_long and its VJP at (B*H, F, T) = (64, 320, 256) -- what maestro22k at L = 368368 and batch 8 launches on level 4 --
          alternated in one process with the EXISTING kernels at (64, 320, 128): --rounds rounds of --reps launches each, timed by events on the
          stream.  FLOP/s with the plan's own counts (4 and 10 * B*H * T^2 * F) and as a fraction of the 157.3 TFLOP/s fp32-MFMA peak.  The
          yardstick is the old kernel's rate; the margin is its own spread over the rounds + 5 % (two more barriers per 128-key chunk).
 e2e    : maestro22k, guided (xi = 0.25), complete T = 36 runs of predict_inpainting: L = 368368 at batch 4 against L = 184184 at batch 8 (the same
          samples per evaluation), alternated twice: evaluations/s, seconds of audio per second, spread of the identical runs.
 parity : once, at full size: forward and one guided evaluation (x_hat, guidance gradient) at L = 368368, B = 1, seeded weights with O(1) gates,
          against the CPU oracle (rel-L2, the project's 1e-4).  Tens of seconds of CPU and ~40 GB of host memory: a tool's job, not a test's."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_FP32_MFMA = 157.3e12
L_SHORT, L_LONG = 184184, 368368


def _rate(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / reps


def kernel_part(a):
    import torch
    from audio_inpainting_diffusion_amd import _lib as L
    L.lib()
    BH, Fd = 64, 320
    B, H = 8, 8

    def case(T, fwd, bwd):
        g = torch.Generator().manual_seed(T)
        qk = torch.randn(B, H * 2 * Fd, T, generator=g).cuda()
        v, go = torch.randn(B, H, Fd, T, generator=g).cuda(), torch.randn(B, H, Fd, T, generator=g).cuda()
        out, gv, gqk = torch.empty_like(v), torch.empty_like(v), torch.empty_like(qk)
        probs, ws = torch.empty(B, H, T, T, device="cuda"), torch.empty(B, H, T, T, device="cuda")
        sc = float(Fd) ** -0.5
        pf = L.AttentionParams(qk.data_ptr(), v.data_ptr(), out.data_ptr(), probs.data_ptr(), B, H, Fd, T, sc, None)
        pb = L.AttentionBwdParams(qk.data_ptr(), v.data_ptr(), probs.data_ptr(), go.data_ptr(), gqk.data_ptr(), gv.data_ptr(), B, H, Fd, T, sc, 0, ws.data_ptr())
        keep = (qk, v, go, out, gv, gqk, probs, ws)
        return {"T": T, "fwd": lambda: L.call(fwd, pf), "bwd": lambda: L.call(bwd, pb), "keep": keep, "names": (fwd, bwd),
                "flops": (4 * BH * T * T * Fd, 10 * BH * T * T * Fd), "t": ([], [])}
    cases = [case(128, "aid_time_attention", "aid_time_attention_bwd"), case(256, "aid_time_attention_long", "aid_time_attention_long_bwd"),
             case(128, "aid_time_attention_long", "aid_time_attention_long_bwd")]
    for c in cases:                                              # warm-up
        _rate(c["fwd"], 20), _rate(c["bwd"], 20)
    for _ in range(a.rounds):
        for c in cases:
            c["t"][0].append(_rate(c["fwd"], a.reps))
            c["t"][1].append(_rate(c["bwd"], a.reps))
    res = []
    for c in cases:
        row = {"entries": c["names"], "BH": BH, "F": Fd, "T": c["T"]}
        for k, which in enumerate(("forward", "vjp")):
            r = sorted(c["flops"][k] / t for t in c["t"][k])
            med = r[len(r) // 2]
            row[which] = {"us_median": round(c["flops"][k] / med * 1e6, 2), "tflops_median": round(med / 1e12, 2), "tflops_min": round(r[0] / 1e12, 2),
                          "tflops_max": round(r[-1] / 1e12, 2), "spread": round((r[-1] - r[0]) / r[-1], 4), "of_fp32_mfma_peak": round(med / PEAK_FP32_MFMA, 4)}
        res.append(row)
    verdict = {}
    for which in ("forward", "vjp"):
        old, new = res[0][which], res[1][which]
        margin = old["spread"] + 0.05
        verdict[which] = {"long_over_old_rate": round(new["tflops_median"] / old["tflops_median"], 4), "margin_old_spread_plus_5pct": round(margin, 4),
                          "long_within_margin_of_old": bool(new["tflops_median"] >= old["tflops_median"] * (1 - margin))}
    return {"rounds": a.rounds, "reps": a.reps, "cases": res, "long_T256_against_old_T128": verdict}


def _full_net(L, dev, gates=False):
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.init import seeded_init_
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    args = make_args("maestro22k", audio_len=L, T=36, xi=0.25)
    kw = dict(gate_scale=10.0, affine_scale=10.0) if gates else {}
    return seeded_init_(Unet_CQT_oct_with_attention(args, dev), 0, **kw), args


def e2e_part(a):
    import torch
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_normal
    from audio_inpainting_diffusion_amd.masks import long_gap_mask
    from audio_inpainting_diffusion_amd.sampler import Sampler
    dev = torch.device("cuda", 0)
    setups = []
    for L, B in ((L_SHORT, 8), (L_LONG, 4)):
        net, args = _full_net(L, dev)
        net.prepare()
        smp = Sampler(model=net, diff_params=EDM(args), args=args)
        y = (torch.from_numpy(seeded_normal(7, 0, B * L)).reshape(B, L).float() * 0.063).to(dev)
        mask = long_gap_mask(L, 22050, 300)
        Tl = [int(net.CQTransform.plan.T_oct[net.num_octs - 1 - i]) for i in range(net.num_octs) if net.attention_layers[i]]
        setups.append({"L": L, "B": B, "smp": smp, "y": y, "mask": mask, "attention_T": Tl, "runs": []})

    def run(s, steps):
        smp = s["smp"]
        smp.nb_steps, smp.seeds = steps, list(range(s["B"]))
        torch.cuda.synchronize()
        n0, t = smp.n_evals, time.perf_counter()
        out = smp.predict_inpainting(s["y"] * s["mask"].to(dev), s["mask"])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        assert bool(torch.isfinite(out).all())
        return (smp.n_evals - n0) / dt, dt
    for s in setups:                                             # warm-up: plans, graphs, pinned buffers
        run(s, 2)
        print(f"[long_segment_bench] warmed L = {s['L']} batch {s['B']}", file=sys.stderr, flush=True)
    for _ in range(2):
        for s in setups:
            s["runs"].append(run(s, 36))
    res = []
    for s in setups:
        ev = [r[0] for r in s["runs"]]
        audio = [s["B"] * s["L"] / 22050 / r[1] for r in s["runs"]]
        res.append({"segment": s["L"], "batch": s["B"], "attention_T_per_level": s["attention_T"], "evals_per_s": [round(v, 2) for v in ev],
                    "run_s": [round(r[1], 3) for r in s["runs"]], "audio_s_restored_per_s": [round(v, 3) for v in audio],
                    "spread_of_identical_runs": round(abs(ev[0] - ev[1]) / max(ev), 5)})
    return {"config": "maestro22k", "T": 36, "xi": 0.25, "runs": res,
            "long_over_short_evals_per_s": round(sum(res[1]["evals_per_s"]) / sum(res[0]["evals_per_s"]), 4)}


def profile_part(a):
    """what a `rocprofv3 --kernel-trace --stats -- python tools/long_segment_bench.py --parts profile` run (a run of its own) should see:
    five guided Heun steps at L = 368368, batch 4, nothing else"""
    import torch
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_normal
    from audio_inpainting_diffusion_amd.masks import long_gap_mask
    from audio_inpainting_diffusion_amd.sampler import Sampler
    dev = torch.device("cuda", 0)
    L, B = L_LONG, 4
    net, args = _full_net(L, dev)
    smp = Sampler(model=net, diff_params=EDM(args), args=args)
    y = (torch.from_numpy(seeded_normal(7, 0, B * L)).reshape(B, L).float() * 0.063).to(dev)
    mask = long_gap_mask(L, 22050, 300)
    smp.nb_steps, smp.seeds = 5, list(range(B))
    n0 = smp.n_evals
    smp.predict_inpainting(y * mask.to(dev), mask)
    torch.cuda.synchronize()
    return {"segment": L, "batch": B, "steps": 5, "evals": smp.n_evals - n0}


def parity_part(a):
    import torch
    from audio_inpainting_diffusion_amd.init import seeded_normal
    from audio_inpainting_diffusion_amd.masks import long_gap_mask
    from oracle.edm import OracleEDM
    from oracle.nsgt_cqt import OracleCQT
    from oracle.unet import OracleUnet
    dev = torch.device("cuda", 0)
    rel = lambda x, r: float((x.double() - r.double()).norm() / r.double().norm())                        # noqa: E731
    Ls = L_LONG
    net, _ = _full_net(Ls, dev, gates=True)
    edm = OracleEDM()
    x = torch.from_numpy(seeded_normal(21, 0, Ls)).reshape(1, Ls) * 0.3
    y = torch.from_numpy(seeded_normal(22, 0, Ls)).reshape(1, Ls) * 0.063
    mask = long_gap_mask(Ls, 22050, 300)
    s = torch.full((1, 1), 0.4)
    v = lambda t: t.reshape(-1).to(dev).contiguous()                                                        # noqa: E731
    cn = edm.cnoise(s)
    with torch.no_grad():
        fwd = net(x.to(dev), cn.reshape(1, 1).to(dev)).cpu()
    xh, g, _ = net.denoise_guided(x.to(dev), v(cn), v(edm.cin(s)), v(edm.cskip(s)), v(edm.cout(s)), True, (y * mask).to(dev), mask.to(dev))
    xh, g = xh.cpu(), g.cpu()
    names = sorted({o.name for o in net._state(1)["plan_body"].ops if o.name.startswith("aid_time_attention")})
    print("[long_segment_bench] GPU side done, oracle on the CPU ...", file=sys.stderr, flush=True)
    t = time.perf_counter()
    orc = OracleUnet(7, 64, OracleCQT(7, 64, "oct", ("kaiser", 1), 22050, Ls)).load_state_dict(net.state_dict())
    with torch.no_grad():
        fwd_ref = orc(x, cn.reshape(1, 1))
    print(f"[long_segment_bench] oracle forward {time.perf_counter() - t:.0f} s", file=sys.stderr, flush=True)
    xr = x.clone().requires_grad_()
    xh_ref = orc.CQTransform.apply_hpf_DC(edm.denoiser(xr, orc, s))
    g_ref = torch.autograd.grad(torch.linalg.norm(y * mask - mask * xh_ref, dim=1, ord=2).sum(), xr)[0]
    res = {"segment": Ls, "batch": 1, "attention_entries_planned": names, "forward_rel_l2": rel(fwd, fwd_ref), "x_hat_rel_l2": rel(xh, xh_ref.detach()),
           "guidance_gradient_rel_l2": rel(g, g_ref), "bound": 1e-4, "oracle_cpu_s": round(time.perf_counter() - t, 1)}
    res["within_bound"] = bool(max(res["forward_rel_l2"], res["x_hat_rel_l2"], res["guidance_gradient_rel_l2"]) < 1e-4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernel,e2e,parity")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    out = {"tool": "long_segment_bench", "device": torch.cuda.get_device_name(0)}
    for part, fn in (("kernel", kernel_part), ("e2e", e2e_part), ("parity", parity_part), ("profile", profile_part)):
        if part in a.parts.split(","):
            out[part] = fn(a)
            print(f"[long_segment_bench] {part} done", file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
            if a.out:                                            # (after every part: a later part that fails keeps what was measured)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    f.write(json.dumps(out) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
