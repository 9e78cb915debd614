#!/usr/bin/env python3
"""Single-clip inference: the plain ``forward`` against ``forward_long`` over a sweep of ``segment_frames``.

Config S (BASELINE configs[1]), fp32, at the shapes the reference's inference callers use (training.py:488-500: one
clip of 360 000 samples; utils.py:238-259: one of 72 000) and at 4 x 72 000.  Protocol: every variant is captured into
a HIP graph after its warm-up calls (and also timed eagerly); the variants are then timed ALTERNATELY, round after
round, between HIP events, so that drift of the shared machine hits all of them alike; the table gives the median
over the rounds and the spread (min .. max).  Each shape runs in a child process of its own under a time limit; the
first failure ends the run.

usage: longform_bench.py [--out FILE] [--rounds N]          (parent: all shapes)
       longform_bench.py --shape B L [--rounds N]           (child: one shape, JSON lines on stdout)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 360000), (1, 72000), (4, 72000)]
SWEEP = {1125: (24, 32, 48, 64, 96, 128, 192, 256, 384), 225: (16, 24, 32, 48, 64, 100)}
CHILD_TIMEOUT_S = 420


def child(batch, length, rounds):
    import torch
    from audio_generation_amd import longform
    from audio_generation_amd.graph import GraphedForward
    from audio_generation_amd.vae import CausalVQAE

    dev = "cuda"
    torch.manual_seed(0)
    model = CausalVQAE(in_channels=1, n_blocks=4, strides=(2, 4, 5, 8), num_quantizers=8, codebook_size=1024,
                       codebook_dim=512, input_format="n c l", wavelet_decoders=False).eval().to(dev)
    gen = torch.Generator().manual_seed(1234)
    x = (0.1 * torch.randn(batch, 1, length, generator=gen)).clamp(-1, 1).to(dev)
    with torch.no_grad():
        model.quantizer.init_from_latents(model._run_encoders(x)[:2])
    rf = longform.receptive_field(model)
    n = -(-length // rf.scale_factor)
    default = longform.default_segment_frames(batch, n, rf.enc_halo_left, rf.enc_halo_right)

    variants = [("plain", None, model)]
    for seg in SWEEP[n]:
        variants.append((f"long seg={seg}", seg, (lambda s: lambda t: model.forward_long(t, segment_frames=s))(seg)))
    with torch.no_grad():
        y_plain, _, idx_plain = model(x)
    rows = []
    for name, seg, fn in variants:
        info = {"variant": name, "segment_frames": seg}
        if seg is not None:
            pe = longform.plan(n, seg, rf.enc_halo_left, rf.enc_halo_right, whole_frames=length // rf.scale_factor)
            pd = longform.plan(n, seg, rf.dec_halo_left, rf.dec_halo_right)
            if pe.single or pd.single:
                continue
            info.update(enc_windows=batch * pe.windows, enc_width=pe.width, dec_windows=batch * pd.windows, dec_width=pd.width,
                        enc_work=round((pe.windows * pe.width + (n - pe.tail_start if pe.tail_start is not None else 0)) / n, 3),
                        dec_work=round((pd.windows * pd.width + (n - pd.tail_start if pd.tail_start is not None else 0)) / n, 3))
            with torch.no_grad():
                y, _, idx = fn(x)
            info.update(bit_identical_waveform=bool(torch.equal(y, y_plain)), bit_identical_indices=bool(torch.equal(idx, idx_plain)),
                        waveform_rms_vs_plain=float((y.double() - y_plain.double()).pow(2).mean().sqrt()))
        rows.append((info, fn, GraphedForward(fn, x)))

    def timed(call, reps=3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    samples = {i: {"graph": [], "eager": []} for i in range(len(rows))}
    with torch.no_grad():
        for _ in range(2):                                     # warm every variant in both modes
            for info, fn, g in rows:
                g.replay()
                fn(x)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for i, (info, fn, g) in enumerate(rows):
                samples[i]["graph"].append(timed(g.replay))
                samples[i]["eager"].append(timed(lambda: fn(x)))
    for i, (info, fn, g) in enumerate(rows):
        for mode in ("graph", "eager"):
            v = samples[i][mode]
            info[mode] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
        print(json.dumps({"batch": batch, "length": length, "frames": n, "default_segment_frames": default, "rounds": rounds, **info}),
              flush=True)


def parent(out, rounds):
    lines = []
    for batch, length in SHAPES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", str(batch), str(length), "--rounds", str(rounds)],
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"shape {batch} x {length} failed ({r.returncode}): nothing more is started")
        lines += [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
    text = [f"# tools/longform_bench.py: config S, fp32, MI355X; ms per forward, median of {rounds} alternating rounds (min .. max)",
            "# work = frames computed / frames of the clip (halo overhead); windows = rows of the folded batch",
            f"{'shape':>12} {'variant':>14} {'enc win x W':>12} {'dec win x W':>12} {'enc work':>8} {'dec work':>8} "
            f"{'graph ms (min .. max)':>26} {'eager ms (min .. max)':>26} {'vs plain':>8}  bit-identical (wave, idx)  rms vs plain"]
    for batch, length in SHAPES:
        mine = [d for d in lines if (d["batch"], d["length"]) == (batch, length)]
        base = next(d for d in mine if d["variant"] == "plain")["graph"]["median_ms"]
        for d in mine:
            g, e = d["graph"], d["eager"]
            fold = d["segment_frames"] is not None
            text.append(
                f"{f'{batch} x {length}':>12} {d['variant']:>14} "
                f"{(str(d['enc_windows']) + ' x ' + str(d['enc_width'])) if fold else '-':>12} "
                f"{(str(d['dec_windows']) + ' x ' + str(d['dec_width'])) if fold else '-':>12} "
                f"{d['enc_work'] if fold else 1.0:>8} {d['dec_work'] if fold else 1.0:>8} "
                f"{g['median_ms']:>9.3f} ({g['min_ms']:.3f} .. {g['max_ms']:.3f}) {e['median_ms']:>9.3f} ({e['min_ms']:.3f} .. {e['max_ms']:.3f}) "
                f"{base / g['median_ms']:>7.2f}x  " + (f"{d['bit_identical_waveform']}, {d['bit_identical_indices']}  "
                                                     f"{d['waveform_rms_vs_plain']:.2e}" if fold else "-"))
        text.append(f"{'':>12} segment_frames=None picks {mine[0]['default_segment_frames']} at this shape")
    body = "\n".join(text) + "\n"
    print(body)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(body)
        with open(out + ".jsonl", "w") as f:
            f.writelines(json.dumps(d) + "\n" for d in lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs=2, type=int)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "longform_times.txt"))
    a = ap.parse_args()
    if a.shape:
        child(a.shape[0], a.shape[1], a.rounds)
    else:
        parent(a.out, a.rounds)
