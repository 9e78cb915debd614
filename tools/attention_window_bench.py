"""Sliding-window attention beside the causal kernels it narrows (informational, no gate).

The protocol of tools/attention_causal_bench.py: one process, HIP events, warm-up calls per case, then ROUNDS rounds; in every
round each case is timed over its CALLS back-to-back calls between two events, the cases alternated; median / min / max of the
per-round microseconds per call (the Python wrapper, which allocates outputs and workspace per call, included).  Every
baseline -- the unchanged causal kernels -- is listed twice (``again``): the two rows were measured in the same run, alternated
with everything else, and their difference is the run-to-run spread a windowed row has to be read against.

Cases: forward and backward at T = 1125, W = 128 against ``attention_alibi_causal`` and its backward; one cached step, tq = 1
at position 1124 with W = 128 on a ring of 256, against the causal cached step on tk = 1125 keys; W >= T against causal at
T = 225 and T = 1125 (report only).  The last lines give each ratio next to the ratio of 64-key blocks the kernels walk.

    python tools/attention_window_bench.py > profiles/attention_window.txt
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audio_generation_amd import ops  # noqa: E402

B, H, DH = 32, 8, 64
T, W, RING = 1125, 128, 256
ROUNDS = 5


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda"
    gen = torch.Generator().manual_seed(0)
    slopes = (2.0 ** (-8.0 / torch.arange(H, 0, -1))).to(dev)
    attn = dict(heads=H, head_dim=DH, scale_div=DH ** 0.5)
    cases = []          # (name, fn, calls per round, warm-up calls)
    pairs = []          # (windowed case, its baseline, 64-key blocks walked: windowed, baseline)

    def add(name, fn, calls, warm):
        cases.append((name, fn, calls, warm))

    def blocks(tq, pos, w):
        per = 2 * B * H * DH * 128 * 64
        return ops._window_macs(B, H, DH, tq, pos, w) // per, ops._causal_macs(B, H, DH, tq, pos + tq, pos) // per

    for t in (225, T):
        qkv = (0.7 * torch.randn(B, 3 * H * DH, t, generator=gen)).to(dev)
        dout = torch.randn(B, H * DH, t, generator=gen).to(dev)
        out_c = ops.attention_alibi_causal(qkv, None, slopes, **attn)
        fc, bc = (200, 50) if t <= 256 else (40, 8)
        cau_f = lambda qkv=qkv: ops.attention_alibi_causal(qkv, None, slopes, **attn)                                    # noqa: E731
        add(f"causal fwd T={t}", cau_f, fc, 20)
        if t == T:
            out_w = ops.attention_alibi_window(qkv, None, slopes, **attn, window=W)
            add(f"window fwd T={t} W={W}", lambda qkv=qkv: ops.attention_alibi_window(qkv, None, slopes, **attn, window=W), fc, 20)
            pairs.append((f"window fwd T={t} W={W}", f"causal fwd T={t}", *blocks(t, 0, W)))
        add(f"window fwd T={t} W={t} (W >= T)", lambda qkv=qkv, t=t: ops.attention_alibi_window(qkv, None, slopes, **attn, window=t),
            fc, 20)
        pairs.append((f"window fwd T={t} W={t} (W >= T)", f"causal fwd T={t}", *blocks(t, 0, t)))
        add(f"causal fwd T={t} again", cau_f, fc, 0)
        if t == T:
            cau_b = lambda qkv=qkv, out=out_c, dout=dout: ops.attention_alibi_causal_backward(qkv, slopes, out, dout, **attn)   # noqa: E731
            add(f"causal bwd T={t}", cau_b, bc, 5)
            add(f"window bwd T={t} W={W}",
                lambda qkv=qkv, out=out_w, dout=dout: ops.attention_alibi_window_backward(qkv, slopes, out, dout, **attn, window=W), bc, 5)
            pairs.append((f"window bwd T={t} W={W}", f"causal bwd T={t}", None, None))
            add(f"causal bwd T={t} again", cau_b, bc, 0)
    q1 = (0.7 * torch.randn(B, H * DH, 1, generator=gen)).to(dev)
    cache = (0.7 * torch.randn(B, 2 * H * DH, T, generator=gen)).to(dev)
    ring = (0.7 * torch.randn(B, 2 * H * DH, RING, generator=gen)).to(dev)
    step_c = lambda: ops.attention_alibi_causal(q1, cache, slopes, **attn, q_pos0=T - 1, tk=T)                           # noqa: E731
    add(f"causal cached step tq=1 tk={T}", step_c, 200, 20)
    add(f"window ring step tq=1 pos={T - 1} W={W} ring={RING}",
        lambda: ops.attention_alibi_window(q1, ring, slopes, **attn, window=W, q_pos0=T - 1, ring=RING), 200, 20)
    pairs.append((f"window ring step tq=1 pos={T - 1} W={W} ring={RING}", f"causal cached step tq=1 tk={T}", *blocks(1, T - 1, W)))
    add(f"causal cached step tq=1 tk={T} again", step_c, 200, 0)

    for _, fn, _, warm in cases:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _, _ in cases}
    for _ in range(ROUNDS):
        for name, fn, calls, _ in cases:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(calls):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(1e3 * start.elapsed_time(stop) / calls)
    print(f"# HIP-event times, us per call (wrapper included), B={B} H={H} Dh={DH}, fp32; {ROUNDS} rounds, cases alternated")
    print(f"# {'case':<50}{'calls':>7}{'median':>11}{'min':>11}{'max':>11}")
    med = {}
    for name, _, calls, _ in cases:
        ts = times[name]
        med[name] = statistics.median(ts)
        print(f"{name:<52}{calls:7d}{med[name]:11.1f}{min(ts):11.1f}{max(ts):11.1f}", flush=True)
    print("# windowed / causal baseline (the two baseline medians span its spread); blocks walked: windowed / causal")
    for name, base, bw, bc in pairs:
        lo, hi = sorted((med[base], med[base + " again"]))
        blk = "" if bw is None else f"   blocks {bw} / {bc} = {bw / bc:.2f}"
        verdict = "not slower" if med[name] <= hi else "SLOWER than the baseline beyond its spread"
        print(f"{name:<52}{med[name]:9.1f} / {lo:.1f}..{hi:.1f} = {med[name] / hi:.2f}..{med[name] / lo:.2f}{blk}   {verdict}")


if __name__ == "__main__":
    main()
