"""Ragged attention beside the cross-attention kernels it is the twin of (informational, no gate).

The protocol of tools/attention_window_bench.py: one process, HIP events, warm-up calls per case, then ROUNDS rounds; in every
round each case is timed over its CALLS back-to-back calls between two events, the cases alternated; median / min / max of the
per-round microseconds per call (the Python wrapper, which allocates outputs and workspace per call, included).  Every
baseline -- the unchanged cross-attention kernels -- is listed twice (``again``): the two rows were measured in the same run,
alternated with everything else, and their difference is the run-to-run spread a ragged row has to be read against.

Cases, at the config-3 attention shape B = 32, H = 8, Dh = 64, T = 225 (q and kv as two tensors for every op):
1. ragged forward / backward with all lengths full against ``attention_alibi_cross`` / ``_backward``;
2. ragged with lengths drawn uniformly in [T/4, T] (seeded) against (1), next to the ratio of the 64-key x 128-query forward
   tiles and of the 16 x 64 backward tiles the kernels walk;
3. the two ``mask_tail`` passes of a block call (out of place on x, in place on the output, (32, 512, 225)) and the config-3
   block, ``Transformer(512, depth=1, heads=8, head_dim=64, context_x=225)`` in eval mode, with and without lengths.

    python tools/attention_ragged_bench.py > profiles/attention_ragged.txt
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audio_generation_amd import ops  # noqa: E402
from audio_generation_amd.transformers import Transformer  # noqa: E402

B, H, DH, T = 32, 8, 64, 225
ROUNDS = 5


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda"
    gen = torch.Generator().manual_seed(0)
    slopes = (2.0 ** (-8.0 / torch.arange(H, 0, -1))).to(dev)
    attn = dict(heads=H, head_dim=DH, scale_div=DH ** 0.5)
    q = (0.7 * torch.randn(B, H * DH, T, generator=gen)).to(dev)
    kv = (0.7 * torch.randn(B, 2 * H * DH, T, generator=gen)).to(dev)
    dout = torch.randn(B, H * DH, T, generator=gen).to(dev)
    drawn = torch.randint(T // 4, T + 1, (B,), generator=gen)
    full = torch.full((B,), T, dtype=torch.int32, device=dev)
    short = drawn.to(torch.int32).to(dev)
    out_c = ops.attention_alibi_cross(q, kv, slopes, **attn)
    out_f = ops.attention_alibi_ragged(q, kv, slopes, **attn, q_len=full, k_len=full)
    out_s = ops.attention_alibi_ragged(q, kv, slopes, **attn, q_len=short, k_len=short)
    print(f"# full lengths against attention_alibi_cross: max difference {float((out_f - out_c).abs().max()):.3e}")

    cases = []          # (name, fn, calls per round, warm-up calls)

    def add(name, fn, calls, warm):
        cases.append((name, fn, calls, warm))

    cross_f = lambda: ops.attention_alibi_cross(q, kv, slopes, **attn)                                              # noqa: E731
    cross_b = lambda: ops.attention_alibi_cross_backward(q, kv, slopes, out_c, dout, **attn)                        # noqa: E731
    add("cross fwd", cross_f, 200, 20)
    add("ragged fwd, full lengths", lambda: ops.attention_alibi_ragged(q, kv, slopes, **attn, q_len=full, k_len=full), 200, 20)
    add("ragged fwd, lengths in [T/4, T]", lambda: ops.attention_alibi_ragged(q, kv, slopes, **attn, q_len=short, k_len=short), 200, 20)
    add("cross fwd again", cross_f, 200, 0)
    add("cross bwd", cross_b, 50, 5)
    add("ragged bwd, full lengths",
        lambda: ops.attention_alibi_ragged_backward(q, kv, slopes, out_f, dout, **attn, q_len=full, k_len=full), 50, 5)
    add("ragged bwd, lengths in [T/4, T]",
        lambda: ops.attention_alibi_ragged_backward(q, kv, slopes, out_s, dout, **attn, q_len=short, k_len=short), 50, 5)
    add("cross bwd again", cross_b, 50, 0)

    torch.manual_seed(0)
    tf = Transformer(H * DH, depth=1, heads=H, head_dim=DH, context_x=T).to(dev).eval()
    x = torch.randn(B, H * DH, T, generator=gen).to(dev)
    y = torch.empty_like(x)

    def masks():
        ops.mask_tail(x, short)
        ops.mask_tail(y, short, out=y)

    def block(**kw):
        with torch.no_grad():
            tf.run_bct(x, **kw)
    add("block, no lengths", block, 50, 5)
    add("block, full lengths", lambda: block(lengths=full), 50, 5)
    add("block, lengths in [T/4, T]", lambda: block(lengths=short), 50, 5)
    add("block, no lengths again", block, 50, 0)
    add("mask_tail x 2 (out of place + in place)", masks, 200, 20)

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
    print(f"# HIP-event times, us per call (wrapper included), B={B} H={H} Dh={DH} T={T}, fp32; {ROUNDS} rounds, cases alternated")
    print(f"# lengths drawn in [{T // 4}, {T}]: {drawn.tolist()}")
    print(f"# {'case':<50}{'calls':>7}{'median':>11}{'min':>11}{'max':>11}")
    med = {}
    for name, _, calls, _ in cases:
        ts = times[name]
        med[name] = statistics.median(ts)
        print(f"{name:<52}{calls:7d}{med[name]:11.1f}{min(ts):11.1f}{max(ts):11.1f}", flush=True)

    cd = lambda a, b: -(-a // b)                                                                                     # noqa: E731
    lens = drawn.tolist()
    fwd_tiles = sum(cd(n, 128) * cd(n, 64) for n in lens) / (B * cd(T, 128) * cd(T, 64))
    bwd_tiles = sum(cd(n, 16) * cd(n, 64) for n in lens) / (B * cd(T, 16) * cd(T, 64))
    print("# ragged / baseline (the two baseline medians span its spread)")
    for name, base, note in (("ragged fwd, full lengths", "cross fwd", ""), ("ragged bwd, full lengths", "cross bwd", ""),
                             ("block, full lengths", "block, no lengths", "")):
        lo, hi = sorted((med[base], med[base + " again"]))
        verdict = "within the spread or faster" if med[name] <= hi else "SLOWER than the baseline beyond its spread"
        print(f"{name:<52}{med[name]:9.1f} / {lo:.1f}..{hi:.1f} = {med[name] / hi:.3f}..{med[name] / lo:.3f}   {verdict}{note}")
    for name, base, tiles in (("ragged fwd, lengths in [T/4, T]", "ragged fwd, full lengths", fwd_tiles),
                              ("ragged bwd, lengths in [T/4, T]", "ragged bwd, full lengths", bwd_tiles),
                              ("block, lengths in [T/4, T]", "block, full lengths", None)):
        tile = "" if tiles is None else f"   tiles walked {tiles:.2f}"
        print(f"{name:<52}{med[name]:9.1f} / {med[base]:.1f} = {med[name] / med[base]:.3f}{tile}")
    share = med["mask_tail x 2 (out of place + in place)"] / med["block, full lengths"]
    print(f"mask_tail x 2 as a share of the block call with lengths: {med['mask_tail x 2 (out of place + in place)']:.1f} / "
          f"{med['block, full lengths']:.1f} = {100 * share:.1f} %")


if __name__ == "__main__":
    main()
