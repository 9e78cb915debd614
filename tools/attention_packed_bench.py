"""Packed variable-length batches beside the padded ``lengths=`` path of the same build (informational, no gate).

The protocol of tools/attention_ragged_bench.py: one process, HIP events, warm-up calls per case, then ROUNDS rounds; in every
round each case is timed over its CALLS back-to-back calls between two events, the cases alternated; median / min / max of the
per-round microseconds per call (the Python wrapper, which allocates outputs and workspace per call, included).  Every baseline
is listed twice (``again``): the two rows were measured in the same run, alternated with everything else, and their difference
is the run-to-run spread a packed row has to be read against.

Cases, at the config-3 shape B = 32, dim 512, H = 8, Dh = 64, T = 225, depth 1, with lengths full and with lengths drawn
uniformly in [T/4, T] (seeded, the draw of tools/attention_ragged_bench.py):
1. the one-layer block forward (eval, no_grad), ``run_packed`` on the (1, 512, N) batch against ``run_bct(lengths=)`` on the
   (32, 512, 225) one -- host partitions (no slack, no mask launch) and, for the short lengths, a device partition too (the two
   slack masks);
2. the same block forward + backward (train mode, dropout 0, input and parameter gradients);
3. the attention kernels alone, ``attention_alibi_packed`` / ``_backward`` against ``attention_alibi_ragged`` / ``_backward`` on
   one qkv tensor, next to the share of the launched workgroups that find nothing to do (the packed grid is sized by
   max_len for every sequence);
4. ``pack_rows`` + ``unpack_rows`` of the (32, 512, 225) activations, what a caller who holds padded data pays to convert.

    python tools/attention_packed_bench.py > profiles/attention_packed.txt
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audio_generation_amd import ops  # noqa: E402
from audio_generation_amd.transformers import Transformer, pack_padded  # noqa: E402

B, H, DH, T = 32, 8, 64, 225
DIM = H * DH
ROUNDS = 5


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda"
    gen = torch.Generator().manual_seed(0)
    slopes = (2.0 ** (-8.0 / torch.arange(H, 0, -1))).to(dev)
    attn = dict(heads=H, head_dim=DH, scale_div=DH ** 0.5)
    qkv = (0.7 * torch.randn(B, 3 * DIM, T, generator=gen)).to(dev)
    dout = torch.randn(B, DIM, T, generator=gen).to(dev)
    gen2 = torch.Generator().manual_seed(0)          # the draw of tools/attention_ragged_bench.py: same stream position
    for shape in ((B, DIM, T), (B, 2 * DIM, T), (B, DIM, T)):
        torch.randn(shape, generator=gen2)
    drawn = torch.randint(T // 4, T + 1, (B,), generator=gen2)
    lens = {"full": [T] * B, "short": drawn.tolist()}

    cases = []          # (name, fn, calls per round, warm-up calls)

    def add(name, fn, calls, warm):
        cases.append((name, fn, calls, warm))

    torch.manual_seed(0)
    tf = Transformer(DIM, depth=1, heads=H, head_dim=DH, context_x=T).to(dev)
    x = torch.randn(B, DIM, T, generator=gen).to(dev)
    w = torch.randn(B, DIM, T, generator=gen).to(dev)
    packed = {}
    for key, ln in lens.items():
        ldev = torch.tensor(ln, dtype=torch.int32, device=dev)
        xp, cu, max_len = pack_padded(x, ln)
        wp = ops.pack_rows(w, cu, xp.shape[-1])
        qp = ops.pack_rows(qkv, cu, xp.shape[-1])
        dp = ops.pack_rows(dout, cu, xp.shape[-1])
        packed[key] = dict(ldev=ldev, xp=xp, wp=wp, cu=cu, cu_host=cu.tolist(), max_len=max_len, qkv=qp, dout=dp, n=xp.shape[-1])
    with torch.no_grad():
        tf.eval()
        a = tf.run_packed(packed["short"]["xp"], packed["short"]["cu_host"])
        b = ops.pack_rows(tf.run_bct(x, lengths=packed["short"]["ldev"]), packed["short"]["cu"], packed["short"]["n"])
    print(f"# run_packed against run_bct(lengths=) on the padded batch, lengths in [T/4, T]: max difference {float((a - b).abs().max()):.3e}")

    def fwd_padded(key):
        def fn():
            tf.eval()
            with torch.no_grad():
                tf.run_bct(x, lengths=packed[key]["ldev"])
        return fn

    def fwd_packed(key, device=False):
        p = packed[key]

        def fn():
            tf.eval()
            with torch.no_grad():
                if device:
                    tf.run_packed(p["xp"], p["cu"], max_len=p["max_len"])
                else:
                    tf.run_packed(p["xp"], p["cu_host"])
        return fn

    def train_padded(key):
        xg = x.clone().requires_grad_()

        def fn():
            tf.train()
            tf.run_bct(xg, lengths=packed[key]["ldev"]).backward(w)
        return fn

    def train_packed(key):
        p = packed[key]
        xg = p["xp"].clone().requires_grad_()

        def fn():
            tf.train()
            tf.run_packed(xg, p["cu_host"]).backward(p["wp"])
        return fn

    for key, label in (("full", "full lengths"), ("short", "lengths in [T/4, T]")):
        add(f"block fwd, padded lengths=, {label}", fwd_padded(key), 50, 5)
        add(f"block fwd, packed, {label}", fwd_packed(key), 50, 5)
        if key == "short":
            add(f"block fwd, packed, device cu, {label}", fwd_packed(key, True), 50, 5)
        add(f"block fwd, padded lengths=, {label} again", fwd_padded(key), 50, 0)
    for key, label in (("full", "full lengths"), ("short", "lengths in [T/4, T]")):
        add(f"block fwd+bwd, padded lengths=, {label}", train_padded(key), 20, 3)
        add(f"block fwd+bwd, packed, {label}", train_packed(key), 20, 3)
        add(f"block fwd+bwd, padded lengths=, {label} again", train_padded(key), 20, 0)

    outs = {}
    for key, label in (("full", "full lengths"), ("short", "lengths in [T/4, T]")):
        p = packed[key]
        outs[key, "r"] = ops.attention_alibi_ragged(qkv, None, slopes, **attn, q_len=p["ldev"], k_len=p["ldev"])
        outs[key, "p"] = ops.attention_alibi_packed(p["qkv"], None, slopes, **attn, cu_q=p["cu"], max_q=p["max_len"])
        rag_f = lambda p=p: ops.attention_alibi_ragged(qkv, None, slopes, **attn, q_len=p["ldev"], k_len=p["ldev"])                  # noqa: E731
        rag_b = lambda p=p, o=outs[key, "r"]: ops.attention_alibi_ragged_backward(qkv, None, slopes, o, dout, **attn, q_len=p["ldev"],  # noqa: E731
                                                                                   k_len=p["ldev"])
        add(f"ragged fwd, {label}", rag_f, 200, 20)
        add(f"packed fwd, {label}", lambda p=p: ops.attention_alibi_packed(p["qkv"], None, slopes, **attn, cu_q=p["cu"], max_q=p["max_len"]),
            200, 20)
        add(f"ragged fwd, {label} again", rag_f, 200, 0)
        add(f"ragged bwd, {label}", rag_b, 50, 5)
        add(f"packed bwd, {label}", lambda p=p, o=outs[key, "p"]: ops.attention_alibi_packed_backward(
            p["qkv"], None, slopes, o, p["dout"], **attn, cu_q=p["cu"], max_q=p["max_len"]), 50, 5)
        add(f"ragged bwd, {label} again", rag_b, 50, 0)
    ps = packed["short"]
    add("pack_rows + unpack_rows, (32, 512, 225), lengths in [T/4, T]",
        lambda: ops.unpack_rows(ops.pack_rows(x, ps["cu"], ps["n"]), ps["cu"], T), 200, 20)

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
    print(f"# HIP-event times, us per call (wrapper included), B={B} dim={DIM} H={H} Dh={DH} T={T} depth 1, fp32; {ROUNDS} rounds, "
          "cases alternated")
    print(f"# lengths drawn in [{T // 4}, {T}]: {lens['short']}")
    print(f"# columns: padded B*T = {B * T}, packed N = {packed['short']['n']} ({packed['short']['n'] / (B * T):.3f} of the padded batch)")
    print(f"# {'case':<66}{'calls':>7}{'median':>11}{'min':>11}{'max':>11}")
    med = {}
    for name, _, calls, _ in cases:
        ts = times[name]
        med[name] = statistics.median(ts)
        print(f"{name:<68}{calls:7d}{med[name]:11.1f}{min(ts):11.1f}{max(ts):11.1f}", flush=True)

    cd = lambda a, b: -(-a // b)                                                                                     # noqa: E731
    print("# packed / baseline (the two baseline medians span its spread)")
    for label in ("full lengths", "lengths in [T/4, T]"):
        pairs = [(f"block fwd, packed, {label}", f"block fwd, padded lengths=, {label}"),
                 (f"block fwd+bwd, packed, {label}", f"block fwd+bwd, padded lengths=, {label}"),
                 (f"packed fwd, {label}", f"ragged fwd, {label}"), (f"packed bwd, {label}", f"ragged bwd, {label}")]
        if label != "full lengths":
            pairs.insert(1, (f"block fwd, packed, device cu, {label}", f"block fwd, padded lengths=, {label}"))
        for name, base in pairs:
            lo, hi = sorted((med[base], med[base + " again"]))
            print(f"{name:<68}{med[name]:9.1f} / {lo:.1f}..{hi:.1f} = {med[name] / hi:.3f}..{med[name] / lo:.3f}")
    ln, mx = lens["short"], max(lens["short"])
    for what, blk in (("forward (128 queries)", 128), ("backward dq / stats (16 queries)", 16), ("backward dkv (64 keys)", 64)):
        launched, busy = B * cd(mx, blk), sum(cd(n, blk) for n in ln)
        print(f"# packed {what}: {launched - busy} of {launched} sequence workgroups per head find nothing to do "
              f"({100 * (launched - busy) / launched:.1f} %); + {cd(mx, blk)} slack workgroups per head")


if __name__ == "__main__":
    main()
