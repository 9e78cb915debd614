#!/usr/bin/env python3
"""In-process A/B timing of libagx kernels on the config-S layer shapes.

Interleaves the variants round-robin (cdna guide rule 24: perf deltas come from
interleaved rounds in ONE process on ONE device) and prints median / min per
variant.  usage: ab_bench.py knob v0 v1 [...]   e.g.  ab_bench.py resblock_res_lds 0 1

``ab_bench.py rb_q4 0 1`` compares the channel-quad layout between residual blocks (include/agx.h): per (C, d) the block alone,
standard layout (0) against input and output in quads (1, a direct ``resblock_forward_q4`` call on a quad tensor), and per C the
stage of three blocks d = 1, 3, 9 through the model's unit walk with the knob at 0 and 1.  Each line also gives the min-max
spread of each variant's repeats: a difference inside it is not a difference.
"""
import ctypes
import statistics
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from audio_generation_amd import _lib, ops  # noqa: E402
from audio_generation_amd.vae import CausalResidualBlock1d  # noqa: E402


def time_fn(fn, reps=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def report(tag, knob, res, flops):
    print(tag + ": " + "  ".join(
        f"{knob}={v}: med {statistics.median(r):7.1f} us min {min(r):7.1f} max {max(r):7.1f} ({flops / statistics.median(r) * 1e-6:5.1f} TF)"
        for v, r in res.items()), flush=True)


def quads(lib, shapes, values, dev="cuda", rounds=9):
    """rb_q4: the block alone per (C, d), then the three-block stage per C."""
    from audio_generation_amd.vae import CausalEncoderBlock, _run_units
    for c, length in shapes:
        blk = CausalEncoderBlock(c, 2 * c, 2).to(dev).eval()
        units = [u for layer, act in list(blk.layers)[:3] for u in layer.units(act)]
        x = torch.randn(32, c, length, device=dev)
        xq = x.reshape(32, c // 4, 4, length).permute(0, 1, 3, 2).contiguous()
        lib.agx_set_tuning(b"rb_q4", 1)
        have = units[0].layer.takes_quads(x.shape, 0.1)
        flops = 2.0 * 32 * c * c * 8 * length
        with torch.no_grad():
            for u in units:
                m = u.layer
                fns = {0: lambda: m.run(x, 0.1), 1: (lambda: m.run_quads(xq, 0.1, True, True)) if have else None}
                res = {v: [] for v in values if fns[v] is not None}
                for _ in range(rounds):
                    for v in res:
                        fns[v]()
                        res[v].append(time_fn(fns[v]))
                report(f"C={c:3d} d={m.conv1.dilation} L={length} block" + ("" if have else " (row opted out)"), "rb_q4", res, flops)
            res = {v: [] for v in values}
            for _ in range(rounds):
                for v in values:
                    lib.agx_set_tuning(b"rb_q4", v)
                    _run_units(units, x)
                    res[v].append(time_fn(lambda: _run_units(units, x)))
            report(f"C={c:3d} d=1,3,9 L={length} stage", "rb_q4", res, 3 * flops)
    lib.agx_set_tuning(b"rb_q4", 1)


def main():
    knob, values = sys.argv[1], [int(v) for v in sys.argv[2:]]
    lib = _lib.load()
    dev = "cuda"
    shapes = [(32, 72000), (64, 36000), (128, 9000), (256, 1800)]
    if knob == "rb_q4":
        return quads(lib, shapes, values)
    for c, length in shapes:
        for d in (1, 9):
            m = CausalResidualBlock1d(c, c, dilation=d).to(dev).eval()
            if __import__("os").environ.get("AGX_BF16X3") == "1":
                m.conv1.impl = m.conv2.impl = _lib.IMPL_MFMA_BF16X3
            x = torch.randn(32, c, length, device=dev)
            with torch.no_grad():
                m.run(x, 0.1)
            res = {v: [] for v in values}
            for _ in range(7):
                for v in values:
                    lib.agx_set_tuning(knob.encode(), v)
                    with torch.no_grad():
                        res[v].append(time_fn(lambda: m.run(x, 0.1)))
            flops = 2.0 * 32 * c * c * 8 * length
            print(f"C={c:3d} d={d} L={length}: " + "  ".join(
                f"{knob}={v}: med {statistics.median(r):7.1f} us min {min(r):7.1f} ({flops / statistics.median(r) * 1e-6:5.1f} TF)"
                for v, r in res.items()), flush=True)
    lib.agx_set_tuning(knob.encode(), values[-1])


if __name__ == "__main__":
    main()
