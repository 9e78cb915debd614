"""One streamed hop of the codec beside what the plain forward offers for the same new frames.

The protocol of tools/causal_conformer_bench.py: one process; every case is captured once as a graph (the Python wrappers and their
allocations are in the capture, not in the replay), warmed up, and replayed once per round between two HIP events, the cases
alternated; median [min .. max] of the per-round microseconds over ROUNDS rounds.  Comparators are listed twice (``again``): the
difference of the two rows is the spread every row has to be read against.

  (a) one ``forward_stream`` step of config S at B in {1, 8}, n in {1, 4} new frames: ring write, 60 step launches, the RVQ, two
      position advances
  (b) ``model.forward`` on a window of 16 + 20 + n + 2 frames -- the encoder's and the decoder's left halos, the new frames and the
      decoder's right halo: what a live user of the plain calls re-runs per hop for the same n frames.  ``--plain-only`` measures
      (b) alone, so that this file runs unchanged in a checkout of the commit before the streaming step (where (a) does not exist)
  (c) per unit of config S (every distinct layer shape), B = 1: the unit's step launches beside the unit's plain call on a window
      of H + n r_in columns

Beside every (a) row: the hop's real time, n * 320 / 24 000 s.

``--counts`` measures the step with per-row frame counts instead, by the same protocol: the uncounted step (twice:
the spread), the counted step with every count full, and the counted step with half of the rows paused (count 0; at B = 1 the one
row).  The counts are device tensors the captured kernels read, so every replay takes the same frames.

``--wire`` measures the RVQ streaming step and its packets, by the same protocol, against the composed launches of
the existing paths: (i) the quantiser alone, ``quantize_bcl`` + ``mask_tail`` + ``codes_pack`` against ``rvq_step_encode``; (ii)
the sender's step, ``encode_stream`` + ``codes_pack`` against ``compress_stream`` -- both with every count full and with half of
the rows paused; (iii) the receiver's quantiser side, ``codes_unpack`` + Q x ``rvq_dequantize`` + a transposition against
``rvq_step_decode``.

``--stages`` measures the ``--wire`` hop with a per-row stage count, by the same protocol at B = 8: the quantiser
alone, the sender's step, the receiver's quantiser side and the relay's ``rvq_packets_restage``, with ``stages=None`` (twice: the
spread) and with a ``stages`` tensor in three settings -- every row at Q, every row at Q / 2, rows mixed over 0 .. Q.

``--wavelet`` measures a streamed decoder hop of the reference default architecture (``CausalVQAE()``: strides 2 3 4 4 5, the second
decoder block a wavelet block), by the same protocol: ``decode_stream`` on a stream made with ``wavelet_blocks=True``
against ``model.decode`` on the decoder's receptive field -- its left halo, the n new frames and the ``flush_frames`` of its delay,
what a live user of the plain call re-runs per hop.  ``--wavelet-steps`` runs 200 eager steps of that stream and nothing else, for
a kernel trace of its own; ``--wavelet-stats CSV`` prints the rows of such a trace's kernel statistics that belong to the stream:

    python tools/codec_stream_bench.py --wavelet > profiles/wavelet_stream.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o wv -- python tools/codec_stream_bench.py --wavelet-steps
    python tools/codec_stream_bench.py --wavelet-stats OUT/.../wv_kernel_stats.csv >> profiles/wavelet_stream.txt

``--multires`` / ``--depthwise`` measure a streamed hop of a model with multires layers (the config-4 model of
tests/test_gpu_blocks.py: strides 2 4 5 8, stereo, one wavelet block, multires layers k = 3, depth = 4 in two encoder and two decoder
blocks) resp. with depthwise residual blocks (config S built with ``depthwise=True``), DESIGN 4.24, by the same protocol at
B in {1, 32}: (b) ``model.forward`` on the receptive field -- what a live user of the plain calls re-runs per hop -- beside (a) the
``forward_stream`` step of a stream made with the keywords and (a0) the step of the same model WITHOUT those units, which is what the
units add to a hop.  ``--multires-steps`` / ``--depthwise-steps`` run 100 eager steps per (B, n) of (a) and of (a0) and nothing
else, for a kernel trace; ``--wavelet-stats CSV`` prints the stream's rows of such a trace too:

    python tools/codec_stream_bench.py --multires > profiles/multires_depthwise_stream.txt
    python tools/codec_stream_bench.py --depthwise >> profiles/multires_depthwise_stream.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o mr -- python tools/codec_stream_bench.py --multires-steps
    python tools/codec_stream_bench.py --wavelet-stats OUT/.../mr_kernel_stats.csv >> profiles/multires_depthwise_stream.txt

    python tools/codec_stream_bench.py [--plain-only] > profiles/codec_stream.txt
    python tools/codec_stream_bench.py --counts > profiles/stream_counts.txt
    python tools/codec_stream_bench.py --wire > profiles/rvq_step.txt
    python tools/codec_stream_bench.py --stages >> profiles/rvq_stages.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audio_generation_amd.vae import CausalVQAE  # noqa: E402

ROUNDS = 9
STEPS_PER_GRAPH = 10
ENC_HALO, DEC_HALO_LEFT, DEC_HALO_RIGHT = 16, 20, 2
SAMPLE_RATE = 24000


def measure(cases, launches):
    """[(name, fn)] -> {name: [microseconds per call, one per round]}."""
    graphs = []
    side = torch.cuda.Stream()
    for _, fn in cases:
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            fn()
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g), torch.no_grad():
            for _ in range(launches):
                fn()
        g.replay()
        graphs.append(g)
    torch.cuda.synchronize()
    times = {name: [] for name, _ in cases}
    for _ in range(ROUNDS):
        for (name, _), g in zip(cases, graphs):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            g.replay()
            stop.record()
            stop.synchronize()
            times[name].append(1e3 * start.elapsed_time(stop) / launches)
    del graphs
    return times


def show(times):
    for name, ts in times.items():
        print(f"  {name:<64}{statistics.median(ts):10.2f} us [{min(ts):10.2f} .. {max(ts):10.2f}]", flush=True)


def config_s(dev):
    torch.manual_seed(0)
    model = CausalVQAE(in_channels=1, n_blocks=4, strides=(2, 4, 5, 8), num_quantizers=8, codebook_size=1024, codebook_dim=512,
                       input_format="n c l", wavelet_decoders=False).eval().to(dev)
    gen = torch.Generator().manual_seed(1234)
    x = (0.1 * torch.randn(2, 1, 72000, generator=gen)).clamp(-1, 1).to(dev)
    with torch.no_grad():
        model.quantizer.init_from_latents(model._run_encoders(model.rearrange_in(x)))
    return model


def counted(model, dev, gen):
    """The step with per-row counts beside the uncounted step, B in {1, 8}, n in {1, 4}."""
    sf = model.scale_factor
    for b in (1, 8):
        for n in (1, 4):
            chunk = (0.1 * torch.randn(b, 1, n * sf, generator=gen)).to(dev)
            full = torch.full((b,), n, dtype=torch.int64, device=dev)
            half = full.clone()
            half[b // 2:] = 0                                                       # B = 1: the one row is paused
            streams = [model.new_stream(b, max_chunk=4) for _ in range(3)]
            plain = lambda: model.forward_stream(chunk, streams[0])                 # noqa: E731
            cases = [("(a) forward_stream step", plain),
                     ("(a) counts=, every row full", lambda: model.forward_stream(chunk, streams[1], counts=full)),
                     (f"(a) counts=, {b - b // 2} of {b} rows paused", lambda: model.forward_stream(chunk, streams[2], counts=half)),
                     ("(a) forward_stream step (again)", plain)]
            times = measure(cases, STEPS_PER_GRAPH)
            print(f"\nB = {b}, n = {n} new frames")
            show(times)
            names = list(times)
            base = min(statistics.median(times[names[0]]), statistics.median(times[names[3]]))
            spread = abs(statistics.median(times[names[0]]) - statistics.median(times[names[3]]))
            print(f"  full counts / uncounted = {statistics.median(times[names[1]]) / base:.3f}; half paused / uncounted = "
                  f"{statistics.median(times[names[2]]) / base:.3f}; the uncounted step against itself: {spread:.2f} us")


def _verdict(times, new, old):
    """A claim holds when the new case's slowest round is below the fastest round of both rows of its comparator."""
    names = list(times)
    rows = [times[n] for n in names if n.startswith(old)]
    assert len(rows) == 2 and new in times, (new, old, names)
    med = [statistics.median(r) for r in rows]
    ok = max(times[new]) < min(rows[0] + rows[1])
    print(f"  {new} / {old} = {statistics.median(times[new]) / min(med):.3f}; comparator against itself: {abs(med[0] - med[1]):.2f} us; "
          f"new's slowest round below the comparator's fastest: {'yes' if ok else 'NO'}")
    return ok


def wire(model, dev, gen):
    """The RVQ streaming step and its packets beside the composed launches they replace, B in {1, 8}, n in {1, 4}:
    (i) the quantiser alone, (ii) the sender's step, (iii) the receiver's quantiser side; full counts and half of the rows paused."""
    from audio_generation_amd import ops, streaming
    sf, bits, quant = model.scale_factor, model._code_bits, model.quantizer
    cbs, q = quant.codebooks.detach(), quant.num_quantizers
    met = {"(i)": [], "(ii)": [], "(iii)": []}
    paused = {}
    for b in (1, 8):
        for n in (1, 4):
            chunk = (0.1 * torch.randn(b, 1, n * sf, generator=gen)).to(dev)
            full = torch.full((b,), n, dtype=torch.int64, device=dev)
            half = full.clone()
            half[b // 2:] = 0                                                       # B = 1: the one row is paused
            with torch.no_grad():                                                   # the latents a step hands its quantiser
                z = {"full": streaming.encode_latents_stream(model, chunk, model.new_stream(b, max_chunk=4), full),
                     "half": streaming.encode_latents_stream(model, chunk, model.new_stream(b, max_chunk=4), half)}
            counts = {"full": full, "half": half}
            tag = {"full": "every row full", "half": f"{b - b // 2} of {b} rows paused"}
            print(f"\nB = {b}, n = {n} new frames")

            def old_q(which):
                zq, index, _ = quant.quantize_bcl(z[which], None, update_codebook=False, prioritize_early=False)
                return ops.mask_tail(zq, None, counts=counts[which]), ops.codes_pack(index, bits)

            cases = []
            for which in ("full", "half"):
                cases += [(f"(i) quantize_bcl + mask_tail + codes_pack, {tag[which]}", lambda which=which: old_q(which)),
                          (f"(i) rvq_step_encode, {tag[which]}",
                           lambda which=which: ops.rvq_step_encode(z[which], cbs, q, None, counts[which], bits))]
            cases += [(name + " (again)", fn) for name, fn in cases[0::2]]
            times = measure(cases, STEPS_PER_GRAPH)
            show(times)
            for which in ("full", "half"):
                ok = _verdict(times, f"(i) rvq_step_encode, {tag[which]}", f"(i) quantize_bcl + mask_tail + codes_pack, {tag[which]}")
                if which == "full":
                    met["(i)"].append(ok)
            paused[(b, n, "(i)")] = (times[f"(i) rvq_step_encode, {tag['half']}"], times[f"(i) rvq_step_encode, {tag['full']}"])

            streams = [model.new_stream(b, max_chunk=4) for _ in range(4)]

            def old_send(s, which):
                _, _, index = model.encode_stream(chunk, s, counts=counts[which])
                return ops.codes_pack(index, bits)

            cases = []
            for i, which in enumerate(("full", "half")):
                cases += [(f"(ii) encode_stream + codes_pack, {tag[which]}", lambda s=streams[2 * i], which=which: old_send(s, which)),
                          (f"(ii) compress_stream, {tag[which]}",
                           lambda s=streams[2 * i + 1], which=which: model.compress_stream(chunk, s, counts=counts[which]))]
            cases += [(name + " (again)", fn) for name, fn in cases[0::2]]
            times = measure(cases, STEPS_PER_GRAPH)
            show(times)
            for which in ("full", "half"):
                ok = _verdict(times, f"(ii) compress_stream, {tag[which]}", f"(ii) encode_stream + codes_pack, {tag[which]}")
                if which == "full":
                    met["(ii)"].append(ok)
            paused[(b, n, "(ii)")] = (times[f"(ii) compress_stream, {tag['half']}"], times[f"(ii) compress_stream, {tag['full']}"])

            with torch.no_grad():
                _, index, packets = ops.rvq_step_encode(z["full"], cbs, q, None, None, bits)
            stream_bytes = ops.codes_pack(index, bits)

            def old_recv():
                idx = ops.codes_unpack(stream_bytes, b * n * q, bits).reshape(b, n, q)
                zq = None
                for i in range(q):
                    zq = ops.rvq_dequantize(cbs[i], idx[..., i], out=zq, accumulate=zq is not None)
                return zq.transpose(1, 2).contiguous()

            cases = [("(iii) codes_unpack + Q x rvq_dequantize + transposition", old_recv),
                     ("(iii) rvq_step_decode", lambda: ops.rvq_step_decode(packets, n, cbs, q, bits)),
                     ("(iii) codes_unpack + Q x rvq_dequantize + transposition (again)", old_recv)]
            times = measure(cases, STEPS_PER_GRAPH)
            show(times)
            met["(iii)"].append(_verdict(times, "(iii) rvq_step_decode", "(iii) codes_unpack + Q x rvq_dequantize + transposition"))
    print("\n(a) full counts, new below old by more than the spread: quantiser alone "
          f"{sum(met['(i)'])} of {len(met['(i)'])} cases, sender's step {sum(met['(ii)'])} of {len(met['(ii)'])} cases")
    for (b, n, what), (h, f) in paused.items():
        if b == 8:
            print(f"(b) B = 8, n = {n}, {what}: 4 rows paused / every row full = {statistics.median(h) / statistics.median(f):.3f} "
                  f"(paused's slowest round at or below full's fastest: {'yes' if max(h) <= min(f) else 'NO'}; median at or below: "
                  f"{'yes' if statistics.median(h) <= statistics.median(f) else 'NO'})")
    print(f"(c) receiver's quantiser side, new below old by more than the spread: {sum(met['(iii)'])} of {len(met['(iii)'])} cases")


def staged(model, dev, gen):
    """The ``--wire`` hop with a ``stages`` tensor, B = 8, n in {1, 4}: the quantiser alone, the sender's step, the
    receiver's quantiser side and the relay's restage, with ``stages=None`` (twice: the spread), every row at Q, every row at Q / 2
    and rows mixed over 0 .. Q.  The stage counts are device tensors the captured kernels read."""
    from audio_generation_amd import ops, streaming
    sf, bits, quant = model.scale_factor, model._code_bits, model.quantizer
    cbs, q = quant.codebooks.detach(), quant.num_quantizers
    b = 8
    settings = {f"every row at Q = {q}": torch.full((b,), q, dtype=torch.int64, device=dev),
                f"every row at Q / 2 = {q // 2}": torch.full((b,), q // 2, dtype=torch.int64, device=dev),
                f"mixed over 0 .. {q}": torch.tensor([(r * q) // (b - 1) for r in range(b)], dtype=torch.int64, device=dev)}
    for n in (1, 4):
        chunk = (0.1 * torch.randn(b, 1, n * sf, generator=gen)).to(dev)
        with torch.no_grad():
            z = streaming.encode_latents_stream(model, chunk, model.new_stream(b, max_chunk=4))
            _, _, packets = ops.rvq_step_encode(z, cbs, q, None, None, bits)
        print(f"\nB = {b}, n = {n} new frames; mixed = {settings[f'mixed over 0 .. {q}'].tolist()}")
        plain_q = lambda: ops.rvq_step_encode(z, cbs, q, None, None, bits)                                     # noqa: E731
        cases = [("(i) rvq_step_encode, stages=None", plain_q)]
        cases += [(f"(i) rvq_step_encode, {tag}", lambda st=st: ops.rvq_step_encode(z, cbs, q, None, None, bits, stages=st))
                  for tag, st in settings.items()]
        cases.append(("(i) rvq_step_encode, stages=None (again)", plain_q))
        show(measure(cases, STEPS_PER_GRAPH))

        streams = [model.new_stream(b, max_chunk=4) for _ in range(1 + len(settings))]
        plain_s = lambda: model.compress_stream(chunk, streams[0])                                             # noqa: E731
        cases = [("(ii) compress_stream, stages=None", plain_s)]
        cases += [(f"(ii) compress_stream, {tag}", lambda s=s, st=st: model.compress_stream(chunk, s, stages=st))
                  for s, (tag, st) in zip(streams[1:], settings.items())]
        cases.append(("(ii) compress_stream, stages=None (again)", plain_s))
        times = measure(cases, STEPS_PER_GRAPH)
        show(times)
        names = list(times)
        base = min(statistics.median(times[names[0]]), statistics.median(times[names[-1]]))
        print("  " + "; ".join(f"{name.split(', ', 1)[1]} / stages=None = {statistics.median(times[name]) / base:.3f}" for name in names[1:-1])
              + f"; stages=None against itself: {abs(statistics.median(times[names[0]]) - statistics.median(times[names[-1]])):.2f} us")

        plain_r = lambda: ops.rvq_step_decode(packets, n, cbs, q, bits)                                        # noqa: E731
        cases = [("(iii) rvq_step_decode, stages=None", plain_r)]
        with torch.no_grad():
            sent = {tag: ops.rvq_step_encode(z, cbs, q, None, None, bits, stages=st)[2] for tag, st in settings.items()}
        cases += [(f"(iii) rvq_step_decode, {tag}", lambda tag=tag, st=st: ops.rvq_step_decode(sent[tag], n, cbs, q, bits, stages=st))
                  for tag, st in settings.items()]
        cases += [(f"(iv) rvq_packets_restage from Q, {tag}", lambda st=st: ops.rvq_packets_restage(packets, n, q, bits, st))
                  for tag, st in settings.items()]
        cases.append(("(iii) rvq_step_decode, stages=None (again)", plain_r))
        show(measure(cases, STEPS_PER_GRAPH))


def default_architecture(dev):
    torch.manual_seed(0)
    model = CausalVQAE(input_format="n c l").eval().to(dev)
    return model


def _decoder_left_halo(plan):
    """Frames before the chunk that the decoder's newest outputs depend on: every unit's reach, in frames, summed."""
    cols = sum((u.reach + u.reach_h) / u.rate_in for u in plan.decoders)
    return int(-(-cols // 1))


def wavelet(dev, gen):
    """A streamed decoder hop of the reference default architecture beside the plain decoder on its receptive field."""
    from audio_generation_amd import ops, streaming
    model = default_architecture(dev)
    sf = model.scale_factor
    plan = streaming.plan(model, 4, wavelet_blocks=True)
    dim = plan.decoders[0].c_in
    left, right = _decoder_left_halo(plan), plan.flush_frames
    w = next(u for u in plan.decoders if u.kind == "wavelet")
    print(f"decoder: delay {plan.decoder_delay} samples, flush {right} frames, left halo {left} frames; wavelet block "
          f"{w.c_in} -> {w.hidden} -> {w.c_out}, k_in {w.k}, s {w.s}, k_out {w.k_out} at {w.rate_in} columns per frame")
    for n in (1, 4):
        print(f"  n = {n}: in-step {ops.wavelet_stream_in_kernel_name(w.c_in, w.hidden, w.k, n, w.rate_in)}, out-step "
              f"{ops.wavelet_stream_out_kernel_name(w.hidden, w.c_out, w.k_out, w.s, n, w.rate_in)}")
    verdicts = []
    for b in (1, 8):
        for n in (1, 4):
            frames = left + n + right
            window = torch.randn(b, dim, frames, generator=gen).to(dev)
            chunk = window[:, :, :n].contiguous()
            stream = model.new_stream(b, max_chunk=4, wavelet_blocks=True)
            plain = lambda: model.decode(window)                                    # noqa: E731
            cases = [(f"(b) model.decode on {frames} frames", plain),
                     ("(a) decode_stream step", lambda: model.decode_stream(chunk, stream)),
                     (f"(b) model.decode on {frames} frames (again)", plain)]
            times = measure(cases, STEPS_PER_GRAPH)
            print(f"\nB = {b}, n = {n} new frames: the hop lasts {1e6 * n * sf / SAMPLE_RATE:.0f} us of audio")
            show(times)
            names = list(times)
            a, b1, b2 = times[names[1]], times[names[0]], times[names[2]]
            ok = max(a) < min(b1 + b2)
            verdicts.append(ok)
            print(f"  (b) / (a) = {min(statistics.median(b1), statistics.median(b2)) / statistics.median(a):.2f}; (a)'s slowest round "
                  f"below (b)'s fastest: {'yes' if ok else 'NO'}")
    print(f"\n(a) below (b) by more than the spread: {sum(verdicts)} of {len(verdicts)} cases")

    # the in-step shares its kernel instance with other layers of the stack, so a kernel-statistics table cannot tell it apart:
    # the block's two launches on their own, and the plain layer on the columns a hop would re-run
    print("\n(c) the wavelet block alone: its two step launches | the plain layer on reach + n r_in columns")
    i = plan.decoders.index(w)
    unit = model._units("decoders")[i]
    layer = unit.layer
    img_in = streaming.packed_image(layer.conv_in, "conv_stream_pack", streaming.CONV_SAME)
    img_out = streaming.packed_image(layer.conv_out, "conv_stream_pack", streaming.CONV_SAME)
    table = streaming.fold_table(layer)
    for b in (1, 8):
        for n in (1, 4):
            ring = torch.randn(b, w.c_in, w.cap, generator=gen).to(dev)
            hid = torch.randn(b, w.hidden, w.cap_h, generator=gen).to(dev)
            dst = torch.empty(b, w.c_out, n * w.rate_out, device=dev)
            pos = torch.full((b,), 1000, dtype=torch.int64, device=dev)
            end = torch.full((b,), ops.STREAM_LIVE, dtype=torch.int64, device=dev)
            window = torch.randn(b, w.c_in, w.reach + w.reach_h + n * w.rate_in, generator=gen).to(dev)
            cases = [("plain wavelet layer", lambda: unit.forward(window)),
                     ("in-step", lambda: ops.wavelet_stream_in_step(w.c_in, w.hidden, w.k, img_in, layer.conv_in.bias.detach(), ring, hid,
                                                                    pos, end, n, w.rate_in, w.delay_in)),
                     ("out-step", lambda: ops.wavelet_stream_out_step(w.hidden, w.c_out, w.k_out, w.s, img_out, layer.conv_out.bias.detach(),
                                                                      table, hid, dst, pos, end, n, w.rate_in, w.delay_h, dst_ring=False,
                                                                      epilogue=streaming.EPI_LEAKY_PRE, slope=unit.slope or 0.0)),
                     ("plain wavelet layer (again)", lambda: unit.forward(window))]
            times = measure(cases, 20)
            print(f"B = {b}, n = {n}")
            show(times)


def wavelet_steps(dev, gen):
    """200 eager steps per (B, n) of the streamed decoder and nothing else: the body of a kernel trace."""
    model = default_architecture(dev)
    from audio_generation_amd import streaming
    dim = streaming.plan(model, 4, wavelet_blocks=True).decoders[0].c_in
    with torch.no_grad():
        for b in (1, 8):
            for n in (1, 4):
                stream = model.new_stream(b, max_chunk=4, wavelet_blocks=True)
                chunk = torch.randn(b, dim, n, generator=gen).to(dev)
                for _ in range(200):
                    model.decode_stream(chunk, stream)
    torch.cuda.synchronize()
    print("800 decode_stream steps: B in {1, 8} x n in {1, 4}, 200 each")


def wavelet_stats(path):
    """The rows of a kernel-statistics CSV (Name, Calls, TotalDurationNs, AverageNs, ...) that belong to the streamed decoder."""
    import csv
    rows = [r for r in csv.DictReader(open(path)) if any(k in r["Name"] for k in ("conv_stream_kernel", "wavelet", "ring_write_rate",
                                                                                  "stream_advance", "multires_stream"))]
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    print("\nkernel statistics of the eager steps of a stream; template arguments <KS, NT, CNT, FOLD, AFF>: FOLD = true is the wavelet "
          "out-step, AFF = true the dilated conv of a depthwise block")
    print(f"  {'calls':>7} {'average us':>11} {'min us':>9} {'max us':>9}  kernel")
    for r in rows:
        print(f"  {int(r['Calls']):>7} {float(r['AverageNs']) / 1e3:>11.2f} {float(r['MinNs']) / 1e3:>9.2f} {float(r['MaxNs']) / 1e3:>9.2f}  "
              f"{r['Name'][:150]}")


CONFIG4 = dict(in_channels=2, n_blocks=4, strides=(2, 4, 5, 8), num_quantizers=2, codebook_size=64, codebook_dim=512, input_format="n c l",
               wavelet_decoders=[False, True, False, False])
CONFIG4_MULTIRES = dict(multires_encoders=[True, False, True, False], multires_decoders=[False, False, True, True], multires_kernel_size=3,
                        multires_depth=4)
CONFIG_S = dict(in_channels=1, n_blocks=4, strides=(2, 4, 5, 8), num_quantizers=8, codebook_size=1024, codebook_dim=512,
                input_format="n c l", wavelet_decoders=False)
UNIT_BATCHES = (1, 32)


def _unit_models(which, dev):
    """(model with the units, the same model without them, the keywords of their streams) for ``which`` in "multires" / "depthwise"."""
    base, extra = (CONFIG4, CONFIG4_MULTIRES) if which == "multires" else (CONFIG_S, dict(depthwise=True))
    models = []
    for kw in (dict(base, **extra), base):
        torch.manual_seed(0)
        model = CausalVQAE(**kw).eval().to(dev)
        x = (0.1 * torch.randn(2, base["in_channels"], 36000, generator=torch.Generator().manual_seed(1234))).clamp(-1, 1).to(dev)
        with torch.no_grad():
            model.quantizer.init_from_latents(model._run_encoders(model.rearrange_in(x)))
        models.append(model)
    return models[0], models[1], dict(wavelet_blocks=True, multires_layers=True, depthwise_blocks=True), dict(wavelet_blocks=True)


def unit_hop(which, dev, gen):
    """A streamed hop of a model with multires layers / depthwise blocks beside the plain forward on its receptive field and beside
    the streamed hop of the same model without those units."""
    from audio_generation_amd import streaming
    model, bare, kw, kw0 = _unit_models(which, dev)
    sf, c = model.scale_factor, model.in_channels
    plan, plan0 = streaming.plan(model, 4, **kw), streaming.plan(bare, 4, **kw0)
    enc_left = -(-plan.enc_left // sf)
    left, right = _decoder_left_halo(plan), plan.flush_frames
    mine = [u for u in (*plan.encoders, *plan.decoders) if u.kind in ("multires", "resdw")]
    launches = lambda p: sum(2 if u.kind in ("res", "resdw", "wavelet") else 1 for u in (*p.encoders, *p.decoders))     # noqa: E731
    print(f"{which}: {len(mine)} such units; encoder left halo {enc_left} frames, decoder left halo {left}, right {right}; step launches "
          f"per hop {launches(plan)} with the units, {launches(plan0)} without")
    if which == "multires":
        for u in mine:
            print(f"  multires C={u.c_in} k={u.k} depth={u.depth} reach {u.reach} at {u.rate_in} columns per frame, delay {u.delay_in}")
    verdicts = []
    for b in UNIT_BATCHES:
        for n in (1, 4):
            frames = enc_left + left + n + right
            window = (0.1 * torch.randn(b, c, frames * sf, generator=gen)).to(dev)
            chunk = window[:, :, :n * sf].contiguous()
            stream, stream0 = model.new_stream(b, max_chunk=4, **kw), bare.new_stream(b, max_chunk=4, **kw0)
            plain = lambda: model(window)                                           # noqa: E731
            cases = [(f"(b) model.forward on {frames} frames", plain),
                     ("(a) forward_stream step", lambda: model.forward_stream(chunk, stream)),
                     ("(a0) forward_stream step, the model without the units", lambda: bare.forward_stream(chunk, stream0)),
                     (f"(b) model.forward on {frames} frames (again)", plain)]
            times = measure(cases, STEPS_PER_GRAPH)
            print(f"\nB = {b}, n = {n} new frames: the hop lasts {1e6 * n * sf / SAMPLE_RATE:.0f} us of audio")
            show(times)
            names = list(times)
            b1, a, a0, b2 = (times[k] for k in names)
            ok = max(a) < min(b1 + b2)
            verdicts.append(ok)
            print(f"  (b) / (a) = {min(statistics.median(b1), statistics.median(b2)) / statistics.median(a):.2f}; (a)'s slowest round below "
                  f"(b)'s fastest: {'yes' if ok else 'NO'}; (a) - (a0) = {statistics.median(a) - statistics.median(a0):.2f} us for "
                  f"{launches(plan) - launches(plan0)} more launches")
    print(f"\n(a) below (b) by more than the spread: {sum(verdicts)} of {len(verdicts)} cases")


def unit_steps(which, dev, gen):
    """100 eager steps per (B, n) of the stream with the units and of the one without, and nothing else: the body of a kernel trace."""
    model, bare, kw, kw0 = _unit_models(which, dev)
    sf, c = model.scale_factor, model.in_channels
    with torch.no_grad():
        for b in UNIT_BATCHES:
            for n in (1, 4):
                chunk = (0.1 * torch.randn(b, c, n * sf, generator=gen)).to(dev)
                for m, k in ((model, kw), (bare, kw0)):
                    stream = m.new_stream(b, max_chunk=4, **k)
                    for _ in range(100):
                        m.forward_stream(chunk, stream)
    torch.cuda.synchronize()
    print(f"{which}: 100 forward_stream steps per (B, n), B in {UNIT_BATCHES} x n in (1, 4), with the units and without")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-only", action="store_true", help="measure (b) alone (a checkout without the streaming step)")
    ap.add_argument("--counts", action="store_true", help="the step with per-row frame counts beside the uncounted step")
    ap.add_argument("--wire", action="store_true", help="the RVQ streaming step and its packets beside the composed launches")
    ap.add_argument("--stages", action="store_true", help="the --wire hop with a per-row stage count: all Q, all Q / 2, mixed")
    ap.add_argument("--wavelet", action="store_true", help="a streamed decoder hop of the reference default architecture (wavelet block)")
    ap.add_argument("--wavelet-steps", action="store_true", help="eager steps of that stream only: the body of a kernel trace")
    ap.add_argument("--wavelet-stats", metavar="CSV", help="print the stream's rows of a kernel-statistics CSV; needs no GPU")
    for which in ("multires", "depthwise"):
        ap.add_argument(f"--{which}", action="store_true", help=f"a streamed hop of a model with {which} units (DESIGN 4.24)")
        ap.add_argument(f"--{which}-steps", action="store_true", help="eager steps of those streams only: the body of a kernel trace")
    args = ap.parse_args()
    if args.wavelet_stats is not None:
        wavelet_stats(args.wavelet_stats)
        return
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda"
    for which in ("multires", "depthwise"):
        if getattr(args, which) or getattr(args, which + "_steps"):
            gen = torch.Generator().manual_seed(0)
            if getattr(args, which + "_steps"):
                unit_steps(which, dev, gen)
                return
            print(f"device: {torch.cuda.get_device_name(0)}; per-call time over {ROUNDS} replays of a graph of {STEPS_PER_GRAPH} back-to-back "
                  f"calls (median [min .. max]); --{which}")
            unit_hop(which, dev, gen)
            return
    if args.wavelet or args.wavelet_steps:
        gen = torch.Generator().manual_seed(0)
        if args.wavelet_steps:
            wavelet_steps(dev, gen)
            return
        print(f"device: {torch.cuda.get_device_name(0)}; reference default architecture; per-call time over {ROUNDS} replays of a graph "
              f"of {STEPS_PER_GRAPH} back-to-back calls (median [min .. max]); --wavelet")
        wavelet(dev, gen)
        return
    model = config_s(dev)
    sf = model.scale_factor
    gen = torch.Generator().manual_seed(0)
    if args.wire:
        print(f"device: {torch.cuda.get_device_name(0)}; config S; per-call time over {ROUNDS} replays of a graph of {STEPS_PER_GRAPH} "
              "back-to-back calls (median [min .. max]); --wire")
        wire(model, dev, gen)
        return
    if args.stages:
        print(f"device: {torch.cuda.get_device_name(0)}; config S; per-call time over {ROUNDS} replays of a graph of {STEPS_PER_GRAPH} "
              "back-to-back calls (median [min .. max]); --stages")
        staged(model, dev, gen)
        return
    if args.counts:
        print(f"device: {torch.cuda.get_device_name(0)}; config S; per-call time over {ROUNDS} replays of a graph of {STEPS_PER_GRAPH} "
              "back-to-back calls (median [min .. max]); --counts")
        counted(model, dev, gen)
        return
    print(f"device: {torch.cuda.get_device_name(0)}; config S; per-call time over {ROUNDS} replays of a graph of {STEPS_PER_GRAPH} "
          f"back-to-back calls (median [min .. max]){'; --plain-only' if args.plain_only else ''}")
    verdicts = []
    for b in (1, 8):
        for n in (1, 4):
            frames = ENC_HALO + DEC_HALO_LEFT + n + DEC_HALO_RIGHT
            window = (0.1 * torch.randn(b, 1, frames * sf, generator=gen)).to(dev)
            plain = lambda: model(window)                                           # noqa: E731
            cases = [(f"(b) model.forward on {frames} frames", plain)]
            if not args.plain_only:
                chunk = window[:, :, :n * sf].contiguous()
                stream = model.new_stream(b, max_chunk=4)
                cases.append(("(a) forward_stream step", lambda: model.forward_stream(chunk, stream)))
            cases.append((f"(b) model.forward on {frames} frames (again)", plain))
            times = measure(cases, STEPS_PER_GRAPH)
            print(f"\nB = {b}, n = {n} new frames: the hop lasts {1e6 * n * sf / SAMPLE_RATE:.0f} us of audio")
            show(times)
            if not args.plain_only:
                names = list(times)
                a, b1, b2 = times[names[1]], times[names[0]], times[names[2]]
                ok = max(a) < min(b1 + b2)
                verdicts.append(ok)
                print(f"  (b) / (a) = {min(statistics.median(b1), statistics.median(b2)) / statistics.median(a):.2f}; (a)'s slowest round "
                      f"below (b)'s fastest: {'yes' if ok else 'NO'}")
    if args.plain_only:
        return
    print(f"\nacceptance (a) below (b) by more than the spread: {sum(verdicts)} of {len(verdicts)} cases")

    from audio_generation_amd import streaming
    print("\n(c) per unit, B = 1: the unit's step launches | the unit's plain call on H + n r_in columns")
    losers = []
    for n in (1, 4):
        plan = streaming.plan(model, n)
        seen = set()
        for which, plans in (("encoders", plan.encoders), ("decoders", plan.decoders)):
            for u, p in zip(model._units(which), plans):
                key = (p.kind, p.c_in, p.c_out, p.k, p.s, p.d, p.rate_in)
                if key in seen:
                    continue
                seen.add(key)
                ring = torch.randn(1, p.c_in, p.cap, generator=gen).to(dev)
                dst = torch.empty(1, p.c_out, n * p.rate_out, device=dev)
                pos = torch.full((1,), 1000, dtype=torch.int64, device=dev)
                window = torch.randn(1, p.c_in, p.reach + n * p.rate_in, generator=gen).to(dev)
                plain = (lambda u=u, window=window: u.layer(window) if u.bare else u.forward(window))
                step = (lambda u=u, p=p, ring=ring, dst=dst, pos=pos: streaming.run_unit(u, p, ring, dst, False, pos, None, n))
                label = f"{p.kind}({p.c_in}->{p.c_out}, k{p.k} s{p.s} d{p.d}) r_in {p.rate_in} n {n}"
                times = measure([(f"plain {label}", plain), (f"step  {label}", step), (f"plain {label} (again)", plain)], 20)
                show(times)
                names = list(times)
                if statistics.median(times[names[1]]) > max(times[names[0]] + times[names[2]]):
                    losers.append(label)
    print(f"\nunits where the step's median is above every round of the plain call: {len(losers)}")
    for label in losers:
        print(f"  {label}")


if __name__ == "__main__":
    main()
