"""The shared checks of the code path on the host (no kernel is launched, no library is loaded): the refusals of
``ops._stage_sizes`` and ``ops._checked_rows``, of the three step helpers of ``streaming``, and -- the order of refusals being
behaviour -- the FIRST refusal of every public packet entry when two faults are present at once, as literals recorded from the
code before the helpers were shared."""
import pytest
import torch

from audio_generation_amd import ops, streaming
from audio_generation_amd._lib import AgxError
from audio_generation_amd.entropy import PriorCoder
from audio_generation_amd.prior import CodePrior
from tests.test_codec_stream_cpu import _model

I64 = torch.int64


# ------------------------------------------------------------------------------------------------- 1. ops
def test_stage_sizes_refusals():
    arr = ops._stage_sizes("op", (16, 5, 1), 3, 16)
    assert list(arr) == [16, 5, 1] and ops._stage_sizes("op", None, 3, 16) is None
    assert ops._arr_ptr(None) is None and ops._arr_ptr(arr).value
    for sizes, n_q, k, message in (((16, 5), 3, 16, r"op: sizes \[16, 5\] for 3 stages of at most 16 codes"),            # the wrong length
                                   ((16, 0, 4), 3, 16, r"op: sizes \[16, 0, 4\] for 3 stages of at most 16 codes"),     # a size of 0
                                   ((16, 17, 4), 3, 16, r"op: sizes \[16, 17, 4\] for 3 stages of at most 16 codes"),   # K + 1
                                   ([4] * 65, 65, 16, "op: at most 64 stages, got 65"),
                                   (None, 65, 16, "op: at most 64 stages, got 65")):
        with pytest.raises(AgxError, match=message):
            ops._stage_sizes("op", sizes, n_q, k)


BAD_ROWS = ((torch.zeros(2, dtype=torch.int32), "{name} must be a contiguous int64 device tensor of 2 entries (one {per} per batch row), "
                                                "got (2,) torch.int32"),
            (torch.zeros(3, dtype=I64), "{name} must be a contiguous int64 device tensor of 2 entries (one {per} per batch row), "
                                        "got (3,) torch.int64"),
            (torch.zeros(4, dtype=I64)[::2], "{name} is not contiguous (stride (2,)): the kernels read 2 adjacent int64"),
            (torch.zeros(2, dtype=I64, device="meta"), "{name} is on 'meta', the stream on 'cpu'"))


def _message(call) -> str:
    with pytest.raises((AgxError, NotImplementedError)) as e:
        call()
    return f"{type(e.value).__name__}: {e.value}"


def test_checked_rows_refusals():
    cpu, good = torch.device("cpu"), torch.zeros(2, dtype=I64)
    assert ops._checked_rows("op", 2, cpu) == (None, None)
    c, s = ops._checked_rows("op", 2, cpu, good, good, on="the stream on")
    assert c is good and s is good
    for bad, message in BAD_ROWS:
        want_c = "AgxError: op: " + message.format(name="counts", per="frame count")
        want_s = "AgxError: op: " + message.format(name="stages", per="stage count")
        assert _message(lambda: ops._checked_rows("op", 2, cpu, counts=bad, on="the stream on")) == want_c
        assert _message(lambda: ops._checked_rows("op", 2, cpu, stages=bad, on="the stream on")) == want_s
        assert _message(lambda: ops._checked_rows("op", 2, cpu, bad, bad, on="the stream on")) == want_c        # counts come first
        # ... which is what the two checks it is built on say
        assert _message(lambda: ops._checked_counts("op", bad, 2, cpu, on="the stream on")) == want_c
        assert _message(lambda: ops._checked_stages("op", bad, 2, cpu, on="the stream on")) == want_s
    # an op (on=None): the operands must be on the GPU as well
    assert "MI355X only" in _message(lambda: ops._checked_rows("op", 2, cpu, good))
    assert "MI355X only" in _message(lambda: ops._checked_rows("op", 2, cpu, stages=good))


# ------------------------------------------------------------------------------------------------- 2. streaming
@pytest.fixture(scope="module")
def ctx():
    """Q = 2, K = 16: 4-bit codes, 6 samples a frame, D = 8; streams of two rows."""
    class Ctx:
        pass
    c = Ctx()
    c.model, c.other = _model(), _model()
    c.s = c.model.new_stream(2, max_chunk=3)
    c.wide = c.model.new_stream(2, max_chunk=ops.RVQ_STEP_MAX_N + 8)
    c.foreign = c.other.new_stream(2, max_chunk=3)
    c.coder = PriorCoder(CodePrior(2, (16, 16), 16, 1, 2, 32, 8, 32).eval())
    c.coder3 = PriorCoder(CodePrior(3, (16, 16, 16), 16, 1, 3, 32, 8, 32).eval())
    c.state = c.coder.new_state(2, 3)
    c.state_wide = c.coder.new_state(2, ops.RVQ_STEP_MAX_N + 8)
    c.state1 = c.coder.new_state(1, 3)
    c.x = torch.zeros(2, 1, 12)                                   # two frames
    c.packets = torch.zeros(2, 2, dtype=torch.uint8)              # of two frames
    c.good = torch.ones(2, dtype=I64)
    c.bad = torch.ones(2, dtype=torch.int32)
    return c


def test_own_stream_refusals(ctx):
    streaming._own_stream(ctx.model, ctx.s, "step")
    assert _message(lambda: streaming._own_stream(ctx.model, ctx.foreign, "step")) == \
        "AgxError: step: the stream belongs to another model (model.new_stream makes one for this model)"
    assert _message(lambda: streaming._own_stream(ctx.model, None, "step")) == \
        "AgxError: step: the stream belongs to another model (model.new_stream makes one for this model)"
    ctx.model.train()
    try:
        assert _message(lambda: streaming._own_stream(ctx.model, ctx.s, "step")) == \
            "NotImplementedError: step: a stream is inference only: call model.eval() (there is no backward through a stream)"
        assert "another model" in _message(lambda: streaming._own_stream(ctx.model, ctx.foreign, "step"))      # ownership first
    finally:
        ctx.model.eval()


def test_step_frames_refusals(ctx):
    n = ops.RVQ_STEP_MAX_N
    assert streaming._step_frames("step", 3, ctx.s) == 3 and streaming._step_frames("step", n, ctx.wide) == n
    assert streaming._step_frames("step", n, None) == n and streaming._step_frames("step", 2, ctx.s, 2) == 2
    for frames, stream, extra, message in (
            (0, ctx.s, None, "step: frames = 0 outside 1 .. the stream's max_chunk = 3"),
            (4, ctx.s, None, "step: frames = 4 outside 1 .. the stream's max_chunk = 3"),
            (n + 1, ctx.wide, None, f"step: frames = {n + 1} exceeds the {n} frames a quantiser step takes"),
            (0, ctx.s, 2, "step: frames = 0 outside 1 .. min(the stream's max_chunk = 3, the coder state's max_frames = 2)"),
            (3, ctx.s, 2, "step: frames = 3 outside 1 .. min(the stream's max_chunk = 3, the coder state's max_frames = 2)"),
            (n + 1, ctx.wide, n + 8, f"step: frames = {n + 1} exceeds the {n} frames a quantiser step takes"),
            (0, None, None, f"step: frames = 0 outside 1 .. the {n} frames a quantiser step takes"),
            (n + 1, None, None, f"step: frames = {n + 1} outside 1 .. the {n} frames a quantiser step takes")):
        assert _message(lambda: streaming._step_frames("step", frames, stream, extra)) == "AgxError: " + message


def test_checked_packet_rows_refusals():
    streaming._checked_packet_rows("step", torch.zeros(2, 3, dtype=torch.uint8), 3, 2, 4)
    for packets, got in ((torch.zeros(2, 2, dtype=torch.uint8), "torch.uint8 (2, 2)"),          # one byte too narrow
                         (torch.zeros(2, 3, dtype=I64), "torch.int64 (2, 3)"), (torch.zeros(6, dtype=torch.uint8), "torch.uint8 (6,)"),
                         ([0] * 3, "list")):
        assert _message(lambda: streaming._checked_packet_rows("step", packets, 3, 2, 4)) == \
            f"AgxError: step: packets of 3 frames x 2 codes x 4 bits are uint8 (B, 3), got {got}"


# ------------------------------------------------------------------------------------------------- 3. the order of refusals
N1 = ops.RVQ_STEP_MAX_N + 1
OWNER = "the stream belongs to another model (model.new_stream makes one for this model)"
EVAL = "a stream is inference only: call model.eval() (there is no backward through a stream)"
ROWS2 = "must be a contiguous int64 device tensor of 2 entries"
# (entry, the two faults, the call, train the model first?, the first refusal as the code before this file's helpers gave it)
TWO_FAULTS = (
    ("compress_stream", "foreign stream + bad stages", lambda c: c.model.compress_stream(c.x, c.foreign, stages=c.bad), False,
     f"AgxError: encode_codes_stream: stages {ROWS2} (one stage count per batch row), got (2,) torch.int32"),
    ("compress_stream", "training + a chunk above the quantiser step", lambda c: c.model.compress_stream(torch.zeros(2, 1, 6 * N1), c.wide), True,
     f"AgxError: encode_codes_stream: a chunk of {N1} frames exceeds the {N1 - 1} frames a quantiser step takes"),
    ("compress_stream", "bad stages + a chunk above the quantiser step",
     lambda c: c.model.compress_stream(torch.zeros(2, 1, 6 * N1), c.wide, stages=c.bad), False,
     f"AgxError: encode_codes_stream: stages {ROWS2} (one stage count per batch row), got (2,) torch.int32"),
    ("compress_stream", "training + bad counts", lambda c: c.model.compress_stream(c.x, c.s, counts=c.bad), True,
     f"NotImplementedError: encode_stream: {EVAL}"),
    ("compress_stream", "foreign stream + training", lambda c: c.model.compress_stream(c.x, c.foreign), True,
     f"AgxError: encode_stream: {OWNER}"),
    ("decompress_stream", "foreign stream + training", lambda c: c.model.decompress_stream(c.packets, c.foreign, 2), True,
     f"AgxError: decode_codes_stream: {OWNER}"),
    ("decompress_stream", "training + frames 0", lambda c: c.model.decompress_stream(c.packets, c.s, 0), True,
     f"NotImplementedError: decode_codes_stream: {EVAL}"),
    ("decompress_stream", "frames past max_chunk and past the quantiser step", lambda c: c.model.decompress_stream(c.packets, c.wide, N1 + 8), False,
     f"AgxError: decode_codes_stream: frames = {N1 + 8} outside 1 .. the stream's max_chunk = {N1 + 7}"),
    ("decompress_stream", "frames above the quantiser step + narrow packets", lambda c: c.model.decompress_stream(c.packets, c.wide, N1), False,
     f"AgxError: decode_codes_stream: frames = {N1} exceeds the {N1 - 1} frames a quantiser step takes"),
    ("decompress_stream", "narrow packets + bad counts", lambda c: c.model.decompress_stream(c.packets, c.s, 3, counts=c.bad), False,
     "AgxError: decode_codes_stream: packets of 3 frames x 2 codes x 4 bits are uint8 (B, 3), got torch.uint8 (2, 2)"),
    ("decompress_stream", "bad counts + bad stages", lambda c: c.model.decompress_stream(c.packets, c.s, 2, counts=c.bad, stages=c.bad), False,
     f"AgxError: decode_codes_stream: counts {ROWS2} (one frame count per batch row), got (2,) torch.int32"),
    ("restage_packets", "frames 0 + narrow packets", lambda c: c.model.restage_packets(c.packets[:, :1], 0, c.good), False,
     f"AgxError: restage_packets: frames = 0 outside 1 .. the {N1 - 1} frames a quantiser step takes"),
    ("restage_packets", "frames above the quantiser step + bad stages", lambda c: c.model.restage_packets(c.packets, N1, c.bad), False,
     f"AgxError: restage_packets: frames = {N1} outside 1 .. the {N1 - 1} frames a quantiser step takes"),
    ("restage_packets", "narrow packets + bad stages", lambda c: c.model.restage_packets(c.packets, 3, c.bad), False,
     "AgxError: restage_packets: packets of 3 frames x 2 codes x 4 bits are uint8 (B, 3), got torch.uint8 (2, 2)"),
    ("restage_packets", "bad stages + bad counts", lambda c: c.model.restage_packets(c.packets, 2, c.bad, counts=c.bad), False,
     f"AgxError: rvq_packets_restage: stages_to {ROWS2} (one stage count per batch row), got (2,) torch.int32"),
    ("restage_packets", "bad stages_from + bad counts", lambda c: c.model.restage_packets(c.packets, 2, c.good, stages_from=c.bad, counts=c.bad),
     False, f"AgxError: rvq_packets_restage: stages_from {ROWS2} (one stage count per batch row), got (2,) torch.int32"),
    ("compress_stream_coded", "x is a list + foreign stream", lambda c: c.model.compress_stream_coded([0.0], c.foreign, c.coder, c.state), False,
     "AgxError: compress_stream_coded: x_chunk must be a tensor, got list"),
    ("compress_stream_coded", "foreign stream + training", lambda c: c.model.compress_stream_coded(c.x, c.foreign, c.coder, c.state), True,
     f"AgxError: compress_stream_coded: {OWNER}"),
    ("compress_stream_coded", "training + no coder", lambda c: c.model.compress_stream_coded(c.x, c.s, None, c.state), True,
     f"NotImplementedError: compress_stream_coded: {EVAL}"),
    ("compress_stream_coded", "another quantiser's coder + a hop above the state's max_frames",
     lambda c: c.model.compress_stream_coded(torch.zeros(2, 1, 24), c.wide, c.coder3, c.state), False,
     "AgxError: compress_stream_coded: the prior models 3 stages of (16, 16, 16) codes, the quantiser has 2 of (16, 16)"),
    ("compress_stream_coded", "a hop above the state's max_frames + a state of another batch",
     lambda c: c.model.compress_stream_coded(torch.zeros(2, 1, 24), c.wide, c.coder, c.state1), False,
     f"AgxError: compress_stream_coded: frames = 4 outside 1 .. min(the stream's max_chunk = {N1 + 7}, the coder state's max_frames = 3)"),
    ("compress_stream_coded", "a hop above the quantiser step + bad counts",
     lambda c: c.model.compress_stream_coded(torch.zeros(2, 1, 6 * N1), c.wide, c.coder, c.state_wide, counts=c.bad), False,
     f"AgxError: compress_stream_coded: frames = {N1} exceeds the {N1 - 1} frames a quantiser step takes"),
    ("compress_stream_coded", "a state of another batch + bad counts",
     lambda c: c.model.compress_stream_coded(c.x, c.s, c.coder, c.state1, counts=c.bad), False,
     "AgxError: compress_stream_coded: the coder state has batch 1 on 'cpu', the stream 2 on 'cpu'"),
    ("compress_stream_coded", "bad counts + bad stages", lambda c: c.model.compress_stream_coded(c.x, c.s, c.coder, c.state, c.bad, c.bad), False,
     f"AgxError: compress_stream_coded: counts {ROWS2} (one frame count per batch row), got (2,) torch.int32"),
    ("decompress_stream_coded", "foreign stream + training",
     lambda c: c.model.decompress_stream_coded(c.packets, c.good, c.foreign, c.coder, c.state, 2), True,
     f"AgxError: decompress_stream_coded: {OWNER}"),
    ("decompress_stream_coded", "training + frames 0", lambda c: c.model.decompress_stream_coded(c.packets, c.good, c.s, c.coder, c.state, 0), True,
     f"NotImplementedError: decompress_stream_coded: {EVAL}"),
    ("decompress_stream_coded", "another quantiser's coder + frames 0",
     lambda c: c.model.decompress_stream_coded(c.packets, c.good, c.s, c.coder3, c.state, 0), False,
     "AgxError: decompress_stream_coded: the prior models 3 stages of (16, 16, 16) codes, the quantiser has 2 of (16, 16)"),
    ("decompress_stream_coded", "frames 0 + bad stages",
     lambda c: c.model.decompress_stream_coded(c.packets, c.good, c.s, c.coder, c.state, 0, stages=c.bad), False,
     "AgxError: decompress_stream_coded: frames = 0 outside 1 .. min(the stream's max_chunk = 3, the coder state's max_frames = 3)"),
    ("decompress_stream_coded", "bad counts + bad stages",
     lambda c: c.model.decompress_stream_coded(c.packets, c.good, c.s, c.coder, c.state, 2, c.bad, c.bad), False,
     f"AgxError: decompress_stream_coded: counts {ROWS2} (one frame count per batch row), got (2,) torch.int32"),
)


@pytest.mark.parametrize("entry,faults,call,train,first", TWO_FAULTS, ids=[f"{e}: {f}" for e, f, *_ in TWO_FAULTS])
def test_two_faults_raise_the_first_refusal_of_before(ctx, entry, faults, call, train, first):
    ctx.model.train(train)
    try:
        with torch.no_grad():
            assert _message(lambda: call(ctx)) == first
    finally:
        ctx.model.eval()


def test_the_quantiser_refusal_of_a_coded_step_precedes_the_eval_refusal(ctx, monkeypatch):
    """Three faults of ``compress_stream_coded`` in the order they are refused: the stream's owner, the bottleneck, eval."""
    monkeypatch.setattr(ctx.model, "quantizer", torch.nn.Identity())
    ctx.model.train()
    try:
        assert _message(lambda: ctx.model.compress_stream_coded(ctx.x, ctx.foreign, ctx.coder, ctx.state)) == \
            f"AgxError: compress_stream_coded: {OWNER}"
        assert _message(lambda: ctx.model.compress_stream_coded(ctx.x, ctx.s, ctx.coder, ctx.state)) == \
            "NotImplementedError: compress_stream_coded: the bottleneck Identity is not a ResidualQuantizer"
    finally:
        ctx.model.eval()
