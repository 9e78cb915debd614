"""Quantiser dropout on the device: ``agx_rvq_forward_staged`` / ``agx_rvq_backward_staged`` and the training call,
module and model built on them, against the CPU statement of tests/rvq_dropout_ref.py.

Row b of a staged call must be row b quantised alone with ``q_used = q_b`` -- bit for bit, by the unstaged op itself -- and the
float64 side is the reference's: sq_err and commit within ``1e-5 max(1, |want|)`` (the tolerance tests/test_gpu_parity.py uses
for the commit loss), the gradients inside the derived bound ``2 (m + 2) 2^-24 sum|addends|`` over live addends, and exact zeros
where nothing is live.  The shapes put row edges inside the forward's 32-frame and the backward's 64-frame workgroups."""
import pytest
import torch

from audio_generation_amd import ops
from audio_generation_amd.dist import GradBucket
from audio_generation_amd.quantizer import ResidualQuantizer
from audio_generation_amd.vae import CausalVQAE
from tests import rvq_dropout_ref as ref
from tests.test_gpu_rvq_backward import PLUMBING, _Recorder, check

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, T, D, K, Q) and the stage counts as given (the kernels clamp them to [0, q_used])
CASES = {
    "row-edges": dict(shape=(3, 37, 33, 100, 3), stages=[1, 3, 2]),                  # frames 37 and 74 fall inside workgroups; odd D
    "channel-major": dict(shape=(2, 31, 64, 300, 4), stages=[4, 1], layout="b c l", g_transposed=True),
    "zero-and-clamped": dict(shape=(4, 5, 8, 16, 2), stages=[0, 9, -3, 1]),
    "model-D-K-Q": dict(shape=(2, 9, 512, 1024, 8), stages=[3, 8]),
    "sized-stages": dict(shape=(3, 37, 64, 128, 3), stages=[2, 3, 1], sizes=(128, 37, 100)),
    "seventeen-stages": dict(shape=(2, 13, 20, 8, 17), stages=[17, 5]),              # the QMAX = 64 backward instance
    "codebook_n-2": dict(shape=(3, 37, 33, 100, 3), stages=[3, 1, 2], q_used=2),
}
_BUILT = {}


def _make(name):
    """The case's CPU tensors and its reference forward, computed once and shared (never written)."""
    if name not in _BUILT:
        spec = CASES[name]
        b, t, d, k, n_q = spec["shape"]
        gen = torch.Generator().manual_seed(sum(map(ord, name)))
        x = torch.randn(b, t, d, generator=gen)
        cbs = torch.randn(n_q, k, d, generator=gen)
        if n_q > 4:
            cbs *= (0.7 ** torch.arange(n_q, dtype=torch.float32)).view(-1, 1, 1)      # later stages refine
        sizes = spec.get("sizes")
        if sizes is not None:
            for q, kq in enumerate(sizes):
                cbs[q, kq:] = 0.0
        g_xq = torch.randn(b, t, d, generator=gen)
        g_l = 0.5 + float(torch.rand((), generator=gen))
        q_used = spec.get("q_used", n_q)
        _BUILT[name] = dict(spec=spec, x=x, cbs=cbs, sizes=sizes, g_xq=g_xq, g_l=g_l, q_used=q_used, stages=spec["stages"],
                            layout=spec.get("layout", "b l c"), fwd=ref.forward(x, cbs, spec["stages"], q_used, sizes))
    return _BUILT[name]


def _device(c):
    """(x, codebooks, packed, g_xq, g_commit, stages) on the device, x and g_xq in the case's layout."""
    cbd = c["cbs"].to(DEV)
    xd, gd = c["x"].to(DEV), c["g_xq"].to(DEV)
    if c["layout"] == "b c l":
        xd = xd.transpose(1, 2).contiguous()
        gd = gd.transpose(1, 2) if c["spec"].get("g_transposed") else gd.transpose(1, 2).contiguous()
    return (xd, cbd, ops.rvq_pack(cbd, c["sizes"]), gd, torch.tensor(c["g_l"], dtype=torch.float32, device=DEV),
            torch.tensor(c["stages"], dtype=torch.int64, device=DEV))


def _blc(v, layout):
    return v.transpose(1, 2) if layout == "b c l" else v


@pytest.mark.parametrize("name", list(CASES))
def test_forward_rows_are_their_own_unstaged_calls(name):
    c = _make(name)
    layout, q_used = c["layout"], c["q_used"]
    xd, cbd, packed, _, _, sd = _device(c)
    xq, idx, sq, commit = ops.rvq_forward(xd, cbd, packed, q_used, layout, stages=sd)
    xq2, idx2, sq2, commit2 = ops.rvq_forward(xd, cbd, packed, q_used, layout, stages=sd)
    assert xq.shape == xd.shape and idx.shape == (xd.shape[0], c["x"].shape[1], q_used) and sq.shape == (q_used,)
    assert torch.equal(xq, xq2) and torch.equal(idx, idx2) and torch.equal(sq, sq2) and torch.equal(commit, commit2)
    q_b = ref.taken(c["stages"], xd.shape[0], q_used)
    for row, q in enumerate(q_b):
        own_q, own_i, _, _ = ops.rvq_forward(xd[row:row + 1], cbd, packed, q, layout)
        assert torch.equal(xq[row:row + 1], own_q), (row, "x_q")
        assert torch.equal(idx[row, :, :q], own_i[0]), (row, "index")
        assert bool((idx[row, :, q:] == -1).all()), (row, "dead stages")
        if q == 0:
            assert float(xq[row].abs().max()) == 0.0
    want_q, want_i, want_sq, want_c = c["fwd"]
    assert torch.equal(idx.cpu(), want_i) and torch.equal(_blc(xq, layout).cpu(), want_q)
    for q in range(q_used):
        got = float(sq[q])
        print(f"{name} sq_err[{q}]: {got!r} want {float(want_sq[q])!r}")
        assert abs(got - float(want_sq[q])) <= 1e-5 * max(1.0, abs(float(want_sq[q])))
        if not any(q < v for v in q_b):
            assert got == 0.0, "no frame is live at this stage"
    print(f"{name} commit: {float(commit)!r} want {want_c!r}")
    assert abs(float(commit) - want_c) <= 1e-5 * max(1.0, abs(want_c))


@pytest.mark.parametrize("name", list(CASES))
def test_backward_against_the_float64_definition(name):
    c = _make(name)
    layout, q_used = c["layout"], c["q_used"]
    xd, cbd, packed, gd, gl, sd = _device(c)
    _, idx, _, _ = ops.rvq_forward(xd, cbd, packed, q_used, layout, stages=sd)
    dx, dc = ops.rvq_backward(xd, cbd, idx, gd, gl, layout, want_codebook_grad=True, stages=sd)
    dx2, dc2 = ops.rvq_backward(xd, cbd, idx, gd, gl, layout, want_codebook_grad=True, stages=sd)
    assert dx.shape == xd.shape and dx.is_contiguous() and dc.shape == cbd.shape
    assert torch.equal(dx, dx2) and torch.equal(dc, dc2), "two calls on the same inputs must agree bit for bit"
    want = ref.definition(c["x"], c["cbs"], idx.cpu(), c["stages"], c["g_xq"], float(gl))
    check(_blc(dx, layout), dc, want, name)                   # the bound, and == 0 for rows nobody chose and stages nobody ran
    assert abs(want[5] - c["fwd"][3]) <= 1e-9 * max(1.0, abs(want[5]))      # the definition's L is the forward's commit
    q_b = ref.taken(c["stages"], xd.shape[0], q_used)
    for q in range(cbd.shape[0]):
        if not any(q < v for v in q_b):
            assert float(dc[q].abs().max()) == 0.0, ("a stage no row runs", q)
    for row, q in enumerate(q_b):
        if q == 0:
            assert torch.equal(dx[row], gd[row]), "q_b = 0: dx is g_xq alone"
    dx3, none = ops.rvq_backward(xd, cbd, idx, gd, gl, layout, want_codebook_grad=False, stages=sd)
    assert none is None and torch.equal(dx3, dx)


@pytest.mark.parametrize("name", ["row-edges", "channel-major", "seventeen-stages", "codebook_n-2"])
def test_every_row_at_q_is_the_unstaged_call(name):
    c = _make(name)
    layout, q_used = c["layout"], c["q_used"]
    xd, cbd, packed, gd, gl, _ = _device(c)
    full = torch.full((xd.shape[0],), cbd.shape[0], dtype=torch.int64, device=DEV)
    plain = ops.rvq_forward(xd, cbd, packed, q_used, layout)
    staged = ops.rvq_forward(xd, cbd, packed, q_used, layout, stages=full)
    for a, b, what in zip(plain, staged, ("x_q", "index", "sq_err", "commit")):
        assert torch.equal(a, b), what
    dx, dc = ops.rvq_backward(xd, cbd, plain[1], gd, gl, layout, want_codebook_grad=True)
    sdx, sdc = ops.rvq_backward(xd, cbd, plain[1], gd, gl, layout, want_codebook_grad=True, stages=full)
    assert torch.equal(dx, sdx) and torch.equal(dc, sdc)


def test_refusals_on_the_device():
    c = _make("zero-and-clamped")
    xd, cbd, packed, gd, gl, sd = _device(c)
    with pytest.raises(ops.AgxError, match="stages is on 'cpu', the inputs are on 'cuda:0'"):
        ops.rvq_forward(xd, cbd, packed, 2, stages=sd.cpu())
    with pytest.raises(ops.AgxError, match="rvq_forward: stages"):
        ops.rvq_forward(xd, cbd, packed, 2, stages=sd.int())
    _, idx, _, _ = ops.rvq_forward(xd, cbd, packed, 2, stages=sd)
    with pytest.raises(ops.AgxError, match="rvq_backward: stages"):
        ops.rvq_backward(xd, cbd, idx, gd, gl, stages=sd[:3])


def _module_case(klass):
    torch.manual_seed(11)
    m = ResidualQuantizer(num_quantizers=3, dim=32, quantizer_class=klass, codebook_sizes=64).to(DEV).train()
    return m, torch.randn(2, 19, 32), torch.randn(2, 19, 32), [2, 1]           # stage 2: no row runs it


@pytest.mark.parametrize("klass", ["base", "ema"])
def test_module_trains_with_stages(klass):
    m, x, w, stages = _module_case(klass)
    cbs = m.codebooks.detach().cpu().clone()
    sd = torch.tensor(stages, dtype=torch.int64, device=DEV)
    xd = x.to(DEV).requires_grad_(True)
    xq, idx, commit = m(xd, stages=sd)
    ((xq * w.to(DEV)).sum() + 3 * commit).backward()
    want_q, want_i, _, want_c = ref.forward(x, cbs, stages)
    assert torch.equal(idx.cpu(), want_i) and torch.equal(xq.detach().cpu(), want_q)
    assert abs(float(commit.detach()) - want_c) <= 1e-5 * max(1.0, abs(want_c))
    want = ref.definition(x, cbs, idx.cpu(), stages, w, 3.0)
    if klass == "base":
        assert m.codebooks.grad is not None, "the learnable codebooks must receive a gradient"
        check(xd.grad, m.codebooks.grad, want, "base module")
        assert float(m.codebooks.grad[2].abs().max()) == 0.0
    else:
        check(xd.grad, None, want, "ema module")
        assert m.codebooks.grad is None and torch.equal(m.codebooks.cpu(), cbs)
    with torch.no_grad():                                     # eval with stages: the same search, a per-row bitrate
        xq_eval, idx_eval, commit_eval = m.eval()(x.to(DEV), stages=sd)
    assert torch.equal(xq.detach(), xq_eval) and torch.equal(idx, idx_eval) and torch.equal(commit.detach(), commit_eval)


def test_stages_written_before_the_backward_raise():
    m, x, w, stages = _module_case("base")
    sd = torch.tensor(stages, dtype=torch.int64, device=DEV)
    xq, _, commit = m(x.to(DEV).requires_grad_(True), stages=sd)
    sd.fill_(3)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (xq.sum() + commit).backward()


def test_ema_statistics_of_a_masked_index():
    """agx_rvq_ema_stats on the staged forward's index: a dead stage matches no code and subtracts nothing (no new kernel)."""
    c = _make("row-edges")
    xd, cbd, packed, _, _, sd = _device(c)
    _, idx, _, _ = ops.rvq_forward(xd, cbd, packed, 3, stages=sd)
    d = xd.shape[2]
    stats = ops.rvq_ema_stats(xd.reshape(-1, d), cbd, idx.reshape(-1, 3)).cpu()
    want = ref.ema_stats(c["x"].reshape(-1, d).double(), c["cbs"].double(), idx.cpu().reshape(-1, 3))
    assert torch.equal(stats[:, :, 0].double(), want[:, :, 0])
    assert stats[:, :, 0].sum(dim=1).tolist() == [3 * 37, 2 * 37, 1 * 37]
    # tests/test_gpu_step.py: sums within 1e-6 * 4 * the largest count
    assert float((stats[:, :, 1:].double() - want[:, :, 1:]).abs().max()) <= 4e-6 * float(want[:, :, 0].max())


def test_update_codebook_with_stages():
    m, x, w, stages = _module_case("ema")
    cbs = m.codebooks.detach().cpu().clone()
    sd = torch.tensor(stages, dtype=torch.int64, device=DEV)
    xd = x.to(DEV).requires_grad_(True)
    xq, idx, commit = m(xd, stages=sd)
    ((xq * w.to(DEV)).sum() + 3 * commit).backward()
    freq, ema_sum = m.cluster_frequency.clone(), m.ema_sum.clone()
    xd2 = x.to(DEV).requires_grad_(True)
    xq2, idx2, commit2 = m(xd2, update_codebook=True, stages=sd)
    assert torch.equal(idx2, idx) and torch.equal(xq2.detach(), xq.detach())
    stats = ref.ema_stats(x.reshape(-1, 32), cbs, idx.cpu().reshape(-1, 3))
    f0 = 0.99 * 1.0 + 0.01 * stats[0, :, 0]
    want_cb0 = (0.99 * cbs[0] + 0.01 * stats[0, :, 1:]) / f0.clamp_min(1e-5).unsqueeze(1)
    assert float((m.codebooks[0].cpu() - want_cb0).abs().max()) < 1e-5
    assert float((m.cluster_frequency[0].cpu() - f0).abs().max()) < 1e-5
    assert not torch.equal(m.codebooks[1].cpu(), cbs[1])                        # row 0 ran stage 1
    # stage 2: no row ran it -- codewords and statistics are bit-identical to before
    assert torch.equal(m.codebooks[2].cpu(), cbs[2]) and torch.equal(m.cluster_frequency[2], freq[2])
    assert torch.equal(m.ema_sum[2], ema_sum[2])
    ((xq2 * w.to(DEV)).sum() + 3 * commit2).backward()
    assert torch.equal(xd2.grad, xd.grad), "the backward sees the codewords the search used"


def test_model_takes_an_adam_step_with_stages():
    torch.manual_seed(3)
    model = CausalVQAE(in_channels=1, first_block_channels=4, n_blocks=2, strides=(2, 2), codebook_dim=16, codebook_size=32,
                       num_quantizers=3, vq_type="base", input_format="n c l", wavelet_decoders=False).to(DEV).train()
    x = 0.1 * torch.randn(2, 1, 256, device=DEV)
    with torch.no_grad():
        model.quantizer.init_from_latents(model._run_encoders(x))
    bucket = GradBucket(model.parameters())
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    cb = model.quantizer.codebooks
    before = cb.detach().clone()
    sd = torch.tensor([2, 1], dtype=torch.int64, device=DEV)                    # stage 2 runs for no row
    y, commit, index = model(x, stages=sd)
    assert index.shape[-1] == 3 and bool((index[0, :, 2] == -1).all()) and bool((index[1, :, 1:] == -1).all())
    assert bool((index[0, :, :2] >= 0).all()) and bool((index[1, :, 0] >= 0).all())
    (((y - x) ** 2).mean() + commit).backward()
    assert bucket.intact()
    lo, hi = bucket.flat.data_ptr(), bucket.flat.data_ptr() + 4 * bucket.flat.numel()
    assert lo <= cb.grad.data_ptr() < hi, "the codebook gradient must land in the bucket view"
    chosen = torch.zeros(3, 32, dtype=torch.bool)
    for q in range(3):
        col = index[..., q].reshape(-1).cpu()
        chosen[q, col[col >= 0]] = True
    assert not chosen[2].any()
    grad = cb.grad.detach().cpu()
    assert float(grad[chosen].abs().max()) > 0.0
    assert bool((grad[~chosen] == 0).all()), "codes nobody chose and the stage no row ran"
    opt.step()
    after = cb.detach().cpu()
    assert not torch.equal(after[:2], before[:2].cpu())
    assert torch.equal(after[~chosen], before.cpu()[~chosen]), "Adam must leave rows with a zero gradient alone"
    assert torch.equal(after[2], before[2].cpu())
    # the same keyword through the training step helpers
    from audio_generation_amd import step
    model.zero_grad(set_to_none=False)
    loss, _, parts = step.training_backward(model, x, stages=sd)
    assert "commit_loss" in parts and float(cb.grad[2].abs().max()) == 0.0 and float(cb.grad[:2].abs().max()) > 0.0


def test_graph_capture_replays_new_stages():
    torch.manual_seed(7)
    m = ResidualQuantizer(num_quantizers=4, dim=32, quantizer_class="ema", codebook_sizes=64).to(DEV).eval()
    x = torch.randn(3, 21, 32, device=DEV)
    first, other = [4, 1, 2], [0, 3, 9]
    sd = torch.tensor(first, dtype=torch.int64, device=DEV)
    with torch.no_grad():
        want = {}
        for key, s in (("first", first), ("other", other)):
            want[key] = [t.clone() for t in m(x, stages=torch.tensor(s, dtype=torch.int64, device=DEV))]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(x, stages=sd)                                   # warm-up: the packed image is built outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = m(x, stages=sd)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs, want["first"]))
        sd.copy_(torch.tensor(other, dtype=torch.int64, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs, want["other"]))
        assert not torch.equal(want["first"][1], want["other"][1])


@pytest.mark.parametrize("klass", ["base", "ema"])
def test_no_aten_arithmetic_in_the_staged_training_call(klass):
    torch.manual_seed(5)
    m = ResidualQuantizer(num_quantizers=3, dim=32, quantizer_class=klass, codebook_sizes=24).to(DEV).train()
    x = torch.randn(2, 32, 19, device=DEV, requires_grad=True)          # (B, D, T): 1216 elements; codebooks: 2304
    sd = torch.tensor([1, 3], dtype=torch.int64, device=DEV)
    if klass == "base":
        m.codebooks.grad = torch.zeros_like(m.codebooks)                # as under a GradBucket: the gradient is accumulated
    g_xq, g_l = torch.randn(2, 32, 19, device=DEV), torch.tensor(3.0, device=DEV)
    m.quantize_bcl(x.detach(), stages=sd)                               # builds the packed image outside the record
    torch.cuda.synchronize()
    with _Recorder() as rec:
        xq, index, commit = m.quantize_bcl(x, stages=sd)
        torch.autograd.backward([xq, commit], [g_xq, g_l])
    assert x.grad is not None and (klass == "ema" or float(m.codebooks.grad.abs().max()) > 0.0)
    assert bool((index[0, :, 1:] == -1).all())
    names = [full for _, full, _ in rec.seen]
    print(names)
    param_shape = tuple(m.codebooks.shape)
    for _, full, shapes in rec.seen:
        if full in PLUMBING:
            continue
        # the only arithmetic: accumulating the parameter-sized gradient into an existing .grad
        assert klass == "base" and full.startswith("aten.add") and shapes == [param_shape], (full, shapes, names)
    banned = ("index", "add", "sub", "mul", "pow", "mean", "clone", "copy", "contiguous")
    for _, full, shapes in rec.seen:
        if any(full.startswith(f"aten.{b}") for b in banned):
            assert all(s == param_shape for s in shapes), (full, shapes)
