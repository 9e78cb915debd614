"""The code-prior kernels on the GPU (csrc/prior.hip) against the mirrors of tests/prior_ref.py: the gather-sum bit for bit, its
backward and the cross-entropy against float64, the sampler row by row where the mirror calls the row decided.

Tolerances are the suite's for like quantities (tests/test_gpu_causal_attention.py): 2e-5 of max(1, |want|) for forward values,
2e-4 of max(1, max|want|) for gradients.  The embedding backward is a plain binary32 sum of at most 10 rows per destination here
(140 in the collision case, where the bound 140 * 2^-24 * max|partial sum| is a tenth of it): the same gradient tolerance."""
import ctypes

import numpy as np
import pytest
import torch

from audio_generation_amd import _lib, ops
from audio_generation_amd._lib import AgxError
from tests import prior_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(a, dtype=dtype).to(DEV)


# ---------------------------------------------------------------------------------------------------------------- embed
def _embed_case(n, d, seed):
    rng = np.random.default_rng(seed)
    tables = rng.standard_normal((3, 17, d)).astype(np.float32)
    index = rng.integers(0, 17, (2, n, 3))
    index[0, 0, 1], index[1, n - 1, 0], index[1, 0, 2] = -1, 17, 1 << 40       # unused, one past the table, far outside
    return tables, index


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("d", [8, 100])
def test_embed_is_the_binary32_chain_bit_for_bit(n, d):
    tables, index = _embed_case(n, d, 10 * n + d)
    got = ops.codes_embed(_dev(index), _dev(tables))
    assert tuple(got.shape) == (2, d, n)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.embed(tables, index).view(np.uint32))
    counts = np.array([n + 3, n - 1])
    got = ops.codes_embed(_dev(index), _dev(tables), _dev(counts))
    want = ref.embed(tables, index, counts)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert float(got[1, :, n - 1:].abs().max()) == 0.0


def test_embed_more_than_one_tile_of_frames_and_channels():
    rng = np.random.default_rng(77)
    tables = rng.standard_normal((2, 9, 130)).astype(np.float32)
    index = rng.integers(-1, 10, (2, 37, 2))
    got = ops.codes_embed(_dev(index), _dev(tables))
    assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.embed(tables, index).view(np.uint32))


def test_embed_of_the_codebooks_is_the_quantisers_xq():
    gen = torch.Generator().manual_seed(21)
    b, t, d, k, q = 3, 11, 20, 24, 3
    x = torch.randn(b, t, d, generator=gen).to(DEV)
    cbs = (torch.randn(q, k, d, generator=gen) * torch.tensor([1.0, 0.5, 0.25])[:, None, None]).to(DEV)
    packed = ops.rvq_pack(cbs)
    stages = torch.tensor([3, 1, 0], dtype=torch.int64, device=DEV)
    for st in (None, stages):
        xq, index, _, _ = ops.rvq_forward(x, cbs, packed, q, stages=st)
        got = ops.codes_embed(index, cbs)
        assert torch.equal(got, xq.transpose(1, 2)), st
    assert int((index == -1).sum()) == t * (2 + 3)


def test_embed_backward_against_float64_with_exact_zeros_and_reproducible():
    rng = np.random.default_rng(31)
    b, n, d, rows = 2, 5, 100, 17
    index = rng.integers(0, 9, (b, n, 3))                     # rows 9 .. 16 are chosen by nobody
    index[0, 1, 0], index[1, 2, 2] = -1, 17
    dout = rng.standard_normal((b, d, n)).astype(np.float32)
    for counts in (None, np.array([n, 2])):
        got = ops.codes_embed_backward(_dev(dout), _dev(index), rows, _dev(counts))
        again = ops.codes_embed_backward(_dev(dout), _dev(index), rows, _dev(counts))
        want = ref.embed_backward(dout, index, rows, counts)
        assert tuple(got.shape) == (3, rows, d) and torch.equal(got, again)
        err = float(np.abs(got.cpu().numpy() - want).max())
        print(f"embed backward counts={None if counts is None else counts.tolist()}: max err {err:.3e}, max|ref| {np.abs(want).max():.3e}")
        assert err < 2e-4 * max(1.0, float(np.abs(want).max()))
        unused = np.abs(want).max(axis=2) == 0.0
        assert unused[:, 9:].all() and float(np.abs(got.cpu().numpy()[unused]).max()) == 0.0


def test_embed_backward_with_every_frame_on_one_code():
    """Heavy collisions: 2 x 70 frames (more than one ballot of 64) all on code 4 of both stages; D = 1030 takes two channel passes."""
    rng = np.random.default_rng(41)
    b, n, d, rows = 2, 70, 1030, 6
    index = np.full((b, n, 2), 4)
    dout = rng.standard_normal((b, d, n)).astype(np.float32)
    got = ops.codes_embed_backward(_dev(dout), _dev(index), rows)
    want = ref.embed_backward(dout, index, rows)
    chain = np.zeros(d, dtype=np.float32)
    for row in range(b):
        for i in range(n):
            chain = (chain + dout[row, :, i]).astype(np.float32)
    assert np.array_equal(got[0, 4].cpu().numpy(), chain) and torch.equal(got[0], got[1])      # frame order, one chain
    assert float(np.abs(got.cpu().numpy() - want).max()) < 2e-4 * max(1.0, float(np.abs(want).max()))
    assert float(got[:, [0, 1, 2, 3, 5]].abs().max()) == 0.0


# -------------------------------------------------------------------------------------------------------- cross-entropy
SIZES = (16, 5, 1)


def _ce_case(t, seed):
    rng = np.random.default_rng(seed)
    logits = (2.0 * rng.standard_normal((2, 3 * 16, t))).astype(np.float32)
    target = np.stack([rng.integers(-1, s + 1, (2, t)) for s in SIZES], axis=-1)      # -1 and `size` are dead
    target[0, 0, 0], target[1, 0, 2] = 3, -1
    return logits, target


@pytest.mark.parametrize("t", [1, 65])
def test_cross_entropy_and_its_backward_against_the_mirror(t):
    logits, target = _ce_case(t, 50 + t)
    g = 0.75
    want_loss, want_nll, want_d, want_live = ref.cross_entropy(logits, target, SIZES, g)
    ld, td = _dev(logits), _dev(target)
    loss, nll, lse, n_live = ops.codes_cross_entropy(ld, td, SIZES)
    again = ops.codes_cross_entropy(ld, td, SIZES)
    assert int(n_live) == want_live and torch.equal(loss, again[0]) and torch.equal(nll, again[1])
    e_loss = abs(float(loss) - want_loss)
    e_nll = float(np.abs(nll.cpu().numpy() - want_nll).max())
    dlogits = ops.codes_cross_entropy_backward(ld, td, lse, n_live, torch.tensor(g, device=DEV), SIZES)
    e_d = float(np.abs(dlogits.cpu().numpy() - want_d).max())
    print(f"cross-entropy T={t}: loss err {e_loss:.3e} (|loss| {abs(want_loss):.3e}), nll err {e_nll:.3e} (max {want_nll.max():.3e}), "
          f"dlogits err {e_d:.3e} (max|ref| {np.abs(want_d).max():.3e}), live {want_live} of {target.size}")
    assert e_loss < 2e-5 * max(1.0, abs(want_loss))
    assert e_nll < 2e-5 * max(1.0, float(want_nll.max()))
    assert e_d < 2e-4 * max(1.0, float(np.abs(want_d).max()))
    dead = ~((target >= 0) & (target < np.array(SIZES)))
    assert dead.any() and float(np.abs(nll.cpu().numpy()[dead]).max()) == 0.0
    d = dlogits.cpu().numpy().reshape(2, 3, 16, t)
    assert float(np.abs(d[:, 1, 5:]).max()) == 0.0 and float(np.abs(d[:, 2, 1:]).max()) == 0.0      # padded k
    assert float(np.abs(d.transpose(0, 3, 1, 2)[dead]).max()) == 0.0                                 # dead entries
    assert float(np.abs(d[:, 2, 0]).max()) == 0.0                                                    # a stage of one code: p = 1


def test_cross_entropy_of_an_all_dead_batch_is_zero():
    logits, target = _ce_case(7, 3)
    target[:] = -1
    ld, td = _dev(logits), _dev(target)
    loss, nll, lse, n_live = ops.codes_cross_entropy(ld, td, SIZES)
    assert float(loss) == 0.0 and int(n_live) == 0 and float(nll.abs().max()) == 0.0
    dlogits = ops.codes_cross_entropy_backward(ld, td, lse, n_live, torch.ones((), device=DEV), SIZES)
    assert float(dlogits.abs().max()) == 0.0


# --------------------------------------------------------------------------------------------------------------- sample
def _run_case(c, carry=None, logits=None, frame0=None):
    logits = c["logits"] if logits is None else logits
    return ops.codes_sample(_dev(logits), len(c["sizes"]), _dev(c["seeds"]), _dev(c["frame0"] if frame0 is None else frame0),
                            _dev(c["temperature"]), _dev(c["top_k"]), _dev(c["top_p"]), c["sizes"], _dev(c["counts"]),
                            _dev(c["stages"]), carry)


@pytest.mark.parametrize("name", list(ref.cases()))
def test_sampler_equals_the_mirror_on_every_decided_row(name):
    c = ref.cases()[name]
    want, decided, want_carry = ref.reference(name)
    b, n_q = want.shape[0], want.shape[2]
    carry = torch.full((b, n_q), -7, dtype=torch.int64, device=DEV)
    got = _run_case(c, carry)
    again = _run_case(c)
    assert torch.equal(got, again)
    got = got.cpu().numpy()
    live = want >= 0
    print(f"sampler {name}: {int(live.sum())} live rows, {int((live & ~decided).sum())} undecided, "
          f"{int((got != want)[decided].sum())} decided rows differ")
    assert np.array_equal(got[decided], want[decided])
    assert np.all(got[~live] == -1)
    sizes = np.array(c["sizes"])[None, None, :]
    assert np.all((got >= -1) & (got < sizes))
    # carry: the codes of frame c_b - 1 where c_b >= 1, untouched (-7) otherwise
    n = want.shape[1]
    for row in range(b):
        cnt = n if c["counts"] is None else int(np.clip(c["counts"][row], 0, n))
        if cnt == 0:
            assert np.all(carry[row].cpu().numpy() == -7)
        else:
            assert np.array_equal(carry[row].cpu().numpy(), got[row, cnt - 1])
    if "inf" in name:
        k = max(c["sizes"])
        for q, size in enumerate(c["sizes"]):
            picked = np.take_along_axis(c["logits"][:, q * k:q * k + size, :], np.maximum(got[:, :, q], 0)[:, None, :], axis=1)[:, 0, :]
            assert np.all(np.isfinite(picked[got[:, :, q] >= 0])), "a -inf logit was chosen"


def test_sampler_frames_do_not_depend_on_the_chunking():
    c = ref.cases()["large"]
    whole = _run_case(c)
    for i in range(c["logits"].shape[2]):
        one = _run_case(c, logits=np.ascontiguousarray(c["logits"][:, :, i:i + 1]), frame0=c["frame0"] + i)
        assert torch.equal(one[:, 0], whole[:, i]), i


def test_sampler_nan_logits_stay_in_bounds():
    c = dict(ref.cases()["edge-randn"])
    logits = c["logits"].copy()
    logits[0] = np.nan
    logits[1, ::7] = np.nan
    got = _run_case(c, logits=logits).cpu().numpy()
    assert np.all((got >= -1) & (got < np.array(c["sizes"])[None, None, :]))


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing():
    """Every refusal is raised by the wrapper or returned by the library's checks, which stand before the first launch; the
    outputs of an accepted call afterwards show the device is untouched by them."""
    tables = torch.randn(3, 17, 8, device=DEV)
    index = torch.zeros(2, 5, 3, dtype=torch.int64, device=DEV)
    logits = torch.randn(2, 48, 5, device=DEV)
    b1 = torch.zeros(2, dtype=torch.int64, device=DEV)
    f1 = torch.ones(2, device=DEV)
    with pytest.raises(AgxError, match="index"):
        ops.codes_embed(index.double(), tables)
    with pytest.raises(AgxError, match="index"):
        ops.codes_embed(index[:, :, :2], tables)
    with pytest.raises(AgxError, match="not contiguous"):
        ops.codes_embed(index.transpose(0, 1).contiguous().transpose(0, 1), tables)
    with pytest.raises(AgxError, match="counts"):
        ops.codes_embed(index, tables, counts=torch.zeros(3, dtype=torch.int64, device=DEV))
    with pytest.raises(AgxError, match="MI355X only"):
        ops.codes_embed(index.cpu(), tables.cpu())
    with pytest.raises(AgxError, match="dout"):
        ops.codes_embed_backward(torch.zeros(2, 8, 5, device=DEV).double(), index, 17)
    with pytest.raises(AgxError, match="sizes"):
        ops.codes_cross_entropy(logits, index, (16, 17, 1))
    with pytest.raises(AgxError, match="logits"):
        ops.codes_cross_entropy(logits[:, :47].contiguous(), index)
    with pytest.raises(AgxError, match="g must"):
        ops.codes_cross_entropy_backward(logits, index, torch.zeros(2, 5, 3, device=DEV), torch.ones((), dtype=torch.int64, device=DEV),
                                         torch.ones((), device=DEV).double())
    with pytest.raises(AgxError, match="CODES_SAMPLE_MAX_K"):
        ops.codes_sample(torch.zeros(2, 2049, 1, device=DEV), 1, b1, b1, f1, b1, f1)
    with pytest.raises(AgxError, match="temperature"):
        ops.codes_sample(logits, 3, b1, b1, f1.double(), b1, f1)
    with pytest.raises(AgxError, match="stages"):
        ops.codes_sample(logits, 3, b1, b1, f1, b1, f1, stages=b1.double())
    with pytest.raises(AgxError, match="carry"):
        ops.codes_sample(logits, 3, b1, b1, f1, b1, f1, carry=torch.zeros(2, 2, dtype=torch.int64, device=DEV))
    lib = _lib.load()
    sizes = (ctypes.c_int32 * 3)(16, 0, 1)
    assert lib.agx_codes_sample(logits.data_ptr(), ctypes.cast(sizes, ctypes.c_void_p), b1.data_ptr(), b1.data_ptr(), f1.data_ptr(),
                                b1.data_ptr(), f1.data_ptr(), None, None, None, None, 2, 5, 3, 16, None) == -1
    assert lib.agx_codes_sample(logits.data_ptr(), None, b1.data_ptr(), b1.data_ptr(), f1.data_ptr(), b1.data_ptr(), f1.data_ptr(), None,
                                None, None, None, 2, 5, 3, 16, None) == -2          # codes is NULL
    assert lib.agx_codes_embed_backward(logits.data_ptr(), index.data_ptr(), None, tables.data_ptr(), 2, 5, 3, 17, 8, None, 0, None) == -3
    torch.cuda.synchronize()
    assert torch.equal(ops.codes_embed(index, tables), (tables[0, 0] + tables[1, 0] + tables[2, 0])[None, :, None].expand(2, 8, 5))
