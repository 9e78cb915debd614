"""The code prior without a GPU: the mirrors of tests/prior_ref.py against independent references, the statistics of the
sampler's contract, the share of undecided rows on the GPU tests' inputs, and the bound symbols."""
import numpy as np
import pytest
import torch

from audio_generation_amd import _lib, ops
from tests import prior_ref as ref


def test_mirror_cross_entropy_is_torch_cross_entropy_with_an_ignore_index():
    gen = torch.Generator().manual_seed(5)
    b, t, n_q, k, sizes = 2, 7, 3, 16, (16, 5, 1)
    logits = torch.randn(b, n_q * k, t, generator=gen, dtype=torch.float64)
    target = torch.stack([torch.randint(-1, s + 1, (b, t), generator=gen) for s in sizes], dim=-1)   # -1 and size: dead
    target[0, 0, 0] = k + 3
    loss, nll, dlogits, n_live = ref.cross_entropy(logits.numpy(), target.numpy(), sizes)
    x = logits.clone().requires_grad_(True)
    total, live = 0.0, 0
    for q, s in enumerate(sizes):
        y = target[:, :, q]
        y = torch.where((y >= 0) & (y < s), y, torch.full_like(y, -100))
        total = total + torch.nn.functional.cross_entropy(x[:, q * k:q * k + s, :], y, ignore_index=-100, reduction="sum")
        live += int((y != -100).sum())
    (total / live).backward()
    assert n_live == live and 0 < live < b * t * n_q
    assert abs(loss - float((total / live).detach())) < 1e-12
    assert float((torch.from_numpy(dlogits) - x.grad).abs().max()) < 1e-14
    assert float(np.abs(nll[(target.numpy() < 0)]).max()) == 0.0
    assert ref.cross_entropy(logits.numpy(), np.full((b, t, n_q), -1), sizes)[0] == 0.0


def test_mirror_embed_is_the_stage_order_sum():
    gen = np.random.default_rng(3)
    tables = gen.standard_normal((3, 17, 8)).astype(np.float32)
    index = gen.integers(-1, 18, (2, 5, 3))
    out = ref.embed(tables, index, counts=np.array([5, 2]))
    want = np.zeros((2, 5, 8))
    for q in range(3):
        ok = (index[:, :, q] >= 0) & (index[:, :, q] < 17)
        want += np.where(ok[:, :, None], tables[q][np.where(ok, index[:, :, q], 0)], 0.0)
    want[1, 2:] = 0.0
    assert np.abs(out.transpose(0, 2, 1) - want).max() < 1e-6 and np.all(out[1, :, 2:] == 0.0)


def test_sampler_contract_frequencies_over_20000_frames():
    """Fixed logits, 20 000 frames: every code with p >= 0.01 lands within 5 binomial standard deviations, under plain
    temperature sampling and under top-k + top-p (whose kept set is renormalised)."""
    rng = np.random.default_rng(11)
    k, n = 24, 20000
    l = (1.5 * rng.standard_normal(k)).astype(np.float32)
    u = ref.uniforms(np.array([12345], dtype=np.int64), np.array([2 ** 33 - 7], dtype=np.int64), n, 1)[0, :, 0]
    assert 0.0 < u.min() and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.01
    for tau, top_k, top_p in ((1.0, 0, 1.0), (0.7, 10, 0.9)):
        codes = np.array([ref.sample_row(l, tau, top_k, top_p, ui)[0] for ui in u])
        order = np.lexsort((np.arange(k), -l.astype(np.float64)))
        p = np.exp(l.astype(np.float64)[order] / np.float32(tau))
        kept0 = top_k if top_k > 0 else k
        p[kept0:] = 0.0
        if top_p < 1.0:
            kept = 1 + int((np.cumsum(p) / p.sum() < np.float32(top_p)).sum())
            p[kept:] = 0.0
        p /= p.sum()
        checked = 0
        for j, code in enumerate(order):
            got = int((codes == code).sum())
            if p[j] == 0.0:
                assert got == 0, (code, got)
            elif p[j] >= 0.01:
                assert abs(got - n * p[j]) <= 5.0 * np.sqrt(n * p[j] * (1.0 - p[j])), (code, got, n * p[j])
                checked += 1
        assert checked >= 5


def test_sampler_rows_are_decided_on_every_gpu_input_set():
    total = undecided = 0
    for name in ref.cases():
        codes, decided, _ = ref.reference(name)
        live = codes >= 0
        assert np.all(decided[~live])
        total += int(live.sum())
        undecided += int((live & ~decided).sum())
        assert int((live & ~decided).sum()) <= 0.001 * max(int(live.sum()), 1), name
    print(f"undecided rows: {undecided} of {total}")
    assert total > 500 and undecided <= 0.001 * total


def test_sampler_settings_that_must_agree():
    """top_k = 1 is greedy, top_p -> 0 keeps one code, and the lowest k wins ties."""
    l = np.array([0.5, 2.0, -1.0, 2.0, -0.0, 0.0], dtype=np.float32)
    for u in (1e-9, 0.3, 0.999999):
        assert ref.sample_row(l, 0.0, 0, 1.0, u) == (1, True)
        assert ref.sample_row(l, 1.0, 1, 1.0, u) == (1, True)
        assert ref.sample_row(l, 1.0, 0, 1e-9, u) == (1, True)
    assert ref.sample_row(l, 1e-3, 2, 1.0, 0.75)[0] == 3      # the two maxima share the mass: the second half is code 3
    assert ref.sample_row(np.full(4, -np.inf, dtype=np.float32), 0.0, 0, 1.0, 0.5)[0] == 0


def test_declared_symbols_are_bound():
    names = ["agx_codes_embed", "agx_codes_embed_backward", "agx_codes_embed_backward_workspace_bytes", "agx_codes_cross_entropy",
             "agx_codes_cross_entropy_workspace_bytes", "agx_codes_cross_entropy_backward", "agx_codes_sample"]
    lib = _lib.load()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.agx_version() == 122
    assert lib.agx_codes_embed_backward_workspace_bytes(2, 5, 3, 7) == 2 * 5 * 7 * 4 + 2 * 5 * 3 * 4
    assert lib.agx_codes_cross_entropy_workspace_bytes(2, 65, 3) == 16 * 7      # ceil(390 / 64) partials
    # refusals on the host, before anything is launched: the supported K, the stage count, a stage larger than K
    assert lib.agx_codes_sample(None, None, None, None, None, None, None, None, None, None, None, 1, 1, 1, 2049, None) == -5
    assert b"2048" in lib.agx_last_error()
    assert lib.agx_codes_embed(None, None, None, None, 1, 1, 65, 4, 4, None) == -5
    assert lib.agx_codes_embed(None, None, None, None, 1, 1, 2, 4, 4, None) == -2
    assert ops.CODES_SAMPLE_MAX_K == ref.MAX_K == 2048 and _lib.CODES_SAMPLE_STREAM == ref.SAMPLE_STREAM
    with pytest.raises(_lib.AgxError, match="MI355X only"):
        ops.codes_embed(torch.zeros(1, 1, 2, dtype=torch.int64), torch.zeros(2, 4, 4))
    from audio_generation_amd.prior import CodePrior
    model = CodePrior(3, (16, 16, 5), 64, 2, 2, 32, 8, 32)
    assert model.embed.shape == (3, 17, 64) and model.head.out_features == 48 and model.codebook_sizes == (16, 16, 5)
    with pytest.raises(_lib.AgxError):
        model(torch.zeros(1, 4, 3, dtype=torch.int64))
