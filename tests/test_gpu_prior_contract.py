"""Memory contract (tests/guarded.py) of the code-prior ops: every output and workspace of ``ops.codes_embed``,
``ops.codes_embed_backward``, ``ops.codes_cross_entropy`` (+ ``_backward``) and ``ops.codes_sample`` sits between guard bands and
starts as poison; so do the inputs, and what a kernel must not read IS the poison -- the indices behind a row's count, the logits
of frames behind it.  A read of either shows as a changed result, a stray store as a damaged guard."""
import numpy as np
import pytest
import torch

from audio_generation_amd import ops
from tests import prior_ref as ref
from tests.guarded import Out, routed, run_contract

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, N, Q, R, D = 3, 5, 3, 17, 20
COUNTS = [N + 1, 2, -1]
TAKEN = [N, 2, 0]
SIZES = (16, 5, 1)


@pytest.fixture(scope="module")
def embed_case():
    rng = np.random.default_rng(91)
    tables = rng.standard_normal((Q, R, D)).astype(np.float32)
    index = rng.integers(-1, R + 1, (B, N, Q))
    dout = rng.standard_normal((B, D, N)).astype(np.float32)
    return tables, index, dout, ref.embed(tables, index, COUNTS), ref.embed_backward(dout, index, R, COUNTS)


def _poisoned(arena, full: torch.Tensor, axis: int):
    """``full`` in the arena with everything behind a row's count left as the arena's poison (frames along ``axis``)."""
    t = arena.empty(tuple(full.shape), dtype=full.dtype)
    for r, c in enumerate(TAKEN):
        sel = [r] + [slice(None)] * (full.dim() - 1)
        sel[axis] = slice(0, c)
        t[tuple(sel)] = full[tuple(sel)].to(DEV)
    return t


def test_embed_memory_contract(embed_case):
    tables, index, _, want, _ = embed_case

    def run(arena):
        idx = _poisoned(arena, torch.from_numpy(index), 1)
        td, counts = arena.place(torch.from_numpy(tables)), arena.place(torch.tensor(COUNTS))
        with routed(arena, ops):
            out = ops.codes_embed(idx, td, counts)
        return [Out("out", out, torch.from_numpy(want), exact=True), Out("tables", td, torch.from_numpy(tables), exact=True),
                Out("counts", counts, torch.tensor(COUNTS), exact=True)]
    assert run_contract(run, DEV)["reproducible"]


def test_embed_backward_memory_contract(embed_case):
    _, index, dout, _, want = embed_case

    def run(arena):
        idx = _poisoned(arena, torch.from_numpy(index), 1)
        dd, counts = arena.place(torch.from_numpy(dout)), arena.place(torch.tensor(COUNTS))
        with routed(arena, ops):                                 # dtables and the workspace come from the arena
            dtables = ops.codes_embed_backward(dd, idx, R, counts)
        return [Out("dtables", dtables, torch.from_numpy(want), tol=2e-4 * max(1.0, float(np.abs(want).max()))),
                Out("dout", dd, torch.from_numpy(dout), exact=True), Out("counts", counts, torch.tensor(COUNTS), exact=True)]
    assert run_contract(run, DEV)["reproducible"]


def test_cross_entropy_memory_contract():
    rng = np.random.default_rng(92)
    t = 65
    logits = (2.0 * rng.standard_normal((B, Q * 16, t))).astype(np.float32)
    target = np.stack([rng.integers(-1, s + 1, (B, t)) for s in SIZES], axis=-1)
    loss, nll, dlogits, n_live = ref.cross_entropy(logits, target, SIZES, 0.5)

    def run(arena):
        ld, td, g = arena.place(torch.from_numpy(logits)), arena.place(torch.from_numpy(target)), arena.place(torch.tensor(0.5))
        with routed(arena, ops):                                 # loss, nll, lse, n_live, the workspace and dlogits
            got_loss, got_nll, lse, got_live = ops.codes_cross_entropy(ld, td, SIZES)
            got_d = ops.codes_cross_entropy_backward(ld, td, lse, got_live, g, SIZES)
        return [Out("loss", got_loss, torch.tensor(loss), tol=2e-5 * max(1.0, abs(loss))),
                Out("nll", got_nll, torch.from_numpy(nll), tol=2e-5 * max(1.0, float(nll.max()))),
                Out("n_live", got_live, torch.tensor(n_live), exact=True),
                Out("dlogits", got_d, torch.from_numpy(dlogits), tol=2e-4 * max(1.0, float(np.abs(dlogits).max()))),
                Out("logits", ld, torch.from_numpy(logits), exact=True), Out("target", td, torch.from_numpy(target), exact=True)]
    assert run_contract(run, DEV)["reproducible"]


def test_sample_memory_contract():
    """The counted case of the sampler tests; the logits of the frames behind a row's count are the poison (NaN, 3.4e38)."""
    c = ref.cases()["counted"]
    want, decided, want_carry = ref.reference("counted")
    assert decided.all()
    b, n = want.shape[:2]
    taken = [int(np.clip(v, 0, n)) for v in c["counts"]]

    def run(arena):
        ld = arena.empty(tuple(c["logits"].shape))
        for r, cnt in enumerate(taken):
            ld[r, :, :cnt] = torch.from_numpy(c["logits"][r, :, :cnt]).to(DEV)
        place = {k: arena.place(torch.from_numpy(c[k])) for k in ("seeds", "frame0", "temperature", "top_k", "top_p", "counts", "stages")}
        carry = arena.place(torch.full((b, len(c["sizes"])), -7, dtype=torch.int64))
        with routed(arena, ops):
            codes = ops.codes_sample(ld, len(c["sizes"]), place["seeds"], place["frame0"], place["temperature"], place["top_k"],
                                     place["top_p"], c["sizes"], place["counts"], place["stages"], carry)
        return [Out("codes", codes, torch.from_numpy(want), exact=True), Out("carry", carry, torch.from_numpy(want_carry), exact=True)] + \
               [Out(k, v, torch.from_numpy(c[k]), exact=True) for k, v in place.items()]
    assert run_contract(run, DEV)["reproducible"]
