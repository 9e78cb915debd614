"""Memory contract of the two staged quantiser entries (``agx_rvq_forward_staged``, ``agx_rvq_backward_staged``) on the
guarded, poisoned arena of ``tests/guarded.py``: inputs (``stages`` among them), outputs and workspaces sit between guard bands
and every byte the ops do not own holds 0x00, 0xFF or 0x7F in turn.  Guards must stay intact, no output may depend on what its
buffer or a workspace held before -- the rows ``S_q`` of dead stages are never written, so they must never be read either --,
the inputs must come back unchanged, and the two runs on clean memory must agree bit for bit.  One parametrisation puts
``stages`` on a view 8 bytes off a 16-byte boundary.  Values: tests/rvq_dropout_ref.py, computed once."""
import pytest
import torch

from audio_generation_amd import _lib, ops
from tests import rvq_dropout_ref as ref
from tests.guarded import Out, routed, run_contract

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE, SIZES, STAGES = (3, 5, 20, 24, 2), (24, 17), (2, 0, 1)
_BUILT = {}


def _build():
    if not _BUILT:
        b, t, d, k, q = SHAPE
        gen = torch.Generator().manual_seed(26)
        x = torch.randn(b, t, d, generator=gen)
        cbs = torch.randn(q, k, d, generator=gen)
        for i, kq in enumerate(SIZES):
            cbs[i, kq:] = 0.0
        g_xq = torch.randn(b, t, d, generator=gen)
        g_l = torch.tensor(1.75)
        stages = torch.tensor(STAGES, dtype=torch.int64)
        xq, index, sq_err, commit = ref.forward(x, cbs, STAGES, q, SIZES)
        _BUILT.update(x=x, cbs=cbs, g_xq=g_xq, g_l=g_l, stages=stages, xq=xq, index=index, sq_err=sq_err, commit=commit,
                      want=ref.definition(x, cbs, index, STAGES, g_xq, float(g_l)))
    return _BUILT


@pytest.mark.parametrize("stages_skew", [0, 8])
def test_staged_rvq_memory_contract(stages_skew):
    c = _build()
    b, t, d, k, q = SHAPE
    dx_w, dc_w, bound_dx, bound_dc, chosen, _ = c["want"]
    fwd_ws = int(_lib.load().agx_rvq_workspace_bytes(b, t, d, k, q))
    rel = lambda want: 1e-5 * max(1.0, float(torch.as_tensor(want).abs().max()))      # tests/test_gpu_parity.py, the commit loss

    def case(arena):
        x, cbs, g_xq, g_l = (arena.place(c[key]) for key in ("x", "cbs", "g_xq", "g_l"))
        stages = arena.place(c["stages"], skew=stages_skew)
        assert stages.data_ptr() % 16 == stages_skew
        with routed(arena, ops):
            packed = ops.rvq_pack(cbs, SIZES)
            first = len(arena.allocs)
            xq, idx, sq, commit = ops.rvq_forward(x, cbs, packed, q, stages=stages)
            made = [(a.dtype, a.nbytes) for a in arena.allocs[first:]]
            assert (torch.float64, 8 * q + fwd_ws) in made and len(made) == 4, made        # x_q, index, sq_err | workspace, commit
            first = len(arena.allocs)
            dx, dc = ops.rvq_backward(x, cbs, idx, g_xq, g_l, want_codebook_grad=True, stages=stages)
            made = [(a.dtype, a.nbytes) for a in arena.allocs[first:]]
            assert (torch.uint8, 4 * q * b * t * d) in made and len(made) == 3, made       # dx, dC, workspace
        outs = [Out("index", idx, c["index"], exact=True), Out("x_q", xq, c["xq"], exact=True),
                Out("sq_err", sq, c["sq_err"], rel(c["sq_err"])),
                Out("commit", commit.reshape(1), torch.tensor([c["commit"]], dtype=torch.float64), rel(c["commit"])),
                Out("dx", dx, dx_w, float(bound_dx.max())), Out("dC", dc, dc_w, float(bound_dc.max())),
                Out("dx of the row without stages", dx[1], c["g_xq"][1], exact=True),
                Out("dC rows no frame chose", dc[~chosen.to(dc.device)], torch.zeros(int((~chosen).sum()), d), exact=True)]
        outs += [Out(f"{key} unchanged", got, c[key], exact=True)
                 for key, got in (("x", x), ("cbs", cbs), ("g_xq", g_xq), ("g_l", g_l), ("stages", stages))]
        return outs
    report = run_contract(case, DEV)
    assert report["reproducible"], report["irreproducible"]
