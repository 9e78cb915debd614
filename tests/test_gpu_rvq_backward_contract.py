"""Memory contract of ``ops.rvq_backward`` on the guarded, poisoned arena of ``tests/guarded.py``: inputs, outputs and the
workspace sit between guard bands, and every byte the op does not own holds 0x00, 0xFF or 0x7F in turn.  Guards must stay
intact, dx and dC must not depend on what their buffers and the workspace held before, and the two runs on clean memory must
agree bit for bit.  The values are checked against the float64 definition of tests/test_gpu_rvq_backward.py, computed once
per case on the indices of the defining search (``oracle.rvq``), with the largest of its per-element bounds as the tolerance."""
import pytest
import torch

from audio_generation_amd import ops
from oracle import rvq
from tests.guarded import Out, routed, run_contract
from tests.test_gpu_rvq_backward import definition

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (B, T, D, K, Q), layout
CASES = {"ragged-odd-D": ((1, 37, 33, 100, 3), "b l c"), "K1024-channel-major": ((2, 19, 64, 1024, 2), "b c l")}
_BUILT = {}


def _build(name):
    if name not in _BUILT:
        (b, t, d, k, q), layout = CASES[name]
        gen = torch.Generator().manual_seed(sum(map(ord, name)))
        x = torch.randn(b, t, d, generator=gen)
        cbs = torch.randn(q, k, d, generator=gen)
        g_xq = torch.randn(b, t, d, generator=gen)
        g_l = torch.tensor(1.75)
        _, idx, _ = rvq.residual_quantize(x, cbs)
        want = definition(x, cbs, idx, g_xq, float(g_l))
        major = (lambda v: v.transpose(1, 2).contiguous()) if layout == "b c l" else (lambda v: v)
        _BUILT[name] = dict(x=major(x), cbs=cbs, idx=idx.contiguous(), g_xq=major(g_xq), g_l=g_l, want=want, major=major,
                            ws_bytes=4 * q * b * t * d, layout=layout)
    return _BUILT[name]


@pytest.mark.parametrize("name", list(CASES))
def test_rvq_backward_memory_contract(name):
    c = _build(name)
    dx_w, dc_w, bound_dx, bound_dc, chosen, _ = c["want"]

    def case(arena):
        x, cbs, idx, g_xq, g_l = (arena.place(c[key]) for key in ("x", "cbs", "idx", "g_xq", "g_l"))
        first = len(arena.allocs)
        with routed(arena, ops):
            dx, dc = ops.rvq_backward(x, cbs, idx, g_xq, g_l, c["layout"], want_codebook_grad=True)
        made = [(a.dtype, a.nbytes) for a in arena.allocs[first:]]
        assert (torch.uint8, c["ws_bytes"]) in made, "the workspace is exactly what agx_rvq_backward_workspace_bytes answers"
        assert len(made) == 3, made                                   # dx, dC, workspace: nothing else is allocated
        return [Out("dx", dx, c["major"](dx_w), float(bound_dx.max())),
                Out("dC", dc, dc_w, float(bound_dc.max())),
                Out("dC rows no frame chose", dc[~chosen.to(dc.device)], torch.zeros(int((~chosen).sum()), dc.shape[2]), exact=True)]
    report = run_contract(case, DEV)
    assert report["reproducible"], report["irreproducible"]
