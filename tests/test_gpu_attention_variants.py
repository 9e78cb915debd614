"""Every row of the three forward attention tables (csrc/attention.hip: ``attn_pick``) launched once, at the smallest shape that
selects it: the name query answers with the row, and the row's launch thunk computes the definition.  A table can attach a
wrong thunk to a right name; the name alone (tests/test_attention_kernel_names_cpu.py) would not notice."""
import pytest
import torch

from audio_generation_amd import ops
from oracle import attention as oattn
from tests.helpers import max_abs, rms
from tests.test_gpu_attention_flash import BF16_MAX_REL, BF16_RMS_REL, _core

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H = 1, 2
DVT = {32: 1, 64: 2, 72: 4}

CASES = [(t, dh, ops.ATTN_FP32, f"attention_alibi<{nj},{DVT[dh]}>") for t, nj in ((64, 2), (65, 4), (129, 8)) for dh in DVT]
CASES += [(257, dh, ops.ATTN_FP32, f"attention_flash<{DVT[dh]},0>") for dh in DVT]
CASES += [(64, dh, ops.ATTN_BF16, f"attention_bf16_lds<{DVT[dh]}>") for dh in DVT]
CASES += [(1025, 32, ops.ATTN_BF16, "attention_flash<1,1>"), (513, 64, ops.ATTN_BF16, "attention_flash<2,1>"),
          (257, 72, ops.ATTN_BF16, "attention_flash<4,1>")]


def test_the_cases_are_all_eighteen_rows():
    assert len({name for *_, name in CASES}) == len(CASES) == 9 + 6 + 3


@pytest.mark.parametrize("t,dh,precision,name", CASES)
def test_each_row_is_named_and_computes_the_definition(t, dh, precision, name):
    assert ops.attention_kernel_name(B, H, dh, t, precision) == name
    qkv = 0.7 * torch.randn(B, 3 * H * dh, t, generator=torch.Generator().manual_seed(t + dh))
    want = _core(qkv, H, dh)
    got = ops.attention_alibi(qkv.to(DEV), oattn.alibi_slopes(H).to(DEV), H, dh, dh ** 0.5, precision=precision).cpu()
    scale, e_max = float(want.abs().max()), max_abs(got, want)
    if precision == ops.ATTN_FP32:
        print(f"{name} T={t} Dh={dh}: max err {e_max:.2e}, max|o| {scale:.2e}")
        assert e_max < 3e-5 * max(1.0, scale)
    else:
        want_rms, e_rms = float(want.pow(2).mean().sqrt()), rms(got, want)
        print(f"{name} T={t} Dh={dh}: max err {e_max / scale:.2e} of max|o|, rms err {e_rms / want_rms:.2e} of rms(o)")
        assert e_max <= BF16_MAX_REL * scale and e_rms <= BF16_RMS_REL * want_rms
