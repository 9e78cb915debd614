"""The channel-wise elementwise kernels share one header (no GPU, no build: the sources are read as text).

1. ``csrc/rowwise.hpp`` holds the one definition of each fixed-order sum, walk and host helper of the family; the names the
   copies went by are gone; a kernel that still writes an order out by hand is on a list here, with the reason.
2. The first refusal of the ``ops`` wrappers that were folded onto shared private bodies, as literals recorded from the code
   before they were folded: the order of refusals is behaviour.
"""
import glob
import os
import re

import pytest
import torch

from audio_generation_amd import _lib, ops

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "audio_generation_amd", "csrc")
SOURCES = {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))}

ONCE = ("wave_sum", "block_sum", "sigmoidf", "siluf", "silu_gradf", "all_aligned16", "same_phase16", "flat_blocks", "row_walk", "flat_walk",
        "channel_sum", "kSeg", "kRedSeg")
GONE = ("block_sum_256", "gate_blocks", "shape_ok")


def _definitions(name: str):
    """(file, line) of every ``inline <type> NAME(`` and ``constexpr ... NAME =``."""
    pattern = re.compile(rf"\binline\s+[\w:<>]+\s+[*&]?{name}\s*\(|\bconstexpr\b[^;=(]*\b{name}\s*=")
    return [(f, text.count("\n", 0, m.start()) + 1) for f, text in SOURCES.items() for m in pattern.finditer(text)]


@pytest.mark.parametrize("name", ONCE)
def test_defined_once_in_the_header(name):
    found = _definitions(name)
    assert len(found) == 1 and found[0][0] == "rowwise.hpp", (name, found)


def test_the_header_is_found_by_the_definition_pattern():
    assert _definitions("groups_sum") == [("rowwise.hpp", SOURCES["rowwise.hpp"][:SOURCES["rowwise.hpp"].index("groups_sum(")].count("\n") + 1)]
    assert _definitions("mrb_block_sum") == [] and _definitions("no_such_name") == []      # a prefix is another name


@pytest.mark.parametrize("name", GONE)
def test_the_copies_names_are_gone(name):
    assert [f for f, text in SOURCES.items() if re.search(rf"\b{name}\b", text)] == []


# The family's files, and in each the orders still written out by hand: {file: {order: (count, why)}}.  Device code is the
# criterion: a site was converted where the kernel came out instruction for instruction as before, and left where it did not.
FAMILY = ("rowwise.hpp", "conditioning.hip", "snake.hip", "conformer.hip", "disc.hip", "wavelet.hip")
ORDERS = {
    "groups": r"\[0\]\S*\s*\+\s*\S+\[1\]\S*\)\s*\+\s*\(\S+\[2\]",       # (x[0] + x[1]) + (x[2] + x[3])
    "wave": r"__shfl_xor\(",
    "finish": r"\bb = p / \w+;",
}
BY_HAND = {
    "rowwise.hpp": {"groups": (2, "block_sum and groups_sum themselves"),
                    "wave": (2, "wave_sum, and block_sum: a nested call of wave_sum reschedules the LDS store in four kernels of disc.hip"),
                    "finish": (1, "channel_sum itself")},
    "conditioning.hip": {"groups": (2, "film_bwd_tc_kernel: the groups are LDS rows of one lane's channel, the walkers of a group registers")},
    "conformer.hip": {"groups": (1, "glu_dwconv_bwd_kernel: a call of groups_sum swaps two instructions of the loop set-up"),
                      "wave": (3, "bn_stats_finish_kernel: one line, the Chan merge of (n, mean, M2) in the wave order"),
                      "finish": (3, "bn_stats_finish_kernel (a merge, not a sum); bn_silu_bwd_finish_kernel (two slots in one pass: two "
                                    "calls walk the partials twice); glu_dwconv_bwd_finish_kernel (a call moves the invariant index "
                                    "arithmetic of the slot loop)")},
    "disc.hip": {"groups": (3, "sn_wt_u_kernel: four row slices of a column; reduce kernels: four accumulators of one thread"),
                 "wave": (1, "sn_w_v_kernel: a wavefront per row, no workgroup sum")},
    "wavelet.hip": {"wave": (4, "mrb_block_sum (a call of wave_sum reschedules its store), the two filter sums of a level that share "
                                "one loop, the dsigma sum of wavelet_fold_bwd_kernel")},
}


def test_orders_written_out_by_hand_are_the_listed_ones():
    found = {f: {o: len(re.findall(p, SOURCES[f])) for o, p in ORDERS.items()} for f in FAMILY}
    found = {f: {o: n for o, n in orders.items() if n} for f, orders in found.items()}
    assert found == {f: {o: n for o, (n, _) in BY_HAND.get(f, {}).items()} for f in FAMILY}
    assert all(why for orders in BY_HAND.values() for _, why in orders.values())


# ------------------------------------------------------------------------------------------------- the wrappers' first refusal
z = torch.zeros
K1 = ops.CONFORMER_MAX_K + 1
F64 = torch.float64
CPU = "AgxError: audio_generation_amd runs on the MI355X only: got a tensor on 'cpu'.  There is no CPU / eager fallback."
OUT = "out must be a contiguous float32 tensor of x's shape"
U = "u must be a contiguous float32 (B, 2 C, T) tensor"


def strided(*shape):
    """A non-contiguous float32 tensor of ``shape``."""
    return z(*shape[:-1], 2 * shape[-1])[..., ::2]


# (the call and its faults, on the host alone -- ``_need_gpu`` switched off -- or as it stands, the call, the first refusal as recorded)
BAD_CALLS = (
    ("glu_dwconv: u float64", True, lambda: ops.glu_dwconv(z(1, 4, 8, dtype=F64), z(2, 1, 3), z(2)),
     f"AgxError: glu_dwconv: {U}, got (1, 4, 8) torch.float64"),
    ("glu_dwconv: u strided", True, lambda: ops.glu_dwconv(strided(1, 4, 8), z(2, 1, 3), z(2)),
     f"AgxError: glu_dwconv: {U}, got (1, 4, 8) torch.float32"),
    ("glu_dwconv: K out of range + bias of 3", True, lambda: ops.glu_dwconv(z(1, 4, 8), z(2, 1, K1), z(3)),
     f"AgxError: glu_dwconv: kernel_size = {K1} is outside [1, {K1 - 1}]"),
    ("glu_dwconv: w float64 + bias of 3", True, lambda: ops.glu_dwconv(z(1, 4, 8), z(2, 1, 3, dtype=F64), z(3)),
     "AgxError: expected float32, got torch.float64"),
    ("glu_dwconv: CPU tensor", False, lambda: ops.glu_dwconv(z(1, 4, 8), z(2, 1, 3), z(2)), CPU),
    ("glu_dwconv_causal: hist of 3 frames for K = 3", True, lambda: ops.glu_dwconv_causal(z(1, 4, 8), z(2, 1, 3), z(2), hist=z(1, 2, 3)),
     "AgxError: glu_dwconv_causal: hist must be a contiguous float32 (1, 2, 2) tensor (B, C, K - 1), got (1, 2, 3) torch.float32"),
    ("glu_dwconv_causal: hist strided", True, lambda: ops.glu_dwconv_causal(z(1, 4, 8), z(2, 1, 3), z(2), hist=strided(1, 2, 2)),
     "AgxError: glu_dwconv_causal: hist must be a contiguous float32 (1, 2, 2) tensor (B, C, K - 1), got (1, 2, 2) torch.float32"),
    ("glu_dwconv_causal: K out of range + bad hist", True, lambda: ops.glu_dwconv_causal(z(1, 4, 8), z(2, 1, K1), z(2), hist=z(1, 2, 3)),
     f"AgxError: glu_dwconv_causal: kernel_size = {K1} is outside [1, {K1 - 1}]"),
    ("glu_dwconv_causal: bn vector of 3 + bad hist", True,
     lambda: ops.glu_dwconv_causal(z(1, 4, 8), z(2, 1, 3), z(2), bn=(z(2), z(3), z(2), z(2)), hist=z(1, 2, 3)),
     "AgxError: glu_dwconv_causal: a per-channel vector holds 3 floats, the tensor has 2 channels"),
    ("glu_dwconv_causal: CPU hist", False, lambda: ops.glu_dwconv_causal(z(1, 4, 8), z(2, 1, 3), z(2), hist=z(1, 2, 2)), CPU),
    ("glu_dwconv_backward: u strided + dz of another length", True, lambda: ops.glu_dwconv_backward(z(1, 2, 7), strided(1, 4, 8), z(2, 1, 3)),
     f"AgxError: glu_dwconv_backward: {U}, got (1, 4, 8) torch.float32"),
    ("glu_dwconv_backward: dz of another length + w float64", True, lambda: ops.glu_dwconv_backward(z(1, 2, 7), z(1, 4, 8), z(2, 1, 3, dtype=F64)),
     "AgxError: glu_dwconv_backward: dz is (1, 2, 7), expected (1, 2, 8)"),
    ("glu_dwconv_backward: dz float64", True, lambda: ops.glu_dwconv_backward(z(1, 2, 8, dtype=F64), z(1, 4, 8), z(2, 1, 3)),
     "AgxError: expected float32, got torch.float64"),
    ("glu_dwconv_causal_backward: K out of range + dz of another length", True,
     lambda: ops.glu_dwconv_causal_backward(z(1, 2, 7), z(1, 4, 8), z(2, 1, K1)),
     f"AgxError: glu_dwconv_causal_backward: kernel_size = {K1} is outside [1, {K1 - 1}]"),
    ("glu_dwconv_causal_backward: dz of another length", True, lambda: ops.glu_dwconv_causal_backward(z(1, 2, 7), z(1, 4, 8), z(2, 1, 3)),
     "AgxError: glu_dwconv_causal_backward: dz is (1, 2, 7), expected (1, 2, 8)"),
    ("glu_dwconv_causal_backward: CPU tensor", False, lambda: ops.glu_dwconv_causal_backward(z(1, 2, 8), z(1, 4, 8), z(2, 1, 3)), CPU),
    ("film_apply: layout 7 + x strided", True, lambda: ops.film_apply(strided(2, 3, 8), z(2, 6), True, layout=7),
     "AgxError: film_apply: layout = 7 is neither FILM_CT nor FILM_TC"),
    ("film_apply: x strided + out of another shape", True, lambda: ops.film_apply(strided(2, 3, 8), z(2, 6), True, out=z(2, 3, 7)),
     "AgxError: film_apply: x must be a contiguous float32 tensor"),
    ("film_apply: x float64", True, lambda: ops.film_apply(z(2, 3, 8, dtype=F64), z(2, 6), True),
     "AgxError: film_apply: x must be a contiguous float32 tensor"),
    ("film_apply: out of another shape + gb float64", True, lambda: ops.film_apply(z(2, 3, 8), z(2, 6, dtype=F64), True, out=z(2, 3, 7)),
     f"AgxError: film_apply: {OUT}"),
    ("sigmoid_gate: z of another shape + out of another shape", True, lambda: ops.sigmoid_gate(z(2, 8), z(2, 7), out=z(2, 7)),
     "AgxError: sigmoid_gate: x must be a contiguous float32 tensor and z of its shape (x (2, 8), z (2, 7))"),
    ("sigmoid_gate: out strided", True, lambda: ops.sigmoid_gate(z(2, 8), z(2, 8), out=strided(2, 8)), f"AgxError: sigmoid_gate: {OUT}"),
    ("snake_forward: x strided", True, lambda: ops.snake_forward(strided(2, 3, 8), z(3), ops.SNAKE_PLAIN),
     "AgxError: snake_forward: x must be a contiguous float32 tensor (x (2, 3, 8), torch.float32)"),
    ("snake_forward: alpha of 4 + out of another shape", True, lambda: ops.snake_forward(z(2, 3, 8), z(4), ops.SNAKE_PLAIN, out=z(2, 3, 7)),
     "AgxError: snake_forward: x is (2, 3, 8) and has 3 channels, alpha (4,) holds 4"),
    ("snake_forward: out float64", True, lambda: ops.snake_forward(z(2, 3, 8), z(3), ops.SNAKE_RELU, out=z(2, 3, 8, dtype=F64)),
     f"AgxError: snake_forward: {OUT}"),
    ("bn_silu: z float64", True, lambda: ops.bn_silu(z(1, 2, 8, dtype=F64), z(2), z(2), z(2), z(2)),
     "AgxError: bn_silu: operands must be contiguous float32 tensors of one shape (1, 2, 8), got (1, 2, 8) torch.float64"),
    ("bn_silu: gamma of 3 + out of another shape", True, lambda: ops.bn_silu(z(1, 2, 8), z(3), z(2), z(2), z(2), out=z(1, 2, 7)),
     "AgxError: bn_silu: a per-channel vector holds 3 floats, the tensor has 2 channels"),
    ("bn_silu: out of another shape", True, lambda: ops.bn_silu(z(1, 2, 8), z(2), z(2), z(2), z(2), out=z(1, 2, 7)), f"AgxError: bn_silu: {OUT}"),
    ("silu: x strided + out of another shape", True, lambda: ops.silu(strided(4, 8), out=z(4, 7)), "AgxError: silu: x must be a contiguous float32 tensor"),
    ("silu: out of another shape", True, lambda: ops.silu(z(4, 8), out=z(4, 7)), f"AgxError: silu: {OUT}"),
    ("silu: CPU out", False, lambda: ops.silu(z(4, 8), out=z(4, 8)), CPU),
    ("silu_backward: dout of another shape + out of another shape", True, lambda: ops.silu_backward(z(4), z(5), out=z(5)),
     "AgxError: silu_backward: x and dout must be contiguous float32 tensors of one shape (x (4,), dout (5,))"),
    ("silu_backward: out float64", True, lambda: ops.silu_backward(z(4), z(4), out=z(4, dtype=F64)), f"AgxError: silu_backward: {OUT}"),
)


@pytest.mark.parametrize("what,host,call,first", BAD_CALLS, ids=[c[0] for c in BAD_CALLS])
def test_first_refusal_is_the_one_of_before(monkeypatch, what, host, call, first):
    monkeypatch.setattr(_lib, "load", lambda: None)            # no refusal needs the library: nothing reaches a launch
    if host:
        monkeypatch.setattr(ops, "_need_gpu", lambda *tensors: None)
    with pytest.raises(_lib.AgxError) as e:
        call()
    assert f"{type(e.value).__name__}: {e.value}" == first
