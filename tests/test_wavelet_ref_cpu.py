"""tests/wavelet_ref.py on the CPU: the restatement is the oracle's function, its bound is not too tight, and the checks of
tests/test_gpu_wavelet_ops.py tell a defective cascade from a sound one.

1. The restatement equals ``oracle.wavelets`` run in float64 -- ``multires_conv``, ``multires_scale_block`` (whose backward is
   ``group_sum``) and ``wavelet_fold``, gradients through autograd -- within 1e-12 of the largest element, on every case of the GPU
   file.
2. On every random-value case the fp32 oracle lies within 1 x the bound (the GPU file allows 2 x).
3. A float32 emulation of the cascade, tile by tile as the kernel walks it, with one planted defect each:

       far_tap      the farthest tap of both filters dropped at the deepest level (dilation 2^(depth - 1))
       w_reversed   w[lvl] read as w[depth + 1 - lvl]
       halo_cut     the left halo cut at one tile: a tile reads nothing more than 1024 columns before its start
       wrap         an index < 0 reads the end of the previous row instead of 0
       no_wx        the w_x x term omitted

   Every defect breaks the bit-equality of a selector case with its anchor (``no_wx``: the anchor itself becomes gelu(0)).
   ``far_tap``, ``w_reversed``, ``wrap`` and ``no_wx`` also exceed 2 x the bound on a random-value case: with the contracting
   filters the bound stays near 1e-6 at every depth, so even the deepest level's farthest tap is hundreds of allowances away.
   SELECTOR-ONLY: ``halo_cut``.  No random-value case has a halo longer than a tile -- a cascade that long with random filters
   carries nothing measurable that far -- so only the selector cases at (K = 3, depth = 10) and (3, 13) see a cut halo.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import wavelets as owv
from tests import wavelet_ref as ref

REL = 1e-12
TILE = 1024
DEFECTS = ["far_tap", "w_reversed", "halo_cut", "wrap", "no_wx"]
SELECTOR_ONLY = {"halo_cut"}


def _close(got, want, what):
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    assert err <= REL * max(scale, 1e-300), (what, err, scale)


def _oracle_grads(x, dout, h0, h1, w, depth, dtype):
    ps = [t.to(dtype).clone().requires_grad_() for t in (x, h0, h1, w)]
    owv.multires_conv(*ps, depth).backward(dout.to(dtype))
    return [torch.zeros_like(p) if p.grad is None else p.grad for p in ps]      # depth 0: the filters are not used


# --------------------------------------------------------------------------- 1, 2: the restatement and its bound
@pytest.mark.parametrize("case", ref.FWD_RANDOM + [ref.FWD_WIDE], ids=ref.ids(ref.FWD_RANDOM + [ref.FWD_WIDE]))
def test_multires_is_the_oracle_and_the_bound_holds_the_fp32_oracle(case):
    x, h0, h1, w = ref.multires_inputs(case)
    y, pre, bound = ref.multires(x, h0, h1, w, case[1])
    _close(y, owv.multires_conv(x.double(), h0.double(), h1.double(), w.double(), case[1]), case)
    ratio = float(((owv.multires_conv(x, h0, h1, w, case[1]).double() - y).abs() / bound.clamp_min(1e-300)).max())
    print(f"multires {case}: fp32 oracle / bound {ratio:.3f}, largest bound {float(bound.max()):.3e}")
    assert ratio <= 1.0 and float(bound.max()) < 1e-5


@pytest.mark.parametrize("case", ref.BWD_RANDOM, ids=ref.ids(ref.BWD_RANDOM))
def test_multires_backward_is_autograd_and_the_bound_holds_the_fp32_oracle(case):
    x, dout, h0, h1, w = ref.multires_inputs(case, backward=True)
    vals, bounds = ref.multires_backward(x, dout, h0, h1, w, case[1])
    for name, v, bd, g64, g32 in zip(("dx", "dh0", "dh1", "dw"), vals, bounds, _oracle_grads(x, dout, h0, h1, w, case[1], torch.float64),
                                     _oracle_grads(x, dout, h0, h1, w, case[1], torch.float32)):
        _close(v, g64, (case, name))
        ratio = float(((g32.double() - v).abs() / bd.clamp_min(1e-300)).max())
        print(f"multires backward {case} {name}: fp32 oracle / bound {ratio:.3f}")
        assert ratio <= 1.0, (case, name)
    if case[1] == 0:
        assert float(vals[1].abs().max()) == 0.0 and float(vals[2].abs().max()) == 0.0


@pytest.mark.parametrize("k,depth,n", ref.FWD_SELECT + ref.BWD_SELECT)
def test_selector_identity_in_the_restatement(k, depth, n):
    """pre IS the delayed input, bit for bit, and dx the advanced dpre; the parameter gradients equal autograd's."""
    gen = torch.Generator().manual_seed(k + depth)
    x, dout = torch.randn(2, 2, n, generator=gen), torch.randn(2, 2, n, generator=gen)
    backward = (k, depth, n) in ref.BWD_SELECT
    for i, a, b in ref.selectors(k, depth):
        h0, h1, w = ref.selector_params(2, k, depth, i, a, b)
        off = ref.selector_offset(k, depth, i, a, b)
        y, pre, _ = ref.multires(x, h0, h1, w, depth)
        assert torch.equal(pre, ref.shifted(x, off).double()), (k, depth, i, a, b)
        _close(y, owv.multires_conv(x.double(), h0.double(), h1.double(), w.double(), depth), (k, depth, i, a, b))
        if backward:
            vals, _ = ref.multires_backward(x, dout, h0, h1, w, depth)
            dpre = dout.double() * ref.gelu_grad(pre)
            assert torch.equal(vals[0], ref.shifted(dpre, -off)), (k, depth, i, a, b)
            for v, g in zip(vals, _oracle_grads(x, dout, h0, h1, w, depth, torch.float64)):
                _close(v, g, (k, depth, i, a, b))


@pytest.mark.parametrize("channelwise", [False, True])
@pytest.mark.parametrize("case", sorted(set(ref.FOLD + ref.FOLD_BWD)))
def test_fold_is_the_oracle_and_the_bound_holds_the_fp32_oracle(case, channelwise):
    h, dout, space, sigma = ref.fold_inputs(case, channelwise)
    y, bound = ref.fold(h, space, sigma, case[0])
    (dh, dsig), (d_dh, d_dsig) = ref.fold_backward(h, dout, space, sigma, case[0])
    grads = {}
    for dtype in (torch.float64, torch.float32):
        hh, ss = h.to(dtype).clone().requires_grad_(), sigma.to(dtype).clone().requires_grad_()
        out = owv.wavelet_fold(hh, space.to(dtype), ss, case[0])
        out.backward(dout.to(dtype))
        grads[dtype] = (out.detach(), hh.grad, ss.grad)
    for name, v, bd, g64, g32 in zip(("y", "dh", "dsigma"), (y, dh, dsig), (bound, d_dh, d_dsig), grads[torch.float64], grads[torch.float32]):
        _close(v, g64, (case, name))
        ratio = float(((g32.double() - v).abs() / bd.clamp_min(1e-300)).max())
        print(f"fold {case} channelwise={channelwise} {name}: fp32 oracle / bound {ratio:.3f}")
        assert ratio <= 1.0, (case, name)


@pytest.mark.parametrize("group,n_out,with_pre", ref.GROUP_SUM)
def test_group_sum_is_the_backward_of_the_scale_block(group, n_out, with_pre):
    """``multires_scale_block`` = multires -> upsample by ``group`` -> 1x1 conv -> GELU: with an identity conv, the gradient at the
    multires output is group_sum of (dout gelu'(upsampled)), and at its pre-activation group_sum(.., gelu_pre)."""
    gen = torch.Generator().manual_seed(group + n_out)
    c = 3
    g = torch.randn(2, c, n_out * group, generator=gen)
    pre = torch.randn(2, c, n_out, generator=gen) if with_pre else None
    out, bound = ref.group_sum(g, group, pre)
    v = (pre if with_pre else torch.randn(2, c, n_out, generator=gen)).double().requires_grad_()
    up = (F.gelu(v) if with_pre else v).repeat_interleave(group, dim=-1)
    up.backward(g.double())
    _close(out, v.grad, (group, n_out, with_pre))
    s32 = g.reshape(2, c, n_out, group).sum(-1)
    got32 = s32 if pre is None else s32 * ref.gelu_grad(pre.double()).float()
    assert bool(((got32.double() - out).abs() <= bound).all())
    # the block itself, in float64: identity 1x1 conv, no level
    x = torch.randn(2, c, n_out, generator=gen).double().requires_grad_()
    h, _, w = ref.selector_params(c, 1, 0, 1, 0, 0)
    blk = owv.multires_scale_block(x, h.double(), h.double(), w.double(), 0, torch.eye(c, dtype=torch.float64)[:, :, None], None, group)
    blk.backward(g.double())
    y = ref.gelu(x.detach())
    want, _ = ref.group_sum(g.double() * ref.gelu_grad(y.repeat_interleave(group, dim=-1)), group, x.detach())
    _close(want, x.grad, (group, n_out, "block"))


# --------------------------------------------------------------------------- 3: the checks discriminate
def _cascade32(x, h0, h1, w, depth, defect=None):
    """The cascade in float32 on whole rows (zero history)."""
    k = h0.shape[-1]
    wc = w[None, :, :, None]
    low, acc = x, torch.zeros_like(x)
    for j in range(depth):
        lvl = depth - j
        idx = torch.arange(x.shape[-1]).reshape(-1, 1) - (k - 1 - torch.arange(k)) * (1 << j)
        taps = torch.where(idx >= 0, low[..., idx.clamp(min=0)], torch.zeros(()))
        f0, f1 = h0[:, 0].clone(), h1[:, 0].clone()
        if defect == "far_tap" and j == depth - 1:
            f0[:, 0], f1[:, 0] = 0.0, 0.0
        wl = wc[:, :, depth + 1 - lvl] if defect == "w_reversed" else wc[:, :, lvl]
        acc = acc + wl * torch.einsum("ck,bclk->bcl", f1, taps)
        low = torch.einsum("ck,bclk->bcl", f0, taps)
    pre = acc + wc[:, :, 0] * low
    return pre if defect == "no_wx" else pre + wc[:, :, depth + 1] * x


def emulate(x, h0, h1, w, depth, defect=None):
    """The forward kernel's walk in float32: a row is cut in tiles of 1024 outputs, each formed from the tile and its left halo."""
    b, c, n = x.shape
    halo = ref.reach(h0.shape[-1], depth)
    if defect not in ("halo_cut", "wrap", "tiled"):
        return F.gelu(_cascade32(x, h0, h1, w, depth, defect))
    pad = torch.zeros(b, c, halo)
    if defect == "wrap" and halo:
        flat = torch.cat([torch.zeros(halo), x.reshape(-1)])                   # before the first row: nothing to wrap into
        rows = torch.arange(b * c).reshape(-1, 1) * n + torch.arange(halo)
        pad = flat[rows].reshape(b, c, halo)
    ext = torch.cat([pad, x], dim=2)                                           # position halo + t holds column t
    out = torch.empty_like(x)
    for t0 in range(0, n, TILE):
        seen = ext.clone()
        if defect == "halo_cut":
            seen[..., :max(0, halo + t0 - TILE)] = 0.0
        out[..., t0:t0 + TILE] = _cascade32(seen, h0, h1, w, depth)[..., halo + t0:halo + t0 + TILE]
    return F.gelu(out)


def _selector_broken(defect):
    """Does ``defect`` break the bit-equality of some selector case with its depth-0 anchor?"""
    for k, depth, n in ref.FWD_SELECT:
        gen = torch.Generator().manual_seed(k + depth)
        x = torch.randn(2, 2, n, generator=gen)
        for i, a, b in ref.selectors(k, depth):
            got = emulate(x, *ref.selector_params(2, k, depth, i, a, b), depth, defect)
            anchor = emulate(ref.shifted(x, ref.selector_offset(k, depth, i, a, b)), *ref.anchor_params(2), 0, defect)
            if defect is None:
                assert torch.equal(got, anchor), (k, depth, i, a, b)
            elif not torch.equal(got, anchor):
                return True
    return False


def _random_broken(defect):
    """Does ``defect`` exceed 2 x the bound on some random-value case?  Prints the worst ratio per case."""
    worst = 0.0
    for case in ref.FWD_RANDOM[:-1] + [ref.FWD_WIDE]:                          # the 70000-row case adds no shape of the cascade
        x, h0, h1, w = ref.multires_inputs(case)
        y, _, bound = ref.multires(x, h0, h1, w, case[1])
        ratio = float(((emulate(x, h0, h1, w, case[1], defect).double() - y).abs() / (2.0 * bound).clamp_min(1e-300)).max())
        print(f"{defect} {case}: error / allowance {ratio:.3f}")
        worst = max(worst, ratio)
    return worst > 1.0


def test_the_sound_emulation_passes_every_check():
    assert not _selector_broken(None) and not _random_broken(None)
    assert not _selector_broken("tiled") and not _random_broken("tiled")       # the tile walk alone, no defect


@pytest.mark.parametrize("defect", DEFECTS)
def test_a_planted_defect_is_caught(defect):
    assert _selector_broken(defect), f"{defect}: no selector case sees it"
    assert _random_broken(defect) == (defect not in SELECTOR_ONLY), defect


@pytest.mark.parametrize("s,p,n", [(5, 40, 41), (8, 256, 33), (256, 256, 3), (4, 8, 7), (1, 4, 19)])
def test_the_int64_fold_reference_is_the_oracle_with_a_flat_wavelet(s, p, n):
    from tests.test_gpu_wavelet_ops import _int_fold
    h = torch.randint(-3, 4, (2, 3, n), generator=torch.Generator().manual_seed(s + p + n)).float()
    want = owv.wavelet_fold(h.double(), torch.zeros(p, dtype=torch.float64), torch.full((1, 3, 1, 1), 40.0, dtype=torch.float64), s)
    assert torch.equal(want.long(), _int_fold(h, p, s)) and torch.equal(want, want.round())
