"""The Conformer classes of ``audio_generation_amd.transformers`` on the host: surface, state dicts, refusals, the return codes
of the C entry points that need no launch, and the float64 restatement of ``tests/conformer_ref.py`` pinned to the goldens of
the reference (``tests/golden/make_goldens_conformer.py``) and to a float64 composition of ``torch.nn.functional`` ops under
autograd, gradients included.

Tolerance against the goldens: they are the reference's own fp32 evaluation, whose sums have at most 64 terms (the hidden width
of the golden block) of magnitude about the result's: 64 u = 4e-6 relative to the tensor's scale per layer, a handful of layers
deep -- 2e-5 max(1, scale) on every tensor.  Against float64 autograd the restatement is held to 1e-10 max(1, scale): 2^-53 = 1e-16, times the conditioning of the
batch-statistics gradient (dbias sums a dz that cancels to zero; rstd reaches 10 on 21 samples)."""
import ctypes
import json
import os
import warnings

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from audio_generation_amd import _lib, ops
from audio_generation_amd._lib import AgxError
from audio_generation_amd.transformers import ConformerBlock, ConformerConvBlock, FeedForward
from tests import conformer_ref as ref
from tests.helpers import GOLDEN, load_npz, sub_sd

OK, BAD_SHAPE, NULL_POINTER, WORKSPACE = 0, -1, -2, -3
MODELS = ("conv_k17", "conv_k4", "block")


@pytest.fixture(scope="module")
def lib():
    from audio_generation_amd import build
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def g12():
    with open(os.path.join(GOLDEN, "meta_g12.json")) as f:
        return load_npz("g12_conformer.npz"), json.load(f)


def _build(meta, name):
    m = meta["models"][name]
    kw = dict(m["kwargs"])
    if m["class"] == "ConformerBlock":
        return ConformerBlock(kw.pop("dim"), **kw)
    return ConformerConvBlock(kw.pop("in_channels"), **kw)


def _close(got, want, tol, what):
    want = torch.as_tensor(want).double()
    err, scale = float((got.double() - want).abs().max()), float(want.abs().max())
    print(f"{what}: err {err:.3e}, max|ref| {scale:.3e}")
    assert got.shape == want.shape and err < tol * max(1.0, scale), what


# ------------------------------------------------------------------------------------------------ surface
@pytest.mark.parametrize("name", MODELS)
def test_construction_and_state_dict_are_the_references(name, g12):
    blob, meta = g12
    model = _build(meta, name)
    m = meta["models"][name]
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == m["state_dict"]
    assert list(model.state_dict()) == list(m["state_dict"])
    assert [n for n, _ in model.named_parameters()] == m["parameters"]
    model.load_state_dict(sub_sd(blob, f"{name}/sd/"))


def test_children_and_layout():
    block = ConformerBlock(64, heads=4, kernel_size=9, context_x=40)
    assert [n for n, _ in block.named_children()] == ["first_ff", "attention", "conv_block", "second_ff", "layer_norm"]
    assert block.attention.dim_head == 16 and block.attention.context == 40 and block.conv_block.kernel_size == 9
    assert block.first_ff.net[1].out_features == 256 and isinstance(block.first_ff.net[2], nn.SiLU)
    conv = ConformerConvBlock(8)
    kinds = [type(m) for m in conv.net]
    assert kinds == [nn.LayerNorm, nn.Conv1d, nn.GLU, nn.Conv1d, nn.BatchNorm1d, nn.SiLU, nn.Conv1d, nn.Dropout]
    assert conv.net[3].groups == 8 and conv.net[3].kernel_size == (17,) and conv.net[3].padding == "same" and conv.net[7].p == 0.1
    assert isinstance(ConformerConvBlock(8, dropout=0.0).net[7], nn.Identity)
    assert ConformerBlock(512).conv_block.net[3].weight.shape == (512, 1, 17)


def test_constructor_errors():
    with pytest.raises(NotImplementedError):
        ConformerConvBlock(8, activation=nn.ReLU)
    with pytest.raises(NotImplementedError):
        ConformerBlock(16, heads=2, conv_activation=nn.GELU)
    with pytest.raises(NotImplementedError):
        ConformerBlock(16, heads=2, ff_activation=nn.Tanh)
    with pytest.raises(NotImplementedError):
        FeedForward(16, 32, activation=nn.Tanh)
    FeedForward(16, 32, activation=nn.SiLU)
    FeedForward(16, 32)
    for k in (0, -1, ops.CONFORMER_MAX_K + 1, 2.5):
        with pytest.raises(ValueError):
            ConformerConvBlock(8, kernel_size=k)
    assert ops.CONFORMER_MAX_K >= 31
    ConformerConvBlock(8, kernel_size=ops.CONFORMER_MAX_K)
    with pytest.raises(TypeError):
        ConformerBlock(16, 4, 2, 0.1, nn.SiLU, nn.SiLU, 17)       # kernel_size and context_x are keyword-only


def test_cpu_tensors_are_refused(lib):
    z = torch.zeros
    for model, shape in ((ConformerBlock(16, heads=2), (2, 5, 16)), (ConformerConvBlock(8), (2, 5, 8)),
                         (FeedForward(16, 32, activation=nn.SiLU), (2, 5, 16))):
        for mode in (True, False):
            model.train(mode)
            with pytest.raises(AgxError, match="MI355X only"):
                model(z(shape))
            with torch.no_grad(), pytest.raises(AgxError, match="MI355X only"):
                model(z(shape))
    for call in (lambda: ops.silu(z(4)), lambda: ops.silu_backward(z(4), z(4)),
                 lambda: ops.glu_dwconv(z(1, 4, 8), z(2, 1, 3), z(2)), lambda: ops.glu_dwconv_backward(z(1, 2, 8), z(1, 4, 8), z(2, 1, 3)),
                 lambda: ops.bn_stats(z(1, 2, 8)), lambda: ops.bn_silu(z(1, 2, 8), z(2), z(2), z(2), z(2)),
                 lambda: ops.bn_silu_backward(z(1, 2, 8), z(1, 2, 8), z(2), z(2), z(2), z(2))):
        with pytest.raises(AgxError, match="MI355X only"):
            call()


def test_wrappers_refuse_mismatched_operands(monkeypatch):
    monkeypatch.setattr(ops, "_need_gpu", lambda *tensors: None)
    z = torch.zeros
    with pytest.raises(AgxError, match="2 C, T"):
        ops.glu_dwconv(z(1, 3, 8), z(1, 1, 3), z(1))
    with pytest.raises(AgxError, match="one filter per channel"):
        ops.glu_dwconv(z(1, 4, 8), z(3, 1, 3), z(2))
    with pytest.raises(AgxError, match="kernel_size"):
        ops.glu_dwconv(z(1, 4, 8), z(2, 1, ops.CONFORMER_MAX_K + 1), z(2))
    with pytest.raises(AgxError, match="per-channel"):
        ops.glu_dwconv(z(1, 4, 8), z(2, 1, 3), z(3))
    with pytest.raises(AgxError, match="dz is"):
        ops.glu_dwconv_backward(z(1, 2, 7), z(1, 4, 8), z(2, 1, 3))
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.bn_stats(z(1, 2, 1))
    with pytest.raises(AgxError, match="per-channel"):
        ops.bn_silu(z(1, 2, 8), z(3), z(2), z(2), z(2))
    with pytest.raises(AgxError, match="one shape"):
        ops.bn_silu_backward(z(1, 2, 7), z(1, 2, 8), z(2), z(2), z(2), z(2))
    with pytest.raises(AgxError, match="one shape"):
        ops.silu_backward(z(4), z(5))


# ------------------------------------------------------------------------------------------------ the C entry points
def test_entry_points_validate_on_the_host(lib):
    assert lib.agx_version() == 122
    buf = ctypes.create_string_buffer(64)          # never dereferenced: every call below is refused or empty
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd, bwd = lib.agx_glu_dwconv_forward, lib.agx_glu_dwconv_backward
    stats, act, act_bwd = lib.agx_bn_stats, lib.agx_bn_silu_forward, lib.agx_bn_silu_backward
    big = 2 ** 20
    for b, c, t, k in ((0, 2, 8, 3), (1, 0, 8, 3), (1, 2, 0, 3), (-1, 2, 8, 3), (1, 2, 8, 0), (1, 2, 8, ops.CONFORMER_MAX_K + 1),
                       (big, big, 1, 3), (big, 4096, 1025, 3)):
        assert fwd(p, p, p, None, None, None, None, 1e-5, p, b, c, t, k, None) == BAD_SHAPE, (b, c, t, k)
        assert bwd(p, p, p, p, p, p, p, 1 << 30, b, c, t, k, None) == BAD_SHAPE
        assert lib.agx_glu_dwconv_backward_workspace_bytes(b, c, t, k) == 0
        if k == 3:
            assert stats(p, p, p, None, None, None, 0.1, p, 1 << 30, b, c, t, None) == BAD_SHAPE
            assert act(p, p, p, p, p, 1e-5, 1, p, b, c, t, None) == BAD_SHAPE
            assert act_bwd(p, p, p, p, p, p, 1e-5, 1, p, p, p, p, 1 << 30, b, c, t, None) == BAD_SHAPE
            assert lib.agx_bn_stats_workspace_bytes(b, c, t) == 0 and lib.agx_bn_silu_backward_workspace_bytes(b, c, t) == 0
    assert b"grid" in lib.agx_last_error()
    assert stats(p, p, p, None, None, None, 0.1, p, 64, 1, 2, 1, None) == BAD_SHAPE and b"more than one value" in lib.agx_last_error()
    # a NULL required pointer, and statistics that come together or not at all
    assert fwd(None, p, p, None, None, None, None, 1e-5, p, 1, 2, 8, 3, None) == NULL_POINTER
    assert fwd(p, p, p, p, None, None, None, 1e-5, p, 1, 2, 8, 3, None) == NULL_POINTER
    assert bwd(p, p, p, p, p, None, p, 1 << 20, 1, 2, 8, 3, None) == NULL_POINTER
    assert bwd(None, p, p, p, None, None, None, 0, 1, 2, 8, 3, None) == NULL_POINTER
    assert bwd(p, p, p, None, None, None, None, 0, 1, 2, 8, 3, None) == OK              # nothing asked for
    assert act_bwd(p, p, p, p, p, p, 1e-5, 1, None, None, None, None, 0, 1, 2, 8, None) == OK
    assert stats(None, p, p, None, None, None, 0.1, p, 64, 1, 2, 8, None) == NULL_POINTER
    assert act(p, None, p, p, p, 1e-5, 1, p, 1, 2, 8, None) == NULL_POINTER
    assert lib.agx_silu(None, p, 4, None) == NULL_POINTER and lib.agx_silu(None, None, 0, None) == OK
    assert lib.agx_silu_backward(p, None, p, 4, None) == NULL_POINTER and lib.agx_silu_backward(None, None, None, -1, None) == OK
    # the workspaces
    seg, tile = ref.SEGMENT, ref.TILE
    assert lib.agx_bn_stats_workspace_bytes(3, 5, seg) == 4 * 2 * 15 and lib.agx_bn_stats_workspace_bytes(3, 5, seg + 1) == 4 * 2 * 30
    assert lib.agx_bn_silu_backward_workspace_bytes(3, 5, seg + 1) == 4 * (2 * 30 + 10)
    assert lib.agx_glu_dwconv_backward_workspace_bytes(3, 5, tile, 17) == 4 * 15 * 18
    assert lib.agx_glu_dwconv_backward_workspace_bytes(3, 5, tile + 1, 4) == 4 * 30 * 5
    assert stats(p, p, p, None, None, None, 0.1, p, 4 * 2 * 15 - 1, 3, 5, seg, None) == WORKSPACE
    assert stats(p, p, p, None, None, None, 0.1, None, 1 << 20, 3, 5, seg, None) == WORKSPACE
    assert act_bwd(p, p, p, p, p, p, 1e-5, 1, p, p, p, p, 4 * 40 - 1, 3, 5, seg, None) == WORKSPACE
    assert bwd(p, p, p, p, p, p, p, 4 * 15 * 18 - 1, 3, 5, tile, 17, None) == WORKSPACE and b"workspace" in lib.agx_last_error()


# ------------------------------------------------------------------------------------------------ the restatement
def _sd64(blob, name, grad=True):
    sd = {k: v.double() for k, v in sub_sd(blob, f"{name}/sd/").items()}
    return {k: (v.requires_grad_() if grad and v.is_floating_point() else v) for k, v in sd.items()}


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("name", MODELS)
def test_the_restatement_reproduces_the_reference(name, mode, g12):
    blob, meta = g12
    m = meta["models"][name]
    sd = _sd64(blob, name)
    x = torch.from_numpy(blob[f"{name}/x"]).double().transpose(1, 2).contiguous().requires_grad_()      # (B, C, T)
    dout = torch.from_numpy(blob[f"{name}/dout"]).double().transpose(1, 2)
    stats, training = {}, mode == "train"
    if m["class"] == "ConformerBlock":
        out = ref.conformer_block(x, sd, m["kwargs"]["heads"], training, stats)
        bn = "conv_block.net.4."
    else:
        out = ref.conv_block(x, sd, "", training, stats)
        bn = "net.4."
    (out * dout).sum().backward()
    tol = 2e-5
    _close(out.detach().transpose(1, 2), blob[f"{name}/{mode}/out"], tol, "out")
    _close(x.grad.transpose(1, 2), blob[f"{name}/{mode}/dx"], tol, "dx")
    for pname in m["parameters"]:
        _close(sd[pname].grad, blob[f"{name}/{mode}/grad/{pname}"], tol, pname)
    r_mean, r_var = sd[bn + "running_mean"].detach(), sd[bn + "running_var"].detach()
    if training:
        r_mean, r_var = ref.running_update(r_mean, r_var, stats["mean"], stats["m2"], stats["n"])
    _close(r_mean, blob[f"{name}/{mode}/after/{bn}running_mean"], tol, "running_mean")
    _close(r_var, blob[f"{name}/{mode}/after/{bn}running_var"], tol, "running_var")
    assert int(blob[f"{name}/{mode}/after/{bn}num_batches_tracked"]) == int(blob[f"{name}/sd/{bn}num_batches_tracked"]) + training


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("k", [1, 3, 4, 17, 31])
def test_the_restatements_formulas_are_autograds(k, training):
    """The hand-written forward and backward formulas against torch.nn.functional under float64 autograd: GLU, the grouped
    "same" conv1d (even K pads as torch does), batch_norm in both modes, SiLU."""
    b, c, t = 3, 5, 7
    gen = torch.Generator().manual_seed(k)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    u, w, bias, gamma, beta = (v.requires_grad_() for v in (r(b, 2 * c, t), r(c, 1, k), r(c), r(c), r(c)))
    r_mean, r_var, dy = r(c), 0.5 + torch.rand(c, generator=gen, dtype=torch.float64), r(b, c, t)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z = F.conv1d(F.glu(u, dim=-2), w, bias, padding="same", groups=c)
    z.retain_grad()
    rm, rv = r_mean.clone(), r_var.clone()
    y = F.silu(F.batch_norm(z, rm, rv, gamma, beta, training, 0.1, ref.EPS))
    (y * dy).sum().backward()
    ud, wd, bd, gd, btd = (v.detach() for v in (u, w, bias, gamma, beta))
    z2 = ref.glu_dwconv(ud, wd, bd)
    mean, var, m2 = ref.batch_stats(z2) if training else (r_mean, r_var, None)
    tol = 1e-10
    _close(z2, z.detach(), tol, "z")
    _close(ref.bn_silu(z2, gd, btd, mean, var), y.detach(), tol, "y")
    if training:
        want_rm, want_rv = ref.running_update(r_mean, r_var, mean, m2, b * t)
        _close(want_rm, rm, tol, "running_mean")
        _close(want_rv, rv, tol, "running_var")
    dz, dgamma, dbeta = ref.bn_silu_backward(dy, z2, gd, btd, mean, var, training=training)
    du, dw, dbias = ref.glu_dwconv_backward(dz, ud, wd)
    for name, got, want in (("dz", dz, z.grad), ("dgamma", dgamma, gamma.grad), ("dbeta", dbeta, beta.grad), ("du", du, u.grad),
                            ("dw", dw, w.grad.reshape(c, k)), ("dbias", dbias, bias.grad)):
        _close(got, want, tol, name)
    x = r(b, c, t)
    _close(ref.silu(x), F.silu(x), tol, "silu")
    _close(ref.layer_norm_ct(x, gd, btd), F.layer_norm(x.transpose(1, 2), (c,), gd, btd).transpose(1, 2), tol, "layer_norm_ct")


def test_bounds_are_positive_and_small():
    """Every bound is finite, positive where its quantity is non-zero, and far below the quantity's scale."""
    gen = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    b, c, t, k = 3, 5, 37, 17
    u, w, bias, gamma, beta, dy = r(b, 2 * c, t), r(c, k), r(c), r(c), r(c), r(b, c, t)
    z = ref.glu_dwconv(u, w, bias)
    mean, var, _ = ref.batch_stats(z)
    bounds = [ref.bound_z(u, w, bias), *ref.bound_stats(z), ref.bound_y(z, gamma, beta, mean, var),
              *ref.bound_bn_backward(dy, z, gamma, beta, mean, var), *ref.bound_bn_backward(dy, z, gamma, beta, mean, var, training=False),
              *ref.bound_conv_backward(dy, u, w), *ref.bound_running(z, mean, var)]
    for bound in bounds:
        assert bool(torch.isfinite(bound).all()) and float(bound.min()) > 0.0 and float(bound.max()) < 1e-3


# ------------------------------------------------------------------------------------------------ the launches
from tests.test_transformer_walk_cpu import STANDINS as TRANSFORMER_STANDINS, Recorder as WalkRecorder  # noqa: E402

NEW_OPS = ("glu_dwconv", "glu_dwconv_backward", "bn_stats", "bn_silu", "bn_silu_backward", "silu", "silu_backward")
DROPOUT_OPS = ("dropout_add", "attention_alibi_dropout", "attention_alibi_dropout_backward")
PACKS = ("conv_pack", "conv_pack_bwd")         # images, cached per weight version: not part of a launch list
REAL = {op: getattr(ops, op) for op in TRANSFORMER_STANDINS + NEW_OPS + DROPOUT_OPS}


class Recorder(WalkRecorder):
    def describe(self, v):
        if isinstance(v, (tuple, list)):          # the bn= tuple of glu_dwconv
            return [self.describe(e) for e in v]
        return super().describe(v)

    def result(self, op, a):
        z = torch.zeros
        if op == "glu_dwconv":
            return z(a["u"].shape[0], a["u"].shape[1] // 2, a["u"].shape[2])
        if op == "glu_dwconv_backward":
            return (torch.zeros_like(a["u"]) if a["want_du"] else None, torch.zeros_like(a["w"]) if a["want_params"] else None,
                    z(a["w"].shape[0]) if a["want_params"] else None)
        if op == "bn_stats":
            return z(a["z"].shape[1]), torch.ones(a["z"].shape[1])
        if op in ("bn_silu", "silu", "silu_backward", "dropout_add"):
            first = a["z"] if op == "bn_silu" else a["x"]
            return torch.zeros_like(first) if a["out"] is None else a["out"]
        if op == "bn_silu_backward":
            c = a["z"].shape[1]
            return torch.zeros_like(a["z"]) if a["out"] is None else a["out"], z(c), z(c)
        if op == "attention_alibi_dropout":
            return z(a["q"].shape[0], a["heads"] * a["head_dim"], a["q"].shape[2])
        if op == "attention_alibi_dropout_backward":
            return torch.zeros_like(a["q"])
        return super().result(op, a)


def _walk(model, x, mp, grad):
    """The ops a call launches, forward and (after "--") backward, pack calls left out; and the full log."""
    rec = Recorder(model)
    for op in TRANSFORMER_STANDINS + NEW_OPS + DROPOUT_OPS:
        mp.setattr(ops, op, REAL[op])              # a stand-in reads the signature of what it replaces: the real op's
        mp.setattr(ops, op, rec.standin(op))
    rec.start()
    if grad:
        y = model(x.requires_grad_())
        rec.mark_backward()
        y.sum().backward()
    else:
        with torch.no_grad():
            model(x)
    log = [json.loads(e) for e in rec.log]
    return [("--" if op.startswith("--") else op) for op, _ in log if op not in PACKS], log


FF = ["layernorm_ct", "conv_forward", "silu", "conv_forward"]
FF_BWD = ["conv_bwd_weight", "conv_bwd_data", "silu_backward", "conv_bwd_weight", "conv_bwd_data", "layernorm_ct_backward"]
ATTN = ["layernorm_ct", "conv_forward", "attention_alibi", "conv_forward"]
ATTN_BWD = ["conv_bwd_weight", "conv_bwd_data", "attention_alibi_backward", "conv_bwd_weight", "conv_bwd_data", "layernorm_ct_backward"]
CONV_EVAL = ["layernorm_ct", "conv_forward", "glu_dwconv", "conv_forward"]
CONV_TRAIN = ["layernorm_ct", "conv_forward", "glu_dwconv", "bn_stats", "bn_silu", "conv_forward"]
CONV_BWD = ["conv_bwd_weight", "conv_bwd_data", "bn_silu_backward", "glu_dwconv_backward", "conv_bwd_weight", "conv_bwd_data",
            "layernorm_ct_backward"]


def test_eval_conv_block_is_four_launches(monkeypatch):
    conv = ConformerConvBlock(8).eval()
    names, log = _walk(conv, torch.zeros(2, 11, 8), monkeypatch, grad=False)
    assert names == CONV_EVAL
    fused = [a for op, a in log if op == "glu_dwconv"][0]
    assert fused["bn"] == ["net.4.weight", "net.4.bias", "net.4.running_mean", "net.4.running_var"] and fused["w"] == "net.3.weight"
    last = [a for op, a in log if op == "conv_forward"][-1]
    assert last["res"] is None and last["desc"][8] == 0               # forward(): no residual epilogue


def test_training_conv_block_walk(monkeypatch):
    conv = ConformerConvBlock(8, dropout=0.0).train()
    names, log = _walk(conv, torch.zeros(2, 11, 8), monkeypatch, grad=True)
    assert names == CONV_TRAIN + ["--"] + CONV_BWD
    stats = [a for op, a in log if op == "bn_stats"][0]
    assert (stats["running_mean"], stats["running_var"], stats["num_batches_tracked"], stats["momentum"]) == (
        "net.4.running_mean", "net.4.running_var", "net.4.num_batches_tracked", 0.1)
    assert [a for op, a in log if op == "glu_dwconv"][0]["bn"] is None
    back = [a for op, a in log if op == "bn_silu_backward"][0]
    assert back["training"] is True and back["out"] == back["dy"]    # dz over dy, in place
    # eval mode with a gradient: z is kept, the statistics are frozen, no statistics launch
    names, log = _walk(conv.eval(), torch.zeros(2, 11, 8), monkeypatch, grad=True)
    assert names == [op for op in CONV_TRAIN if op != "bn_stats"] + ["--"] + CONV_BWD
    assert [a for op, a in log if op == "bn_silu_backward"][0]["training"] is False


def test_block_launch_lists(monkeypatch):
    block = ConformerBlock(16, heads=2, dropout=0.0)
    names, _ = _walk(block.eval(), torch.zeros(2, 11, 16), monkeypatch, grad=False)
    assert names == FF + ATTN + CONV_EVAL + FF + ["layernorm_ct"] and len(names) == 17
    names, log = _walk(block.train(), torch.zeros(2, 11, 16), monkeypatch, grad=True)
    assert names == FF + ATTN + CONV_TRAIN + FF + ["layernorm_ct", "--", "layernorm_ct_backward"] + FF_BWD + CONV_BWD + ATTN_BWD + FF_BWD
    # the 0.5 is in the packed image: every residual add is a conv epilogue, nothing scales an activation
    res = [a["res"] is not None for op, a in log if op == "conv_forward"]
    assert res == [False, True, False, True, False, True, False, True]
    # dropout 0.1, the default: six more launches (19 + 6 ops; bn_stats is two launches: 26), one seed, seven distinct streams
    block = ConformerBlock(16, heads=2).train()
    torch.manual_seed(3)
    names, log = _walk(block, torch.zeros(2, 11, 16), monkeypatch, grad=False)
    assert len(names) == 25 and names.count("dropout_add") == 6 and names.count("attention_alibi_dropout") == 1
    sites = [(a["seed"], a["stream_id"]) for op, a in log if op in ("dropout_add", "attention_alibi_dropout")]
    assert len({seed for seed, _ in sites}) == 1 and sites[0][0] == block.last_dropout_seed
    assert sorted(stream for _, stream in sites) == [2, 3, 4, 5, 8, 14, 15]


def test_gelu_feed_forward_keeps_its_launches(monkeypatch):
    names, log = _walk(FeedForward(16, 32).eval(), torch.zeros(2, 11, 16), monkeypatch, grad=False)
    assert names == ["layernorm_ct", "conv_forward", "conv_forward"]
    assert [a["desc"][8] for op, a in log if op == "conv_forward"] == [8, 0]        # EPI_GELU_PRE, then no epilogue
