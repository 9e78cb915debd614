"""Generate ``g12_conformer.npz`` and ``meta_g12.json`` from the REFERENCE: ``ConformerConvBlock`` and ``ConformerBlock`` of
networks/transformers.py (:281-368), in training and in eval mode with dropout 0, with ``x.grad`` and every parameter gradient
from the reference's own autograd under a seeded incoming gradient, and the running statistics after the step.  Same rules as
``make_goldens.py`` (build container only, CPU only; numeric inputs / outputs and plain settings only; nothing from ``oracle/``
or the product package is imported).

The reference's two classes cannot be constructed or run as they stand.  They run here under three stubs and
nothing else -- every layer, initialisation and line of arithmetic is the reference's own:

1. a class attribute ``ConformerConvBlock.out_channels`` (= in_channels: the conv is depthwise), which ``__init__`` reads at
   :323-324 and never sets;
2. a subclass of the reference ``Attention`` that swallows the ``activation`` keyword ``ConformerBlock.__init__`` passes (:353);
3. a ``ConformerConvBlock.forward`` that applies the reference's own ``net[0]`` (the LayerNorm over channels) before the
   rearrangement to (b, d, n) and ``net[1:]`` after it.
"""
from __future__ import annotations

import json
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_goldens import OUT, REF, _install_placeholders  # noqa: E402

B, T = 3, 11
MODELS = {   # name: (class, constructor kwargs, seed)
    "conv_k17": ("ConformerConvBlock", dict(in_channels=8, kernel_size=17, dropout=0.0), 31),
    "conv_k4": ("ConformerConvBlock", dict(in_channels=8, kernel_size=4, dropout=0.0), 32),
    "block": ("ConformerBlock", dict(dim=16, heads=2, dropout=0.0), 33),
}


def _stub(ref_tf):
    from einops import rearrange

    class Attention(ref_tf.Attention):
        def __init__(self, *args, activation=None, **kwargs):
            super().__init__(*args, **kwargs)

    def forward(self, x):
        x = self.net[0](x)
        x = rearrange(x, "b n d -> b d n")
        x = self.net[1:](x)
        return rearrange(x, "b d n -> b n d")

    ref_tf.Attention = Attention
    ref_tf.ConformerConvBlock.forward = forward


def _build(ref_tf, cls, kwargs):
    channels = kwargs.get("in_channels", kwargs.get("dim"))
    ref_tf.ConformerConvBlock.out_channels = channels
    return getattr(ref_tf, cls)(**kwargs)


def main():
    _install_placeholders()
    sys.path.insert(0, REF)
    import transformers as ref_tf  # noqa: E402  (reference's networks/transformers.py)

    _stub(ref_tf)
    torch.set_num_threads(4)
    g, meta = {}, {"torch": torch.__version__, "generator": "tests/golden/make_goldens_conformer.py", "batch": B, "frames": T,
                   "models": {}}
    for name, (cls, kwargs, seed) in MODELS.items():
        torch.manual_seed(seed)
        model = _build(ref_tf, cls, kwargs)
        with torch.no_grad():      # every parameter and running statistic away from its initial value
            for p in model.parameters():
                p.add_(0.1 * torch.randn_like(p))
            for n, buf in model.named_buffers():
                if n.endswith("running_mean"):
                    buf.copy_(0.2 * torch.randn_like(buf))
                if n.endswith("running_var"):
                    buf.copy_(0.5 + torch.rand_like(buf))
        sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
        width = kwargs.get("in_channels", kwargs.get("dim"))
        x0, dout = torch.randn(B, T, width), torch.randn(B, T, width)
        for k, v in sd0.items():
            g[f"{name}/sd/{k}"] = v.numpy().copy()
        g[f"{name}/x"], g[f"{name}/dout"] = x0.numpy().copy(), dout.numpy().copy()
        for mode in ("train", "eval"):
            model.load_state_dict(sd0)
            model.train(mode == "train")
            model.zero_grad()
            x = x0.clone().requires_grad_(True)
            out = model(x)
            out.backward(dout)
            g[f"{name}/{mode}/out"] = out.detach().numpy().copy()
            g[f"{name}/{mode}/dx"] = x.grad.numpy().copy()
            for n, p in model.named_parameters():
                g[f"{name}/{mode}/grad/{n}"] = p.grad.numpy().copy()
            for n, buf in model.named_buffers():
                if "running_" in n or n.endswith("num_batches_tracked"):
                    g[f"{name}/{mode}/after/{n}"] = buf.detach().numpy().copy()
        meta["models"][name] = {"class": cls, "kwargs": kwargs, "seed": seed,
                                "state_dict": {k: list(v.shape) for k, v in sd0.items()},
                                "parameters": [n for n, _ in model.named_parameters()]}
    assert all(v.dtype in (np.float32, np.int64) for v in g.values()), {k: v.dtype for k, v in g.items() if v.dtype != np.float32}
    np.savez_compressed(os.path.join(OUT, "g12_conformer.npz"), **g)
    with open(os.path.join(OUT, "meta_g12.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("g12_conformer.npz", os.path.getsize(os.path.join(OUT, "g12_conformer.npz")), len(g), "arrays")


if __name__ == "__main__":
    main()
