"""Generate ``g11_snake.npz`` and ``meta_g11.json`` from the REFERENCE: ``Snek`` and ``SnekReLU`` of networks/utils.py
(:44-105), ``dim`` 1 and 2, with their alphas moved off the initial ones, and ``x.grad`` / ``alphas.grad`` from the reference's
own autograd under a seeded incoming gradient.  Same rules as ``make_goldens.py`` (build container only, CPU only; numeric
inputs / outputs and plain settings only; nothing from ``oracle/`` or the product package is imported).  The reference module
imports under the placeholders of ``make_goldens._install_placeholders``.
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

MODELS = {   # name: (class, in_channels, dim, x shape, seed)
    "snek1": ("Snek", 5, 1, (3, 5, 37), 21),
    "snek2": ("Snek", 5, 2, (2, 5, 3, 7), 22),
    "snekrelu1": ("SnekReLU", 5, 1, (3, 5, 37), 23),
    "snekrelu2": ("SnekReLU", 5, 2, (2, 5, 3, 7), 24),
    "snek1_shared": ("Snek", 1, 1, (3, 5, 37), 25),          # one alpha broadcast over five channels
}


def main():
    _install_placeholders()
    sys.path.insert(0, REF)
    import utils as ref  # noqa: E402  (reference's networks/utils.py)

    torch.set_num_threads(4)
    g, meta = {}, {"torch": torch.__version__, "generator": "tests/golden/make_goldens_snake.py", "eps": 1e-6, "models": {}}
    for name, (cls, channels, dim, shape, seed) in MODELS.items():
        torch.manual_seed(seed)
        model = getattr(ref, cls)(channels, dim=dim)
        init = model.alphas.detach().clone()
        with torch.no_grad():
            model.alphas.copy_(0.25 + 2.0 * torch.rand_like(model.alphas))
            if channels > 1:
                model.alphas.view(-1)[1] = -1.5          # a negative alpha
        x = (2.0 * torch.randn(shape)).requires_grad_(True)
        with torch.no_grad():
            x.view(-1)[:4] = torch.tensor([0.0, -0.0, 1.0, -1.0])       # the zero point of the clamp, both signs
        dout = torch.randn(shape)
        out = model(x)
        out.backward(dout)
        sd = model.state_dict()
        for k, v in sd.items():
            g[f"{name}/sd/{k}"] = v.detach().numpy().astype(np.float32).copy()
        g[f"{name}/x"] = x.detach().numpy().copy()
        g[f"{name}/dout"] = dout.numpy().copy()
        g[f"{name}/out"] = out.detach().numpy().copy()
        g[f"{name}/dx"] = x.grad.numpy().copy()
        g[f"{name}/dalphas"] = model.alphas.grad.numpy().copy()
        meta["models"][name] = {"class": cls, "in_channels": channels, "dim": dim, "seed": seed, "x_shape": list(shape),
                                "state_dict": {k: list(v.shape) for k, v in sd.items()},
                                "parameters": [n for n, _ in model.named_parameters()],
                                "initial_alphas": sorted(set(init.reshape(-1).tolist()))}
    assert all(v.dtype == np.float32 for v in g.values())
    np.savez_compressed(os.path.join(OUT, "g11_snake.npz"), **g)
    with open(os.path.join(OUT, "meta_g11.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("g11_snake.npz", os.path.getsize(os.path.join(OUT, "g11_snake.npz")), len(g), "arrays")


if __name__ == "__main__":
    main()
