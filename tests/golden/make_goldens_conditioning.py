"""Generate ``g10_conditioning.npz`` and ``meta_g10.json`` from the REFERENCE: ``FiLM`` and ``SqueezeExcite`` of
networks/conditioning.py (:3-52).  Same rules as ``make_goldens.py`` (build container only, CPU only; numeric inputs /
outputs and plain settings only; nothing from ``oracle/`` or the product package is imported).  The reference module imports
with torch alone: its demo sits behind ``__main__``.
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
from make_goldens import OUT, REF  # noqa: E402

B, L = 3, 37
MODELS = {   # name: (class, args, kwargs, seed)
    "film": ("FiLM", (20, 24), {}, 11),
    "film_nobias": ("FiLM", (20, 24), {"bias": False}, 12),
    "se": ("SqueezeExcite", (24,), {}, 13),
}


def main():
    sys.path.insert(0, REF)
    import conditioning as ref  # noqa: E402  (reference's networks/conditioning.py)

    torch.set_num_threads(4)
    g, meta = {}, {"torch": torch.__version__, "generator": "tests/golden/make_goldens_conditioning.py", "batch": B, "length": L,
                   "models": {}}
    for name, (cls, args, kwargs, seed) in MODELS.items():
        torch.manual_seed(seed)
        model = getattr(ref, cls)(*args, **kwargs).eval()
        sd = model.state_dict()
        for k, v in sd.items():
            g[f"{name}/sd/{k}"] = v.detach().numpy().astype(np.float32).copy()
        dim = model.out_dim if cls == "FiLM" else model.dim
        x = torch.randn(B, L, dim)
        g[f"{name}/x"] = x.numpy().copy()
        with torch.no_grad():
            if cls == "FiLM":
                cond = torch.randn(B, model.dim)
                g[f"{name}/cond"] = cond.numpy().copy()
                g[f"{name}/out"] = model(x.clone(), cond.clone()).numpy().copy()
                assert model(x, None) is x
            else:
                g[f"{name}/out"] = model(x.clone()).numpy().copy()
        meta["models"][name] = {"class": cls, "args": list(args), "kwargs": kwargs, "seed": seed,
                                "state_dict": {k: list(v.shape) for k, v in sd.items()}}
    assert all(v.dtype == np.float32 for v in g.values())
    np.savez_compressed(os.path.join(OUT, "g10_conditioning.npz"), **g)
    with open(os.path.join(OUT, "meta_g10.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("g10_conditioning.npz", os.path.getsize(os.path.join(OUT, "g10_conditioning.npz")), len(g), "arrays")


if __name__ == "__main__":
    main()
