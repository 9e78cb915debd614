"""Generate ``g9_cross_attention.npz`` and ``meta_g9.json`` from the REFERENCE: the cross-attention branch of
networks/transformers.py (``Alibi(context_x, context_y)`` :24-77, ``Attention.forward(x, y)`` :157-191,
``Transformer(context_y=...)`` :241-279).  Same rules as ``make_goldens.py`` (build container only, CPU only; numeric
inputs / outputs and plain settings only; nothing from ``oracle/`` or the product package is imported).

The reference builds ``Alibi.M`` as (H, context_y, context_x) and crops it as ``M[:, :Tx, :Ty]``, so a call runs iff
``Tx <= context_y and Ty <= context_x``: with contexts (48, 32) the case (32, 48) below is that transposed reach.
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

KW = dict(dim=64, depth=1, heads=4, head_dim=16)
MODELS = {   # name: (context_x, context_y, seed, [(case, Tx, Ty)])
    "square50": (50, 50, 9, [("full", 50, 50), ("crop", 37, 41)]),
    "cx48_cy32": (48, 32, 10, [("t20_30", 20, 30), ("t30_20", 30, 20), ("t32_32", 32, 32), ("t32_48", 32, 48)]),
}


def main():
    _install_placeholders()
    sys.path.insert(0, REF)
    import transformers as ref_tf  # noqa: E402  (reference's networks/transformers.py)

    torch.set_num_threads(4)
    g, meta = {}, {"torch": torch.__version__, "generator": "tests/golden/make_goldens_cross.py", "kwargs": KW, "models": {}}
    for name, (cx, cy, seed, cases) in MODELS.items():
        torch.manual_seed(seed)
        tf = ref_tf.Transformer(KW["dim"], depth=KW["depth"], heads=KW["heads"], head_dim=KW["head_dim"], context_x=cx,
                                context_y=cy).eval()
        with torch.no_grad():    # LayerNorm affine away from identity so it is exercised (as G3)
            for p in tf.parameters():
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn_like(p))
        for k, v in tf.state_dict().items():
            g[f"{name}/sd/{k}"] = v.detach().numpy().astype(np.float32).copy()
        for case, tx, ty in cases:
            x, y = torch.randn(2, tx, KW["dim"]), torch.randn(2, ty, KW["dim"])
            with torch.no_grad():
                g[f"{name}/{case}/attn"] = tf.layers[0][0](x.clone(), y=y.clone()).numpy().copy()   # the attention sub-block
                g[f"{name}/{case}/out"] = tf(x.clone(), y=y.clone()).numpy().copy()                 # the block
            g[f"{name}/{case}/x"], g[f"{name}/{case}/y"] = x.numpy().copy(), y.numpy().copy()
        meta["models"][name] = {"context_x": cx, "context_y": cy, "seed": seed, "cases": [list(c) for c in cases]}
        meta["state_dict_keys"] = list(tf.state_dict().keys())
    g["alibi_cx32_cy48_h4"] = ref_tf.Alibi(32, 48, n_heads=4).M.numpy().astype(np.float32).copy()
    g["alibi_cx48_cy32_h4"] = ref_tf.Alibi(48, 32, n_heads=4).M.numpy().astype(np.float32).copy()
    assert all(v.dtype == np.float32 for v in g.values())
    np.savez_compressed(os.path.join(OUT, "g9_cross_attention.npz"), **g)
    with open(os.path.join(OUT, "meta_g9.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("g9_cross_attention.npz", os.path.getsize(os.path.join(OUT, "g9_cross_attention.npz")), len(g), "arrays")


if __name__ == "__main__":
    main()
