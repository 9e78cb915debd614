"""Float64 restatement of ``FiLM`` and ``SqueezeExcite`` (networks/conditioning.py), written from the formulas:

    FiLM:           out[b, l, c] = x[b, l, c] * gamma[b, c] + beta[b, c],   gamma = cond Wg^T + bg,  beta = cond Wb^T + bb (or 0)
    SqueezeExcite:  out[b, l, :] = x[b, l, :] * sigmoid(W2 relu(W1 x[b, l, :] + b1) + b2)

Everything is plain torch arithmetic in the dtype of the operands, so the same functions give the float64 checker (``f64``
the operands first) and, on float32 operands, the fp32 CPU evaluation whose distance from the checker is fp32's own noise.
Gradients come from autograd on these functions.  Layout: the reference's, (B, L, dim); ``bct`` transposes for the
channel-major entry points.  ``tests/test_conditioning_cpu.py`` pins both functions to the goldens of the reference.
"""
import torch

U = 2.0 ** -24          # unit roundoff of fp32


def f64(*tensors):
    out = tuple(None if t is None else torch.as_tensor(t).detach().double() for t in tensors)
    return out[0] if len(out) == 1 else out


def bct(x):
    """(B, L, C) <-> (B, C, L)."""
    return x.transpose(1, 2).contiguous()


def film_gb(cond, wg, bg, wb=None, bb=None):
    """(B, C) gamma and (B, C) beta or None."""
    gamma = cond @ wg.T + bg
    beta = None if wb is None else cond @ wb.T + bb
    return gamma, beta


def film(x, cond, wg, bg, wb=None, bb=None):
    """x (B, L, C), cond (B, D), wg / wb (C, D), bg / bb (C,)."""
    gamma, beta = film_gb(cond, wg, bg, wb, bb)
    out = x * gamma[:, None, :]
    return out if beta is None else out + beta[:, None, :]


def sigmoid(z):
    return 1.0 / (1.0 + torch.exp(-z))


def squeeze_excite(x, w1, b1, w2, b2):
    """x (B, L, C), w1 (Hd, C), b1 (Hd,), w2 (C, Hd), b2 (C,)."""
    hidden = torch.clamp(x @ w1.T + b1, min=0.0)
    z = hidden @ w2.T + b2
    return x * sigmoid(z)


def gate(x, z):
    return x * sigmoid(z)


def with_grads(fn, operands, dout):
    """(out, [gradient of every operand or None]) of ``fn(*operands)`` under the incoming gradient ``dout``, in the operands' dtype."""
    leaves = [None if t is None else t.detach().clone().requires_grad_(True) for t in operands]
    out = fn(*leaves)
    out.backward(dout.to(out.dtype))
    return out.detach(), [None if t is None else t.grad for t in leaves]
