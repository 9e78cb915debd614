"""CPU statement of the quantiser's staged training call ("quantiser dropout"): a stage count per batch row.

``q_b = clamp(stages[b], 0, q_used)``; stage q of frame (b, t) is live when ``q < q_b``.  The search is greedy, so row b of a
staged call is row b quantised alone with ``codebook_n = q_b``:

* ``forward``: row by row through ``oracle.rvq.residual_quantize(x[b:b+1], cbs, q_b, sizes=)`` -- index -1 and x_q exact 0 where
  nothing is live, sq_err in float64 over the live frames of each stage, commit = sum(sq_err) / (B T D);
* ``definition``: the float64 autograd definition of tests/test_gpu_rvq_backward.py (the fp32 residual chain carried
  straight-through) with a live mask -- a dead stage subtracts nothing AND leaves the loss, which is not what an index of -1
  does there -- and its derived bound ``2 (m + 2) 2^-24 sum|addends|`` over the addends of live stages only;
* ``ema_stats``: the assignment statistics of the EMA update on a masked index (a dead stage counts and subtracts nothing).
"""
import torch

from oracle import rvq

U = 2.0 ** -24


def taken(stages, batch, q_used):
    """The stage counts the kernels use: clamp(stages[b], 0, q_used); None is q_used everywhere."""
    if stages is None:
        return [int(q_used)] * batch
    got = [max(0, min(int(s), int(q_used))) for s in stages]
    assert len(got) == batch
    return got


def live_mask(stages, batch, q_used):
    """(B, q_used) bool: stage q of row b is live."""
    q_b = torch.tensor(taken(stages, batch, q_used), dtype=torch.int64)
    return torch.arange(q_used).unsqueeze(0) < q_b.unsqueeze(1)


def forward(x, cbs, stages, q_used=None, sizes=None):
    """x (B, T, D) f32, cbs (n_q, K, D) f32 -> (x_q (B, T, D) f32, index (B, T, q_used) int64, sq_err (q_used) f64, commit f64)."""
    b, t, d = x.shape
    q_used = cbs.shape[0] if q_used is None else int(q_used)
    xq = torch.zeros(b, t, d, dtype=torch.float32)
    index = torch.full((b, t, q_used), -1, dtype=torch.int64)
    sq_err = torch.zeros(q_used, dtype=torch.float64)
    for row, q_b in enumerate(taken(stages, b, q_used)):
        xq_row, idx_row, _ = rvq.residual_quantize(x[row:row + 1], cbs, q_b, sizes=sizes)
        xq[row], index[row, :, :q_b] = xq_row[0], idx_row[0]
        r = x[row].float().clone()
        for q in range(q_b):
            r = r - cbs[q][idx_row[0, :, q]]                  # the search's own fp32 residual
            sq_err[q] += float((r.double() ** 2).sum())
    return xq, index, sq_err, float(sq_err.sum()) / (b * t * d)


def definition(x, cbs, idx, stages, g_xq, g_l):
    """x (B, T, D), cbs (n_q, K, D), idx (B, T, q_used) (only its live entries are read), stages (B,) or None, g_xq (B, T, D) or
    None, g_l float -- all on the CPU.  Returns float64 (dx, dC, bound_dx, bound_dC, chosen (n_q, K) bool, L): autograd of
    sum(g_xq * x_q) + g_l * L  with the straight-through x_q over the live stages and
    L = sum_q sum over the frames live at q of r_{q+1}^2 / (B T D)."""
    b, t, d = x.shape
    n_q, k, _ = cbs.shape
    q_used, n = idx.shape[-1], b * t
    live = live_mask(stages, b, q_used)                         # (B, q_used)
    x64 = x.double().requires_grad_(True)
    c64 = cbs.double().requires_grad_(True)
    g64 = torch.zeros(b, t, d, dtype=torch.float64) if g_xq is None else g_xq.double()
    r, sel, loss, res, valid = x64, torch.zeros_like(x64), x64.new_zeros(()), [], []
    r32 = x.float().clone()
    for q in range(q_used):
        ok = (idx[..., q] >= 0) & (idx[..., q] < k) & live[:, q].unsqueeze(1)          # (B, T): a codeword is subtracted
        on = live[:, q].view(b, 1, 1).double()                                         # the stage runs for this row
        c = c64[q][idx[..., q].clamp(0, k - 1)] * ok.unsqueeze(-1)
        r, sel = r - c, sel + c
        r32 = r32 - c.detach().float()                        # the definition's r_{q+1} = fl32(r_q - c), straight-through
        r = r + (r32.double() - r).detach()
        loss = loss + ((r ** 2) * on).sum() / (n * d)
        res.append(r.detach().abs() * on)
        valid.append(ok)
    xq = x64 + (sel - x64).detach()
    ((xq * g64).sum() + g_l * loss + 0.0 * c64.sum()).backward()
    a = abs(2.0 * g_l / (n * d))
    suffix = [None] * q_used                                  # sum over the live q' >= q of |r_{q'+1}|
    for q in range(q_used - 1, -1, -1):
        suffix[q] = res[q] + (suffix[q + 1] if q + 1 < q_used else 0.0)
    bound_dx = 2 * (q_used + 2) * U * (g64.abs() + a * (suffix[0] if q_used else 0.0))
    bound_dc = torch.zeros(n_q, k, d, dtype=torch.float64)
    chosen = torch.zeros(n_q, k, dtype=torch.bool)
    for q in range(q_used):
        flat = idx[..., q].reshape(-1)[valid[q].reshape(-1)]
        rows = suffix[q].reshape(n, d)[valid[q].reshape(-1)]
        counts = torch.bincount(flat, minlength=k).double()
        mags = torch.zeros(k, d, dtype=torch.float64).index_add_(0, flat, rows)
        bound_dc[q] = 2 * (counts.unsqueeze(1) * q_used + 2) * U * a * mags
        chosen[q] = counts > 0
    return x64.grad, c64.grad, bound_dx, bound_dc, chosen, float(loss.detach())


def ema_stats(frames, cbs, index):
    """``oracle.rvq.ema_assignment_stats`` on a masked index: frames (N, D), cbs (Q, K, D) before the update, index (N, q_used)
    with -1 at dead stages -> stats (q_used, K, D + 1); a dead stage neither counts nor subtracts."""
    n, d = frames.shape
    q_used, k = index.shape[1], cbs.shape[1]
    stats = torch.zeros(q_used, k, d + 1, dtype=frames.dtype)
    residual = frames.clone()
    for q in range(q_used):
        idx = index[:, q]
        ok = idx >= 0
        stats[q, :, 0] = torch.bincount(idx[ok], minlength=k).to(frames.dtype)
        stats[q, :, 1:].index_add_(0, idx[ok], residual[ok])
        residual = residual - cbs[q][idx.clamp_min(0)] * ok.unsqueeze(1)
    return stats
