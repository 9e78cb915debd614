"""Memory contract of the ops of ``csrc/conformer.hip`` on the guarded, poisoned arena of ``tests/guarded.py``: every operand
sits between guard bands, and every byte the ops do not own holds 0x00, 0xFF or 0x7F in turn.  Guards must stay intact, every
element of every output and of every workspace must be written (a poisoned one misses the reference), inputs must come back
untouched, the running statistics and the counter are updated in place, and the results must be bitwise the same on every
pattern and on both clean runs.  The in-place forms (``y`` over ``z``, ``dz`` over ``dy``, SiLU over its operand) are included.
Every op is given exact operands -- z, the statistics and dz are placed, not taken from the op before -- so the tolerances are
the derived bounds of tests/conformer_ref.py at their largest element, times 2.  The bad-shape returns of the C entry points
follow: nothing is launched, so nothing may be written."""
import ctypes

import pytest
import torch

from audio_generation_amd import _lib, ops
from tests import conformer_ref as ref
from tests.guarded import Out, routed, run_contract

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
SHAPES = [(2, 5, 37, 17), (1, 3, ref.SEGMENT + 1, 4), (3, 130, 3, 31)]       # (B, C, T, K)


def _tol(*bounds):
    return 2.0 * max(float(b.max()) for b in bounds) + 1e-30


def _payload(alloc):
    return alloc.raw[alloc.lead:alloc.lead + alloc.nbytes].view(torch.float32)


def _only(v, lo, hi):
    """v with everything outside [lo, hi) of the time axis zeroed: the share of a tile or segment in a sum over t."""
    out = torch.zeros_like(v)
    out[..., lo:hi] = v[..., lo:hi]
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conformer_ops_memory_contract(shape):
    b, c, t, k = shape
    n, rows = b * t, b * c
    segs, tiles = -(-t // ref.SEGMENT), -(-t // ref.TILE)
    gen = torch.Generator().manual_seed(sum(shape))
    r = lambda *s: torch.randn(*s, generator=gen)
    u, w, bias, gamma, beta, dy = 2.0 * r(b, 2 * c, t), r(c, 1, k) / k ** 0.5, r(c), 1.0 + 0.3 * r(c), 0.3 * r(c), r(b, c, t)
    r_mean, r_var = 0.2 * r(c), 0.5 + torch.rand(c, generator=gen)
    u[0, 0, 0], u[0, c, t - 1] = 0.0, -0.0
    count = torch.tensor(7, dtype=torch.int64)
    x, dout = 3.0 * r(rows * t), r(rows * t)
    u64, w64, bias64, gamma64, beta64, dy64, rm64, rv64, x64, dout64 = ref.f64(u, w, bias, gamma, beta, dy, r_mean, r_var, x, dout)
    z = ref.glu_dwconv(u64, w64, bias64).float()              # the z, mean and var the later ops are given
    mean, var = (v.float() for v in ref.batch_stats(z.double())[:2])
    z64, mean64, var64 = ref.f64(z, mean, var)
    bn_run, bn_batch = (gamma64, beta64, rm64, rv64, EPS), (gamma64, beta64, mean64, var64, EPS)

    want, tol = {}, {}
    want["z"], tol["z"] = ref.glu_dwconv(u64, w64, bias64), _tol(ref.bound_z(u64, w64, bias64))
    scale = ref.bn_parts(want["z"], *bn_run)["scale"].abs().reshape(1, -1, 1)
    want["y_fused"] = ref.bn_silu(want["z"], *bn_run)         # |dy / dz| <= 1.1 |scale| carries the error of z
    tol["y_fused"] = _tol(ref.bound_y(want["z"], *bn_run, False) + 1.1 * scale * ref.bound_z(u64, w64, bias64))
    m64, v64, m2 = ref.batch_stats(z64)
    d_mean, d_var = ref.bound_stats(z64)
    want["mean"], want["var"], tol["mean"], tol["var"] = m64, v64, _tol(d_mean), _tol(d_var)
    want["running_mean"], want["running_var"] = ref.running_update(rm64, rv64, m64, m2, n)
    tol["running_mean"], tol["running_var"] = (_tol(v) for v in ref.bound_running(z64, rm64, rv64))
    seg = lambda v, s: v.reshape(rows, t)[:, s * ref.SEGMENT:(s + 1) * ref.SEGMENT]
    seg_mean = torch.stack([seg(z64, s).mean(1) for s in range(segs)], 1)
    seg_m2 = torch.stack([(seg(z64, s) - seg_mean[:, s:s + 1]).square().sum(1) for s in range(segs)], 1)
    want["stats_ws"], tol["stats_ws"] = torch.stack([seg_mean, seg_m2], 2), max(_tol(d_mean), n * _tol(d_var))
    want["y_eval"], tol["y_eval"] = ref.bn_silu(z64, *bn_run), _tol(ref.bound_y(z64, *bn_run, False))
    want["y"], tol["y"] = ref.bn_silu(z64, *bn_batch), _tol(ref.bound_y(z64, *bn_batch, True))
    for mode, bn, training in (("", bn_batch, True), ("_eval", bn_run, False)):
        got3, bound3 = ref.bn_silu_backward(dy64, z64, *bn, training), ref.bound_bn_backward(dy64, z64, *bn, training)
        for name, g, d in zip(("dz", "dgamma", "dbeta"), got3, bound3):
            want[name + mode], tol[name + mode] = g, _tol(d)
        p = ref.bn_parts(z64, *bn[:4], EPS)
        da = dy64 * ref.silu_grad(p["a"])
        parts = torch.stack([torch.stack([seg(da, s).sum(1), seg(da * p["zhat"], s).sum(1)], 1) for s in range(segs)], 1)
        want["bwd_ws" + mode] = torch.cat([parts.reshape(-1), torch.stack([got3[2], got3[1]], 1).reshape(-1)])
        tol["bwd_ws" + mode] = _tol(bound3[1], bound3[2])      # a partial is part of its channel's sum
    want["du"], want["dw"], want["dbias"] = ref.glu_dwconv_backward(dy64, u64, w64)
    tol["du"], tol["dw"], tol["dbias"] = (_tol(v) for v in ref.bound_conv_backward(dy64, u64, w64))
    share = lambda i, s: ref.glu_dwconv_backward(_only(dy64[i:i + 1], s * ref.TILE, (s + 1) * ref.TILE), u64[i:i + 1], w64)[1:]
    want["conv_ws"] = torch.stack([torch.stack([torch.cat([share(i, s)[0], share(i, s)[1].unsqueeze(1)], 1) for s in range(tiles)], 1)
                                   for i in range(b)]).reshape(-1)                  # (B, C, tiles, K + 1)
    tol["conv_ws"] = max(tol["dw"], tol["dbias"])
    want["silu"], tol["silu"] = ref.silu(x64), _tol(ref.bound_silu(x64))
    want["silu_dx"] = dout64 * ref.silu_grad(x64)
    tol["silu_dx"] = _tol(dout64.abs() * ref.bound_silu_grad(x64) + ref.U * want["silu_dx"].abs())

    def run(arena):
        ud, wd, bd, gd, btd, dyd, rmd, rvd, zd, md, vd, xd, dd = (
            arena.place(v) for v in (u, w, bias, gamma, beta, dy, r_mean, r_var, z, mean, var, x, dout))
        rm_io, rv_io, cnt, zi, dyi, dyi_eval, xi, di = (arena.place(v) for v in (r_mean, r_var, count, z, dy, dy, x, dout))
        run_args, batch_args = (gd, btd, rmd, rvd, EPS), (gd, btd, md, vd, EPS)
        first = len(arena.allocs)
        with routed(arena, ops):
            z_out = ops.glu_dwconv(ud, wd, bd)
            y_fused = ops.glu_dwconv(ud, wd, bd, bn=(gd, btd, rmd, rvd), eps=EPS)
            mean_out, var_out = ops.bn_stats(zd, rm_io, rv_io, cnt, 0.1)
            y_eval = ops.bn_silu(zd, *run_args, training=False)
            y = ops.bn_silu(zd, *batch_args, training=True)
            ops.bn_silu(zi, *batch_args, training=True, out=zi)
            dz, dgamma, dbeta = ops.bn_silu_backward(dyd, zd, *batch_args, training=True)
            dz_eval, dgamma_eval, dbeta_eval = ops.bn_silu_backward(dyd, zd, *run_args, training=False)
            ops.bn_silu_backward(dyi, zd, *batch_args, training=True, want_params=False, out=dyi)
            ops.bn_silu_backward(dyi_eval, zd, *run_args, training=False, want_params=False, out=dyi_eval)
            du, dw, dbias = ops.glu_dwconv_backward(dyd, ud, wd)
            du_only, _, _ = ops.glu_dwconv_backward(dyd, ud, wd, want_params=False)
            silu = ops.silu(xd)
            ops.silu(xi, out=xi)
            silu_dx = ops.silu_backward(xd, dd)
            ops.silu_backward(xd, di, out=di)
        made = arena.allocs[first:]
        f, vec, bwd_ws = 4 * rows * t, 4 * c, 8 * rows * segs + 8 * c
        assert [(a.dtype, a.nbytes) for a in made] == [
            (torch.float32, f), (torch.float32, f),                                                         # z, y_fused
            (torch.float32, vec), (torch.float32, vec), (torch.uint8, 8 * rows * segs),                      # mean, var, workspace
            (torch.float32, f), (torch.float32, f),                                                         # y_eval, y
            (torch.float32, f), (torch.float32, vec), (torch.float32, vec), (torch.uint8, bwd_ws),           # dz, dgamma, dbeta
            (torch.float32, f), (torch.float32, vec), (torch.float32, vec), (torch.uint8, bwd_ws),           # the same, eval
            (torch.uint8, bwd_ws), (torch.uint8, bwd_ws),                                                   # in place: workspaces only
            (torch.float32, 2 * f), (torch.float32, 4 * c * k), (torch.float32, vec), (torch.uint8, 4 * rows * tiles * (k + 1)),
            (torch.float32, 2 * f),                                                                         # du alone: no workspace
            (torch.float32, f), (torch.float32, f)], made                                                   # silu, its dx
        outs = dict(z=z_out, y_fused=y_fused, mean=mean_out, var=var_out, running_mean=rm_io, running_var=rv_io,
                    stats_ws=_payload(made[4]).reshape(rows, segs, 2), y_eval=y_eval, y=y, dz=dz, dgamma=dgamma, dbeta=dbeta,
                    bwd_ws=_payload(made[10]), dz_eval=dz_eval, dgamma_eval=dgamma_eval, dbeta_eval=dbeta_eval,
                    bwd_ws_eval=_payload(made[14]), du=du, dw=dw.reshape(c, k), dbias=dbias, conv_ws=_payload(made[20]), silu=silu,
                    silu_dx=silu_dx)
        aliases = dict(y_inplace=(zi, "y"), dz_inplace=(dyi, "dz"), dz_eval_inplace=(dyi_eval, "dz_eval"), bwd_ws_inplace=(_payload(made[15]), "bwd_ws"),
                       bwd_ws_eval_inplace=(_payload(made[16]), "bwd_ws_eval"), du_only=(du_only, "du"), silu_inplace=(xi, "silu"),
                       silu_dx_inplace=(di, "silu_dx"))
        untouched = dict(u=(ud, u), w=(wd, w), bias=(bd, bias), gamma=(gd, gamma), beta=(btd, beta), dy=(dyd, dy), r_mean=(rmd, r_mean),
                         r_var=(rvd, r_var), z_in=(zd, z), mean_in=(md, mean), var_in=(vd, var), x=(xd, x), dout=(dd, dout))
        return ([Out(name, got, want[name], tol[name]) for name, got in outs.items()]
                + [Out(name, got, want[of], tol[of]) for name, (got, of) in aliases.items()]
                + [Out(name, got, src, exact=True) for name, (got, src) in untouched.items()]
                + [Out("count", cnt, count + 1, exact=True)])
    report = run_contract(run, DEV)
    assert report["reproducible"], report["irreproducible"]


def test_bad_shapes_return_before_a_launch():
    lib = _lib.load()
    bad = -1
    buf = torch.zeros(64, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    big = 2 ** 20
    for b, c, t, k in ((0, 2, 8, 3), (1, 0, 8, 3), (1, 2, -8, 3), (1, 2, 8, 0), (1, 2, 8, ops.CONFORMER_MAX_K + 1), (big, big, 1, 3),
                       (big, 4096, ref.TILE + 1, 3)):
        assert lib.agx_glu_dwconv_forward(p, p, p, None, None, None, None, EPS, p, b, c, t, k, None) == bad
        assert lib.agx_glu_dwconv_backward(p, p, p, p, p, p, p, 256, b, c, t, k, None) == bad
        if k == 3:
            assert lib.agx_bn_stats(p, p, p, p, p, None, 0.1, p, 256, b, c, t, None) == bad
            assert lib.agx_bn_silu_forward(p, p, p, p, p, EPS, 1, p, b, c, t, None) == bad
            assert lib.agx_bn_silu_backward(p, p, p, p, p, p, EPS, 1, p, p, p, p, 256, b, c, t, None) == bad
    assert lib.agx_bn_stats(p, p, p, p, p, None, 0.1, p, 256, 1, 2, 1, None) == bad           # B T == 1
    torch.cuda.synchronize()
    assert not buf.any(), "a refused call wrote"
