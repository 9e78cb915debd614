"""(no GPU) The two bf16x3 instruments of tests/b3_probe.py checked against a torch emulation of the six-term arithmetic:
the conditions under which tests/test_gpu_b3_products.py cannot pass vacuously.

* the palette splits into exactly the intended pieces under every scale and sign used;
* every probe case of the GPU file has at most one product per output, and one on every output past the halo;
  every tap and every 16-channel input chunk is hot for some row of every 32-row block;
* the full six-term emulation passes both instruments; each single-term omission, each term issued in place of another and
  an omission confined to 8 of 32 rows fail both."""
import itertools

import pytest
import torch

from tests import b3_probe as P

MUT = P.mutations()


# ------------------------------------------------------------------------------------------------ palette
def test_palette_splits_into_the_intended_pieces():
    for base, pieces in ((P.X_RICH, P.X_PIECES), (P.W_RICH, P.W_PIECES)):
        assert sum(pieces) == base
        for e, sign in itertools.product(range(-P.MAX_EXP, P.MAX_EXP + 1), (1.0, -1.0)):
            s = sign * 2.0 ** e
            v = torch.tensor([base * s], dtype=torch.float64).float()
            assert float(v.double()) == base * s                               # the scaled value is an exact fp32
            got = tuple(float(p) for p in P.split3(v))
            assert got == tuple(q * s for q in pieces), (base, s, got)


def test_palette_products_tell_the_six_terms_apart():
    prod = {(i, j): P.W_PIECES[i] * P.X_PIECES[j] for i in range(3) for j in range(3)}
    full = P.W_RICH * P.X_RICH
    six = sorted(prod[t] for t in P.TERMS)
    assert all(b > a for a, b in zip(six, six[1:]))                            # pairwise different magnitudes
    assert min(six) >= 2.0 ** -20 * full
    assert sum(prod[t] for t in P.DROPPED) < 2.0 ** -25 * full
    # the six-term sum is exact in fp32 in any order: every partial sum is a multiple of 2^-20 below 2
    assert float(torch.tensor(sum(six), dtype=torch.float64).float().double()) == sum(six)
    assert abs(sum(six) - full) / full < 0.05 * P.PROBE_BOUND
    # the smallest defect: a missing term, or one term issued in place of another
    gaps = [abs(a - b) for a in six for b in six if a != b]
    assert min(min(six), min(gaps)) / full >= 3.9 * P.PROBE_BOUND


def test_a_scaled_product_stays_exact_in_fp32():
    """|x| |w| up to 2^8 and down to 2^-8, and the residual block's second product on top (2^+-12): no overflow, no
    denormal, and the intermediate h of probe A splits exactly into three bf16 pieces again."""
    for ex, ew in itertools.product((-4, 0, 4), repeat=2):
        x = torch.tensor([P.X_RICH * 2.0 ** ex], dtype=torch.float64).float()
        w = torch.tensor([P.W_RICH * 2.0 ** ew], dtype=torch.float64).float()
        h = P.emulate(lambda a, b, bias=None: a * b, w, x)
        six = sum(P.W_PIECES[i] * P.X_PIECES[j] for i, j in P.TERMS) * 2.0 ** (ex + ew)
        assert float(h.double()) == six
        hp = P.split3(h)                                                       # asserts h + m + l == h bit for bit
        assert all(float(p) != 0 for p in hp)
        assert abs(float(h.double()) - P.W_RICH * P.X_RICH * 2.0 ** (ex + ew)) <= 0.05 * P.PROBE_BOUND * six


# ------------------------------------------------------------------------------------------------ the probe cases
def _check_1d(kind, cin, cout, k, s, d, batch, length):
    op = P.conv1d_op(kind, s, d)
    x = P.rich_activation((batch, cin, length), cin + length)
    hots = []
    for rot in range(P.ROTATIONS):
        w, h = P.probe_weight_1d(kind, cin, cout, k, s, rot)
        hots += h
        inner = P.interior(op, w, x, (s,) if kind == "convt" else (1,))
        assert bool(inner.any())
        P.assert_one_product(op, w, x, inner)
    P.assert_coverage(cout, cin, k, hots)


@pytest.mark.parametrize("row,lengths", P.RING, ids=P.RING_IDS)
def test_ring_probe_cases_have_one_product_per_output(row, lengths):
    _, kind, cin, cout, k, s = row
    batch, length = lengths[1]
    _check_1d(kind, cin, cout, k, s, 1, 1, min(length, 129))      # (the count does not depend on the batch)


def test_other_1d_probe_cases_have_one_product_per_output():
    kind, cin, cout, k, s, batch, length = P.MFMA_K9S3
    _check_1d(kind, cin, cout, k, s, 1, 1, length)
    for cout, (k, d) in itertools.product((32, 64, 128), ((3, 1), (7, 3))):       # the bf16x3 rows of the tile-variant tables
        _check_1d("causal", 16, cout, k, 1, d, 1, 200)
    _check_1d("convt", 32, 32, 4, 2, 1, 1, 50)                                    # two output phases (CPU only)


def test_causal_interior_starts_past_the_halo_of_k_minus_one_dilated_taps():
    x = torch.ones(1, 16, 40)
    w = torch.ones(32, 16, 7)
    inner = P.interior(P.conv1d_op("causal", 1, 3), w, x)
    assert not bool(inner[..., :18].any()) and bool(inner[..., 18:].all())


@pytest.mark.parametrize("c,k,d", [(c, 7, d) for c, d in P.RB_RING + [(64, 2)]] + [(c, 3, 1) for c in P.RB_TILE])
def test_resblock_probe_cases(c, k, d):
    batch, length = 1, 7 * d + 40
    for which in "AB":
        h1, h2 = [], []
        for rot in range(P.ROTATIONS):
            x, w1, w2, a, b = P.probe_resblock(c, k, d, batch, length, rot, which)
            h1 += a
            h2 += b
            assert bool((x[:, 1::2] == 0).all()) and bool((x[:, ::2] > 0).all())
            assert bool((w1[:, 1::2] == 0).all()) and float(w1.min()) >= 0 and float(w2.min()) >= 0
            op1, op2 = P.conv1d_op("causal", 1, d), P.conv1d_op("causal")
            P.assert_one_product(op1, w1, x, P.interior(op1, w1, torch.ones_like(x)))
            hmask = P.product_count(op1, w1, x)
            n = P.assert_one_product(op2, w2, hmask)
            assert bool((n[..., (k - 1) * d:] == 1).all())
        P.assert_coverage(c, c, k, h1)
        P.assert_coverage(c, c, 1, h2)
        # (the coverage above counts only the rows held to the probe's bound: the h rows an odd output reads at that
        # rotation, the odd rows of conv2)  every row of h ends on an odd output, once per turn of conv1's assignment
        assert all(bool((h1[2 * v][2] ^ h1[2 * v + 1][2]).all()) for v in range(P.ROTATIONS // 2))
        assert set(int(v) for c1, _, _ in h2 for v in c1[1::2]) == set(range(c))


@pytest.mark.parametrize("f,name", P.C2D_FWD, ids=[n for _, n in P.C2D_FWD])
def test_conv2d_forward_probe_cases(f, name):
    b, cin, cout, h, w_, kh, kw, sh, sw, ph, pw = f
    op = P.conv2d_op((sh, sw), (ph, pw))
    x = P.rich_activation((1, cin, min(h, 12), min(w_, 40)), cin)
    hots = []
    for rot in range(P.ROTATIONS):
        w, hh = P.probe_weight_2d(cin, cout, kh, kw, rot)
        hots += hh
        P.assert_one_product(op, w, x, P.interior(op, w, x))
    P.assert_coverage(cout, cin, kh * kw, hots)


@pytest.mark.parametrize("f,name", P.C2D_BWD, ids=[f"{n}-w{f[4]}" for f, n in P.C2D_BWD])
def test_conv2d_backward_data_probe_cases(f, name):
    b, cin, cout, h, w_, kh, kw, sh, sw, ph, pw = f        # (the count is checked on a crop of the map: it is local)
    f = (1, cin, cout, min(h, 12), min(w_, 40), kh, kw, sh, sw, ph, pw)
    op = P.conv2d_bwd_data_op((sh, sw), (ph, pw), (1, cin) + f[3:5])
    dy = P.rich_activation(P.out_shape_2d(f), cout)
    hots = []
    for rot in range(P.ROTATIONS):
        w, hh = P.probe_weight_2d_bwd(cin, cout, kh, kw, sh, sw, rot)
        hots += hh
        P.assert_one_product(op, w, dy, P.interior(op, w, dy, (sh, sw)))
    P.assert_coverage(cin, cout, kh * kw, hots)


# ------------------------------------------------------------------------------------------------ both instruments bite
def _probe_fails(y, want):
    worst, stray = P.probe_errors(y, want)
    return worst > 1.0 or stray > 0


def _projection_fails(y, want, terms, dim=1):
    w = P.worst_coefficients(P.projection(y, want, terms, dim))
    return any(not abs(w[t]) <= P.PROJ_BOUND for t in P.TERMS)


def _bites(op, a_probe, b_probe, a_dense, b_dense, bias, dim=1, form=None):
    """Both instruments on the emulation of ``op``: the six-term arithmetic passes, every mutation fails both.  ``form``: the
    (op, weight operand) the kernel contracts (b3_probe.kernel_form) where that is not the layer's own -- the references stay
    those of the layer."""
    want_p = op(a_probe.double(), b_probe.double())
    want_d = op(a_dense.double(), b_dense.double(), None if bias is None else bias.double())
    if form is not None:
        (op, a_probe), (_, a_dense) = form(a_probe), form(a_dense)
    terms = P.term_tensors(op, a_dense, b_dense)
    good_p, good_d = P.emulate(op, a_probe, b_probe), P.emulate(op, a_dense, b_dense, bias)
    assert P.assert_probe(good_p, want_p) < 0.05
    c = P.projection(good_d, want_d, terms, dim)
    P.assert_projection(c, "emulation")
    assert max(abs(v) for ij, v in P.worst_coefficients(c).items() if ij in P.TERMS) < 0.02
    for name, tl in MUT.items():
        assert _probe_fails(P.emulate(op, a_probe, b_probe, None, tl), want_p), name
        assert _projection_fails(P.emulate(op, a_dense, b_dense, bias, tl), want_d, terms, dim), name
    for t in P.TERMS:                                                          # the omission in 8 of every 32 rows only
        tl = tuple(u for u in P.TERMS if u != t)
        assert _probe_fails(P.in_rows(good_p, P.emulate(op, a_probe, b_probe, None, tl), 8, 16, dim), want_p), t
        bad = P.in_rows(good_d, P.emulate(op, a_dense, b_dense, bias, tl), 8, 16, dim)
        w = P.worst_coefficients(P.projection(bad, want_d, terms, dim))
        assert -0.4 < w[t] < -0.15, (t, w[t])                                  # -1/4: past the bound with room


@pytest.mark.parametrize("kind,cin,cout,k,s,d,length", [("causal", 32, 64, 5, 2, 1, 300), ("causal", 32, 32, 7, 1, 3, 150),
                                                        ("upconv", 64, 32, 5, 2, 1, 80), ("convt", 32, 32, 7, 1, 1, 150),
                                                        ("convt", 32, 32, 4, 2, 1, 80)])
def test_both_instruments_bite_on_1d_layers(kind, cin, cout, k, s, d, length):
    op = P.conv1d_op(kind, s, d)
    w, _ = P.probe_weight_1d(kind, cin, cout, k, s, 1)
    x, wd, bias = P.dense_layer_1d(kind, cin, cout, k, 2, length, 5)
    _bites(op, w, P.rich_activation((2, cin, length), 3), wd, x, bias, form=lambda a: P.kernel_form(kind, s, d, a))


def test_an_upsampling_layer_is_projected_on_its_folded_weights():
    """The polyphase form is the layer (float64, to rounding); its weights are sums of taps formed before the split, so a
    term lost by the kernel is a term of the FOLDED weights: on the pieces of the single taps it reads far from -1."""
    s, cin, cout = 4, 32, 32
    x, w, bias = P.dense_layer_1d("upconv", cin, cout, 9, 2, 60, 1)
    op = P.conv1d_op("upconv", s)
    want = op(w.double(), x.double(), bias.double())
    opk, wf = P.kernel_form("upconv", s, 1, w)
    assert wf.dtype == torch.float32 and wf.shape == (s, cout, cin, 3)
    assert torch.allclose(opk(P.upconv_fold(w.double(), s), x.double(), bias.double()), want, rtol=1e-12, atol=1e-13)
    bad = P.emulate(opk, wf, x, bias, tuple(t for t in P.TERMS if t != (1, 1)))
    folded = P.worst_coefficients(P.projection(bad, want, P.term_tensors(opk, wf, x)))
    single = P.worst_coefficients(P.projection(bad, want, P.term_tensors(op, w, x)))
    assert folded[(1, 1)] < -0.9 and abs(single[(1, 1)]) < 0.5, (folded[(1, 1)], single[(1, 1)])


def test_both_instruments_bite_on_conv2d_forward_and_backward_data():
    cin, cout = 32, 32
    gen = torch.Generator().manual_seed(2)
    wd = torch.randn(cout, cin, 4, 4, generator=gen) / (cin * 16) ** 0.5
    x = torch.randn(1, cin, 14, 40, generator=gen)
    op = P.conv2d_op((2, 2), (1, 1))
    w, _ = P.probe_weight_2d(cin, cout, 4, 4, 2)
    _bites(op, w, P.rich_activation((1, cin, 14, 40), 4), wd, x, torch.randn(cout, generator=gen) * 0.1)
    f = (1, cin, cout, 14, 40, 4, 4, 2, 2, 1, 1)
    op = P.conv2d_bwd_data_op((2, 2), (1, 1), (1, cin, 14, 40))
    w, _ = P.probe_weight_2d_bwd(cin, cout, 4, 4, 2, 2, 3)
    dy = torch.randn(P.out_shape_2d(f), generator=gen)
    _bites(op, w, P.rich_activation(P.out_shape_2d(f), 6), wd, dy, None)


def test_the_projection_bites_on_weight_gradients():
    gen = torch.Generator().manual_seed(8)
    for kind, cin, cout, k, s in (("causal", 32, 64, 5, 2), ("upconv", 32, 32, 5, 2), ("convt", 32, 32, 4, 2)):
        fwd = P.conv1d_op(kind, s, 1)
        shape = (cin, cout, k) if kind == "convt" else (cout, cin, k)
        op = P.wgrad_op(fwd, shape)
        rows = 1 if kind == "convt" else 0                                     # Cout: the kernel's output rows
        x = torch.randn(2, cin, 120, generator=gen)
        dy = torch.randn(fwd(torch.zeros(shape), x).shape, generator=gen)
        want, terms = op(dy.double(), x.double()), P.term_tensors(op, dy, x)
        good = P.emulate(op, dy, x)
        P.assert_projection(P.projection(good, want, terms, rows), f"emulated dW {kind}")
        for name, tl in MUT.items():
            assert _projection_fails(P.emulate(op, dy, x, None, tl), want, terms, rows), (kind, name)
        for t in P.TERMS:
            bad = P.in_rows(good, P.emulate(op, dy, x, None, tuple(u for u in P.TERMS if u != t)), 8, 16, rows)
            assert _projection_fails(bad, want, terms, rows), (kind, t)


@pytest.mark.parametrize("c,d", [(32, 3), (64, 1)])
def test_both_instruments_bite_on_the_residual_block(c, d):
    length = 160
    # probes: A guards conv1's terms, B conv2's; the odd output channels carry the single product
    for which in "AB":
        x, w1, w2, _, _ = P.probe_resblock(c, 7, d, 2, length, 1, which)
        want, h64 = P.resblock_ref(x, w1, None, w2, None, d)
        odd = lambda y: y[:, 1::2]
        assert bool((want[:, 1::2, 6 * d:] > 0).all())
        good = P.resblock_emulate(x, w1, None, w2, None, d)
        assert P.assert_probe(odd(good), odd(want)) < 0.05
        assert float((good.double() - want)[:, ::2].abs().max()) < 1e-5 * max(1.0, float(want.abs().max()))
        P.split3(P.emulate(P.conv1d_op("causal", 1, d), w1, x))                # probe A's h: three pieces, bit for bit
        for name, tl in MUT.items():
            kw = {"terms1": tl} if which == "A" else {"terms2": tl}
            assert _probe_fails(odd(P.resblock_emulate(x, w1, None, w2, None, d, **kw)), odd(want)), (which, name)
        for t in P.TERMS:                                                      # the omission in 8 of every 32 rows only
            tl = tuple(u for u in P.TERMS if u != t)
            kw = {"terms1": tl, "rows1": (8, 16)} if which == "A" else {"terms2": tl, "rows2": (8, 16)}
            assert _probe_fails(odd(P.resblock_emulate(x, w1, None, w2, None, d, **kw)), odd(want)), (which, t)
    # projection of conv1's terms through leaky' and conv2
    x, w1, b1, w2, b2 = P.dense_resblock(c, 7, d, 2, length, 9)
    want, h64 = P.resblock_ref(x, w1, b1, w2, b2, d)
    terms = P.resblock_conv1_terms(x, w1, w2, h64, d)
    P.assert_projection(P.projection(P.resblock_emulate(x, w1, b1, w2, b2, d), want, terms), "emulated block")
    for name, tl in MUT.items():
        assert _projection_fails(P.resblock_emulate(x, w1, b1, w2, b2, d, terms1=tl), want, terms), name
    for t in P.TERMS:                               # lost in 8 of every 32 rows of h: conv2 spreads it over all outputs, -1/4
        tl = tuple(u for u in P.TERMS if u != t)
        w = P.worst_coefficients(P.projection(P.resblock_emulate(x, w1, b1, w2, b2, d, terms1=tl, rows1=(8, 16)), want, terms))
        assert -0.45 < w[t] < -0.12, (t, w[t])
