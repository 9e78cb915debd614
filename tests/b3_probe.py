"""Two instruments that tell whether a bf16x3 kernel issues all six of its piece products.

The arithmetic splits each fp32 operand into three bf16 pieces h + m + l and sums six of the nine piece products
(m.m  h.l  l.h  h.m  m.h  h.h, small terms first); m.l, l.m and l.l are dropped by design.  A dense random test at
1e-5 of the output scale cannot see one of the three small products go missing.  These can:

* **Exact piece-product probe.**  Weights with ONE non-zero (input channel, tap) per output row (per output phase of a
  transposed layer, per parity class of a strided backward-data), dense activations, every value ``+-2^e`` times a palette
  constant whose three pieces are known and non-zero.  Each output is then a single product, the six-term sum of it is exact
  in fp32, and the float64 product differs from it by the three dropped terms only (2.5 x 2^-28 of it).  A missing term
  costs between 2^-19 and 1, a term issued in place of another at least 2^-20; the bound is 2^-22.  Where the reference
  has no product (the causal halo) the output is an exact zero.
* **Term projection.**  On dense random data the op is bilinear in its operands, so the kernel's error ``y - want64``
  is projected on each of the nine float64 tensors ``D_ij = op(piece_i(a), piece_j(b))``, per block of 32 output rows:
  ``c_ij = <y - want64, D_ij> / <D_ij, D_ij>`` is ~0 for an issued term, -1 for a missing one, +1 for one issued twice
  and -1/4 for one missing in 8 of the 32 rows.  ``|c_ij| <= 0.1`` for the six pairs with i + j <= 2.  The pieces are
  those of the operand the kernel splits (``kernel_form``: an upsampling layer splits its folded polyphase weights).

Every expected value comes from a float64 reference of the op (oracle/codec.py, torch conv2d); nothing is compared with the
code under test.  ``emulate`` is the torch stand-in for a kernel that tests/test_b3_probe_cpu.py mutates to show that both
instruments fire; tests/test_gpu_b3_products.py applies them to the kernels."""
import torch
import torch.nn.functional as F

from oracle import codec

X_RICH = 1 + 2.0 ** -9 + 2.0 ** -18            # pieces 1, 2^-9, 2^-18
W_RICH = 1 + 3 * 2.0 ** -11 + 2.0 ** -19       # pieces 1, 3 x 2^-11, 2^-19
X_PIECES = (1.0, 2.0 ** -9, 2.0 ** -18)
W_PIECES = (1.0, 3 * 2.0 ** -11, 2.0 ** -19)
TERMS = ((1, 1), (0, 2), (2, 0), (0, 1), (1, 0), (0, 0))      # (piece of a, piece of b) in issue order: small terms first
DROPPED = ((1, 2), (2, 1), (2, 2))
PROBE_BOUND = 2.0 ** -22      # of |want64|, elementwise
PROJ_BOUND = 0.1
ROTATIONS = 4
MAX_EXP = 4                   # operands are scaled by +-2^e, e in [-4, 4]


# ------------------------------------------------------------------------------------------------ pieces
def split3(t):
    """(h, m, l) as float32: the device split -- bf16 casts round to nearest even -- with h + m + l == t bit for bit."""
    t = t.float()
    h = t.bfloat16().float()
    r = t - h
    m = r.bfloat16().float()
    low = (r - m).bfloat16().float()
    assert torch.equal((h + m) + low, t), "the three pieces do not add up to the operand"
    return h, m, low


def _scales(shape, gen, signed):
    s = torch.pow(2.0, torch.randint(-MAX_EXP, MAX_EXP + 1, shape, generator=gen).double())
    if signed:
        s = s * (1 - 2 * torch.randint(0, 2, shape, generator=gen)).double()
    return s


def rich_activation(shape, seed, signed=True):
    """Dense float32 tensor of ``+-2^e X_RICH`` (exact), e drawn per element."""
    gen = torch.Generator().manual_seed(seed)
    return (X_RICH * _scales(shape, gen, signed)).float()


# ------------------------------------------------------------------------------------------------ hot assignments
def hot(rows, nin, taps, rot, cls=0, in_step=1):
    """(input channel, tap) of every output row for rotation ``rot`` (and class ``cls``: output phase / parity class whose
    taps are ``taps``).  Over ROTATIONS rotations every tap and every 16-channel input chunk is hot for some row of every
    32-row block (``assert_coverage``): j runs through 32 ROTATIONS consecutive values per block, the tap is j mod the tap
    count and the chunk 7 j + rot mod the chunk count.  ``in_step`` = 2 keeps to the even input channels."""
    row = torch.arange(rows)
    blk, r = row // 32, row % 32
    j = r + 32 * rot + 5 * blk + 11 * cls
    tap = torch.tensor(taps)[j % len(taps)]
    nch = -(-nin // 16)
    chunk = (7 * j + rot) % nch
    ncand = -(-torch.clamp(nin - 16 * chunk, max=16) // in_step)
    return 16 * chunk + in_step * ((3 * j + blk) % ncand), tap


def assert_coverage(rows, nin, ntaps, hots):
    """``hots``: the (input channel, tap) or (input channel, tap, checked) entries of all rotations and classes; ``checked`` is
    the bool mask of the rows whose product is held to the probe's bound in that entry (all of them when it is left out).
    In every full 32-row block every tap and every 16-channel chunk must have been hot on a checked row."""
    for b0 in range(0, rows - 31, 32):
        on = [e[2][b0:b0 + 32] if len(e) > 2 else torch.ones(32, dtype=torch.bool) for e in hots]
        taps = set(int(t) for e, m in zip(hots, on) for t in e[1][b0:b0 + 32][m])
        chunks = set(int(c) // 16 for e, m in zip(hots, on) for c in e[0][b0:b0 + 32][m])
        assert taps == set(range(ntaps)), (b0, sorted(set(range(ntaps)) - taps))
        assert chunks == set(range(-(-nin // 16))), (b0, sorted(set(range(-(-nin // 16))) - chunks))


def _values(rows, seed, rich, signed):
    gen = torch.Generator().manual_seed(seed)
    return (W_RICH if rich else 1.0) * _scales((rows,), gen, signed)


def probe_weight_1d(kind, cin, cout, k, s, rot, rich=True, signed=True, in_step=1):
    """(w float32, hots): ``(cout, cin, k)`` -- ``(cin, cout, k)`` for kind "convt" -- with one ``+-2^e W_RICH`` (or ``2^e``)
    per output row, and per output phase of a transposed layer (taps of one residue mod the stride)."""
    transposed = kind == "convt"
    classes = [[t for t in range(k) if t % s == p] for p in range(s)] if transposed else [list(range(k))]
    w = torch.zeros((cin, cout, k) if transposed else (cout, cin, k), dtype=torch.float64)
    row = torch.arange(cout)
    hots = []
    for c, taps in enumerate(classes):
        if not taps:
            continue
        ci, tap = hot(cout, cin, taps, rot, c, in_step)
        val = _values(cout, 1000 * rot + 17 * c + cout + k, rich, signed)
        if transposed:
            w[ci, row, tap] = val
        else:
            w[row, ci, tap] = val
        hots.append((ci, tap))
    return w.float(), hots


def probe_weight_2d(cin, cout, kh, kw, rot):
    """(w (cout, cin, kh, kw), hots): one hot (input channel, tap) per output channel -- the forward probe."""
    ci, tap = hot(cout, cin, list(range(kh * kw)), rot)
    w = torch.zeros(cout, cin, kh * kw, dtype=torch.float64)
    w[torch.arange(cout), ci, tap] = _values(cout, 2000 * rot + cout + kh * kw, True, True)
    return w.reshape(cout, cin, kh, kw).float(), [(ci, tap)]


def probe_weight_2d_bwd(cin, cout, kh, kw, sh, sw, rot):
    """(w (cout, cin, kh, kw), hots): one hot (output channel, tap) per INPUT channel and parity class (taps of one residue mod
    the stride in each direction reach one class of dx positions) -- the backward-data probe."""
    w = torch.zeros(cout, cin, kh * kw, dtype=torch.float64)
    hots = []
    for ph in range(sh):
        for pw in range(sw):
            taps = [a * kw + b for a in range(kh) for b in range(kw) if a % sh == ph and b % sw == pw]
            co, tap = hot(cin, cout, taps, rot, ph * sw + pw)
            w[co, torch.arange(cin), tap] = _values(cin, 3000 * rot + 31 * (ph * sw + pw) + cin, True, True)
            hots.append((co, tap))
    return w.reshape(cout, cin, kh, kw).float(), hots


def probe_resblock(c, k, d, batch, length, rot, which):
    """(x, w1 (c, c, k), w2 (c, c, 1), hots of w1, hots of w2) of residual-block probe "A" (rich w1, power-of-two w2) or "B"
    (power-of-two w1, rich w2).  All values positive (LeakyReLU is the identity), x is zero on the odd channels and conv1
    reads even channels only, so an odd output channel is the single product w2 w1 x with no residual.

    Only the odd outputs are held to the probe's bound, so the hots carry the mask of the rows that count: conv2 routes h row
    34 u + rot to output 2 u + 1, i.e. rotation ``rot`` checks the h rows of parity ``rot % 2`` -- every h row twice in
    four rotations.  conv1's hot (channel, tap) therefore turns with ``rot // 2``: the two rotations of a turn check the
    even and the odd h rows of the same assignment, 32 consecutive j of ``hot`` per block and turn.  conv2's chunks are those
    that the 16 odd rows of a block read in four rotations."""
    co = torch.arange(c)
    c1 = (34 * (co // 2) + rot + 8 * (1 - co % 2)) % c
    read = torch.zeros(c, dtype=torch.bool)
    read[c1[1::2]] = True                                   # the h rows that end on an odd output at this rotation
    w1, h1 = probe_weight_1d("causal", c, c, k, 1, rot // 2, rich=which == "A", signed=False, in_step=2)
    h1 = [(ci, tap, read) for ci, tap in h1]
    w2 = torch.zeros(c, c, 1, dtype=torch.float64)
    w2[co, c1, 0] = _values(c, 500 * rot + c + d, which == "B", False)
    w2, h2 = w2.float(), [(c1, torch.zeros(c, dtype=torch.long), co % 2 == 1)]
    x = rich_activation((batch, c, length), 77 * c + d + rot, signed=False)
    x[:, 1::2] = 0.0
    return x, w1, w2, h1, h2


# ------------------------------------------------------------------------------------------------ the ops (any dtype)
def conv1d_op(kind, s=1, d=1):
    """op(w, x, bias=None) of a 1-D layer kind, by the oracle's definitions."""
    def op(w, x, bias=None):
        if kind == "convt":
            return codec.causal_conv_t1d(x, w, bias, stride=s)
        if kind == "upconv":
            return codec.upsample_conv1d(x, w, bias, s)
        return codec.causal_conv1d(x, w, bias, stride=s, dilation=d)
    return op


def upconv_fold(w, s):
    """(s, cout, cin, 3): the polyphase weights an upsampling layer really contracts.  Output phase p of the K = 2 s + 1 'same'
    conv over the s-fold repeated input reads x[u - 1 + q], q = 0..2, with the SUM of the taps k that land there,
    floor((p + k - s) / s) == q - 1 -- summed in ``w``'s dtype in ascending k from zero, as csrc/pack.hip: fwd_weight does in
    fp32.  The kernel splits these sums, so the pieces of the weight operand are theirs, not those of the single taps."""
    cout, cin, k = w.shape
    assert k == 2 * s + 1
    out = torch.zeros(s, cout, cin, 3, dtype=w.dtype)
    for p in range(s):
        for kk in range(k):
            q = (p + kk - s) // s + 1
            out[p, :, :, q] = out[p, :, :, q] + w[:, :, kk]
    return out


def upconv_poly_op(s):
    """op(folded w, x, bias=None): the upsampling layer on its polyphase weights."""
    def op(wf, x, bias=None):
        xp = F.pad(x, (1, 1))
        y = torch.stack([F.conv1d(xp, wf[p]) for p in range(s)], dim=-1).reshape(x.shape[0], wf.shape[1], -1)
        return y if bias is None else y + bias.reshape(1, -1, 1)
    return op


def kernel_form(kind, s, d, w):
    """(op, weight operand) as the kernel contracts them: the folded polyphase weights for an upsampling layer (a sum of
    taps is formed BEFORE the split), the layer's own op and weight otherwise (strided, transposed and space-to-depth forms
    only move weights around)."""
    if kind == "upconv":
        return upconv_poly_op(s), upconv_fold(w.float(), s)
    return conv1d_op(kind, s, d), w


def conv2d_op(stride, pad):
    def op(w, x, bias=None):
        return F.conv2d(x, w, bias, stride, pad)
    return op


def conv2d_bwd_data_op(stride, pad, x_shape):
    """op(w, dy): the gradient of conv2d with respect to its input of shape ``x_shape``."""
    def op(w, dy, bias=None):
        x0 = torch.zeros(x_shape, dtype=w.dtype, requires_grad=True)
        dx, = torch.autograd.grad(F.conv2d(x0, w, None, stride, pad), x0, dy)
        return dx
    return op


def wgrad_op(fwd, w_shape):
    """op(dy, x): dW of the layer whose forward is ``fwd(w, x)``."""
    def op(dy, x, bias=None):
        w0 = torch.zeros(w_shape, dtype=x.dtype, requires_grad=True)
        dw, = torch.autograd.grad(fwd(w0, x), w0, dy)
        return dw
    return op


def product_count(op, a, b):
    """How many non-zero products each output sums: the op on the 0/1 masks of its operands, in float64."""
    return op((a != 0).double(), (b != 0).double())


def assert_one_product(op, a, b, interior=None):
    """The probe's precondition: at most one product per output, and at least one on ``interior`` (a bool mask)."""
    n = product_count(op, a, b)
    assert float(n.max()) <= 1.0, float(n.max())
    if interior is not None:
        assert bool((n[interior] >= 1).all()), "an output past the halo has no product"
    return n


def interior(op, a, b, phases=(1,)):
    """Bool mask of the outputs all of whose taps read real data (no padding, no halo): where the op on all-ones operands
    reaches its maximum, taken per output phase (``phases``: the period along each of the last dims).  For a causal stride-1
    layer this is t >= (K - 1) d."""
    n = op(torch.ones_like(a, dtype=torch.float64), torch.ones_like(b, dtype=torch.float64))
    m = torch.zeros_like(n, dtype=torch.bool)
    if len(phases) == 1:
        for p in range(phases[0]):
            m[..., p::phases[0]] = n[..., p::phases[0]] == n[..., p::phases[0]].max()
    else:
        for p in range(phases[0]):
            for q in range(phases[1]):
                part = n[..., p::phases[0], q::phases[1]]
                m[..., p::phases[0], q::phases[1]] = part == part.max()
    return m


# ------------------------------------------------------------------------------------------------ the emulated kernel
def emulate(op, a, b, bias=None, terms=TERMS):
    """The six-term arithmetic in torch: one fp32 op per (piece of a, piece of b) in ``terms``, summed in fp32 in that order."""
    pa, pb = split3(a), split3(b)
    y = None
    for i, j in terms:
        t = op(pa[i], pb[j])
        y = t if y is None else y + t
    return y if bias is None else y + bias.reshape((1, -1) + (1,) * (y.dim() - 2))


def mutations():
    """{name: term list}: each single omission, and each term issued in place of another."""
    names = {(0, 0): "hh", (0, 1): "hm", (1, 0): "mh", (1, 1): "mm", (0, 2): "hl", (2, 0): "lh"}
    out = {f"no {names[t]}": tuple(u for u in TERMS if u != t) for t in TERMS}
    for t in TERMS:
        for u in TERMS:
            if u != t:
                out[f"{names[u]} for {names[t]}"] = tuple(u if v == t else v for v in TERMS)
    return out


def in_rows(y_ok, y_bad, lo=0, hi=8, dim=1):
    """``y_bad`` in rows lo..hi of every 32-row block along ``dim``, ``y_ok`` elsewhere."""
    r = torch.arange(y_ok.shape[dim]) % 32
    shape = [1] * y_ok.dim()
    shape[dim] = -1
    return torch.where(((r >= lo) & (r < hi)).reshape(shape), y_bad, y_ok)


# ------------------------------------------------------------------------------------------------ the residual block
def resblock_ref(x, w1, b1, w2, b2, d):
    """(y, h) in float64: y = x + conv2(leaky(h)), h = conv1(x) -- oracle/codec.py: residual_block, plain weights."""
    sd = {"conv1.conv.weight": w1.double(), "conv2.conv.weight": w2.double()}
    if b1 is not None:
        sd["conv1.conv.bias"], sd["conv2.conv.bias"] = b1.double(), b2.double()
    h = codec.causal_conv1d(x.double(), sd["conv1.conv.weight"], sd.get("conv1.conv.bias"), dilation=d)
    return codec.residual_block(x.double(), sd, "", d), h


def resblock_emulate(x, w1, b1, w2, b2, d, terms1=TERMS, terms2=TERMS, rows1=None, rows2=None):
    """The block on the emulated arithmetic; ``rows1`` = (lo, hi): ``terms1`` holds in those rows of every 32 of h only,
    ``rows2``: ``terms2`` in those rows of every 32 of conv2's output only."""
    h = emulate(conv1d_op("causal", 1, d), w1, x, b1, terms1)
    if rows1 is not None:
        h = in_rows(emulate(conv1d_op("causal", 1, d), w1, x, b1), h, *rows1)
    a = codec.leaky(h)
    y = emulate(conv1d_op("causal"), w2, a, b2, terms2)
    if rows2 is not None:
        y = in_rows(emulate(conv1d_op("causal"), w2, a, b2), y, *rows2)
    return x + y


def resblock_conv1_terms(x, w1, w2, h64, d):
    """conv1's nine term tensors carried to the block's output in float64: conv2(leaky'(h) D_ij)."""
    slope = torch.where(h64 > 0, 1.0, codec.LEAKY_SLOPE).double()
    terms = term_tensors(conv1d_op("causal", 1, d), w1, x)
    return {ij: codec.causal_conv1d(slope * dt, w2.double(), None) for ij, dt in terms.items()}


def dense_resblock(c, k, d, batch, length, seed):
    gen = torch.Generator().manual_seed(seed)
    w1 = torch.randn(c, c, k, generator=gen) / (c * k) ** 0.5
    w2 = torch.randn(c, c, 1, generator=gen) / c ** 0.5
    b1, b2 = torch.randn(c, generator=gen) * 0.1, torch.randn(c, generator=gen) * 0.1
    return torch.randn(batch, c, length, generator=gen), w1, b1, w2, b2


# ------------------------------------------------------------------------------------------------ instrument 1
def probe_errors(y, want64):
    """(worst |y - want64| / |want64| over the outputs that have a product, in units of PROBE_BOUND; number of non-zero
    outputs where the reference has none)."""
    y = y.detach().cpu().double()
    assert y.shape == want64.shape, (y.shape, want64.shape)
    has = want64 != 0
    assert bool(has.any())
    rel = ((y - want64).abs()[has] / want64.abs()[has]).max()
    return float(rel) / PROBE_BOUND, int((y[~has] != 0).sum())


def assert_probe(y, want64, what=""):
    worst, stray = probe_errors(y, want64)
    assert stray == 0, (what, "non-zero outputs where the reference has no product", stray)
    assert worst <= 1.0, (what, f"|y - want| = {worst:.3g} x 2^-22 |want|")
    return worst


# ------------------------------------------------------------------------------------------------ instrument 2
def term_tensors(op, a, b):
    """The nine float64 tensors D_ij = op(piece_i(a), piece_j(b))."""
    pa, pb = split3(a), split3(b)
    return {(i, j): op(pa[i].double(), pb[j].double()) for i in range(3) for j in range(3)}


def projection(y, want64, terms, dim=1, block=32):
    """{(i, j): c_ij per block of ``block`` output rows along ``dim``}."""
    e = (y.detach().cpu().double() - want64).movedim(dim, 0)
    e = e.reshape(e.shape[0], -1)
    out = {}
    for ij, dt in terms.items():
        dt = dt.movedim(dim, 0).reshape(e.shape[0], -1)
        num = torch.stack([(e[r:r + block] * dt[r:r + block]).sum() for r in range(0, e.shape[0], block)])
        den = torch.stack([(dt[r:r + block] ** 2).sum() for r in range(0, e.shape[0], block)])
        out[ij] = num / den
    return out


def worst_coefficients(c):
    """{(i, j): the c_ij of largest magnitude over the blocks}."""
    return {ij: float(v[v.abs().argmax()]) for ij, v in c.items()}


def format_coefficients(c):
    w = worst_coefficients(c)
    names = "hml"
    return " ".join(f"{names[i]}{names[j]}={w[(i, j)]:+.4f}" for i, j in TERMS + DROPPED)


def assert_projection(c, what=""):
    """|c_ij| <= 0.1 in every block for the six issued pairs; the three dropped ones are reported only (they read -1)."""
    line = format_coefficients(c)
    print(f"c_ij {what}: {line}")
    w = worst_coefficients(c)
    bad = {ij: v for ij, v in w.items() if ij in TERMS and not abs(v) <= PROJ_BOUND}
    assert not bad, (what, line)
    return line


# ------------------------------------------------------------------------------------------------ dense random layers
def dense_layer_1d(kind, cin, cout, k, batch, length, seed):
    """(x, w, bias) of the existing tests' kind: normal x, w / sqrt(cin k), bias 0.1 normal -- no weight norm, so that the
    pieces of the weight the kernel splits are the pieces of ``w``."""
    gen = torch.Generator().manual_seed(seed)
    shape = (cin, cout, k) if kind == "convt" else (cout, cin, k)
    w = torch.randn(shape, generator=gen) / (cin * k) ** 0.5
    bias = torch.randn(cout, generator=gen) * 0.1
    return torch.randn(batch, cin, length, generator=gen), w, bias


# the conv_b3 ring layers: channel counts of LAYERS / STRIDED in tests/test_gpu_conv_b3.py, (batch, length) one shorter than a
# tile and one ragged over two tiles
RING_UP = [("up8", "upconv", 512, 256, 17, 8), ("up5", "upconv", 256, 128, 11, 5), ("up4", "upconv", 128, 64, 9, 4),
           ("up2", "upconv", 64, 32, 5, 2), ("k7", "convt", 512, 512, 7, 1), ("up4", "upconv", 512, 256, 9, 4)]
RING_DOWN = [("down2", "causal", 32, 64, 5, 2), ("down4", "causal", 64, 128, 9, 4), ("down5", "causal", 128, 256, 11, 5),
             ("down8", "causal", 256, 512, 17, 8), ("k3", "causal", 512, 512, 3, 1), ("down4", "causal", 256, 512, 9, 4)]
UP_LENGTHS = ((2, 60), (1, 129))
DOWN_LENGTHS = ((2, 64), (1, 521))
RING = [(row, UP_LENGTHS) for row in RING_UP] + [(row, DOWN_LENGTHS) for row in RING_DOWN]
RING_IDS = [f"{row[0]}-{row[2]}" for row, _ in RING]
MFMA_K9S3 = ("causal", 64, 128, 9, 3, 2, 400)       # the k9 s3 layer of test_other_layers_keep_their_kernels: no ring form

# the fused residual block's ring kernel: every (C, dilation) it has, lengths one past a tile and ragged over two (per clip)
RB_TILE = {32: 512, 64: 512, 128: 256, 256: 128}
RB_RING = [(c, d) for c in (32, 64, 128, 256) for d in (1, 3, 9)]


def rb_lengths(c):
    return ((1, RB_TILE[c] + 1), (2, RB_TILE[c] + 37))


# Conv2d: (batch, cin, cout, h, w, kh, kw, sh, sw, ph, pw) -> kernel name; the smallest shape of tests/test_gpu_conv2d_b3.py
# (and the patch-tile row of tests/test_gpu_tile_variants.py) per name
C2D_FWD = [((2, 32, 32, 37, 128, 3, 3, 1, 1, 1, 1), "conv2d_b3<3x3,32x256>"),
           ((2, 32, 64, 21, 96, 3, 3, 1, 1, 1, 1), "conv2d_b3<3x3,64x256>"),
           ((1, 64, 128, 19, 30, 3, 3, 1, 1, 1, 1), "conv2d_b3<3x3,128x128>"),
           ((2, 32, 64, 21, 64, 3, 4, 1, 2, 1, 1), "conv2d_b3<3x4 s(1,2) as 3x2 s2d,64x256>"),
           ((1, 128, 128, 17, 128, 3, 4, 1, 2, 1, 1), "conv2d_b3<3x4 s(1,2) as 3x2 s2d,128x128>"),
           ((2, 64, 128, 22, 64, 4, 4, 2, 2, 1, 1), "conv2d_b3<4x4 s2 as 2x2 s2d,128x128>"),
           ((1, 16, 32, 64, 64, 3, 3, 1, 1, 0, 0), "conv_mfma<1,4,1,4,16>")]
# backward-data; the last two have a base grid wider than 192 columns: the q == 2 plan with the peeled first column
C2D_BWD = [((2, 32, 32, 37, 128, 3, 3, 1, 1, 1, 1), "conv2d_b3<3x3,32x256>"),
           ((1, 64, 128, 19, 30, 3, 3, 1, 1, 1, 1), "conv2d_b3<3x3,64x256>"),
           ((1, 128, 256, 15, 16, 3, 3, 1, 1, 1, 1), "conv2d_b3<3x3,128x128>"),
           ((2, 32, 64, 21, 62, 3, 4, 1, 2, 1, 1), "conv2d_b3<3x2 phases 1x2,64x256>"),
           ((1, 128, 128, 17, 126, 3, 4, 1, 2, 1, 1), "conv2d_b3<3x2 phases 1x2,128x128>"),
           ((1, 128, 256, 30, 30, 4, 4, 2, 2, 1, 1), "conv2d_b3<2x2 phases 2x2,128x128>"),
           ((1, 32, 64, 9, 512, 3, 4, 1, 2, 1, 1), "conv2d_b3<3x2 phases 1x2,64x256>"),
           ((1, 128, 128, 5, 384, 4, 4, 2, 2, 1, 1), "conv2d_b3<2x2 phases 2x2,128x128>")]


def out_shape_2d(f):
    b, cin, cout, h, w, kh, kw, sh, sw, ph, pw = f
    return b, cout, (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1


# weight gradients whose contraction is bf16x3: the staged 1-D kernel (the default dispatch answers a bf16x3 descriptor with
# the exact fp32 direct kernel; knob dw_direct = 0 puts it back on the staged one), (kind, cin, cout, k, s, batch, length) ...
WGRAD_1D = [(("causal", 32, 128, 7, 1, 2, 300), "conv_bwd_weight<2,2,2,2,1>"),
            (("causal", 32, 64, 5, 2, 2, 300), "conv_bwd_weight<1,2,2,2,1>"),
            (("causal", 16, 32, 7, 1, 2, 300), "conv_bwd_weight<1,1,1,4,1>"),
            (("upconv", 64, 32, 5, 2, 2, 150), "conv_bwd_weight<1,2,2,2,1>"),
            (("convt", 32, 48, 5, 2, 2, 150), "conv_bwd_weight<1,2,2,2,1>")]
# ... and the staged and shared 2-D kernels, (batch, cin, cout, h, w, kh, kw, sh, sw, ph, pw): B3_SHAPES of
# tests/test_gpu_weight_grad_training_size.py
WGRAD_2D = [((2, 16, 80, 8, 64, 3, 3, 1, 1, 1, 1), "conv2d_bwd_weight_shared<2,2,2,2,1>"),
            ((2, 16, 48, 8, 64, 3, 3, 1, 1, 1, 1), "conv2d_bwd_weight_shared<2,1,1,4,1>"),
            ((2, 16, 128, 8, 32, 3, 3, 2, 1, 1, 1), "conv2d_bwd_weight<2,2,2,2,1>"),
            ((2, 16, 64, 8, 32, 3, 3, 2, 1, 1, 1), "conv2d_bwd_weight<1,2,2,2,1>"),
            ((2, 8, 32, 8, 32, 3, 3, 2, 1, 1, 1), "conv2d_bwd_weight<1,1,1,4,1>")]
