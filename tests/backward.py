"""Per-element judge for the backward pass of a decoder training step (helper, not collected).

A train step (csrc/api_train.hip) saves every activation of its forward pass and runs a backward pass that is LINEAR in that saved
state: ReLU masks, pool winners and TV signs are read from it, never recomputed.  So the reference here does not re-derive the
forward pass (whose fp16 roundings would flip masks and winners, which is why tests/test_gpu_train.py needs 1e-3 .. 6e-2 on a
Frobenius ratio).  It takes the forward state from the device: every saved activation is rebuilt bit for bit through the op-level
entry points (build_state with GpuOps; those kernels are pinned per element by tests/test_gpu_pointwise.py), the rebuild is proved by
the three losses (losses_from_state: equal to the returned ones to one fp32 ulp), and the backward pass is then run in float64 on
that state (backward).  Every element of every dW and db is held against its own bound,

    |got - want| <= e

`want`: float64 adjoints, masks from the rebuilt post-ReLU activations (as relu_mask16/32_kernel take them), pool winners = first
maximum in row-major order of the rebuilt fp16 pool input, TV signs from the float32 differences of D, data gradients through the
fp32 master weights (decoder w32, encoder fp32 weights, folded fp32 conv1_1), weight gradients from the rebuilt fp16 inputs with
reflect pad and folded x2 upsample.  `e` is carried down the same chain (Track): every stage is linear, y = f(g), with a
non-negative abs-operator |f| (the same stage on |W|, |activation|, 0/1 masks), and a device that computes it with constant tau
from an input that is off by e_in returns, to first order,

    e_out = |f| e_in + tau |f| |g_in| + a

The coarser form tau_path * s + a_path, with s the whole chain run on absolute values from the seed |feature term| + |pixel term| +
|tv term| and tau_path the sum of the stage constants, dominates e element by element (|g_in| <= s_in at every stage), so e is
never the wider of the two; it is used because the coarse s outgrows the gradient by sqrt(9 Cin) per layer of zero-mean filters
and would see nothing below the first decoder layer (see SEEDS).  The stage constants, with u = 2^-24 (fp32 round to nearest):

 * mse seed (mse_kernel): d = a - b, gscale = 2 weight / n on the host, gscale * d: 3 roundings, tau = 3u.
 * the seeds at D: the pixel term 3u as above, the tv term 2u (weight / B, times a small integer), and two accumulating adds of u
   each: charged as 5u (|feature term| + |pixel term| + |tv term|) on top of the feature path's e (a sum bound, not the max).
 * conv_first_dgrad_kernel: per channel up to 9 * 64 products and adds into one fp32 register: 576 adds and one product rounding
   ahead of each (a contracted multiply-add only removes roundings): tau = 577u.  fp32 filters, no MFMA, no doubling.
 * reflect_fold_kernel: ny * nx terms added to a zero register, ny = 1 + [y == 1] + [y == H - 2] (3 when H == 3), same for nx:
   4 adds where H, W >= 4, up to 9 on a 3-wide map: tau = fold_adds(H, W) u.
 * upsample_adjoint_kernel: (p0 + p1) + (p2 + p3): charged 3u.  Masks, pool adjoint, pad3to4, transpose_w: exact.
 * colsum_rows_kernel + reduce_slabs_kernel (bias): rows split over nslab = min(rows, 256) blocks of per = ceil(rows / nslab) rows, a
   block's rows over rg = 256 / min(C, 256) row groups: ceil(per / rg) adds per thread, rg - 1 to join the groups, nslab adds in the
   second stage.  A sum of that depth errs by at most depth * u * sum|g|: tau = bias_adds(rows, C) u.
 * gemm_f16x2_kernel.  A split operand x (scaled by a power of two: exact) is hi = fp16(x), lo = fp16(x - hi): |x - hi - lo| <=
   2^-22 |x| while lo is a normal fp16 number.  dgrad splits both operands (2 * 2^-22, and the dropped lo * lo <= 2^-22 of the
   product); wgrad splits the gradient alone, the activation is an exact fp16 number.  Every product is exact in fp32.  Per k the
   accumulator takes mf = 3 (dgrad: lo hi, hi lo, hi hi) or 2 (wgrad) products, whose absolute sum is <= (1 + 2^-10) of the term, so
   K terms are mf K additions: <= mf K u (1 + 2^-10) s, doubled for an MFMA whose internal adds are not individually rounded to
   nearest (as pointwise.tau_direct): tau_gemm = splits 2^-22 [+ 2^-22] + 2 mf K u (1 + 2^-10).  K = 9 Cout for dgrad (the padded 4
   for the 64 -> 3 layer), the longest slab for wgrad; the slab sum adds ns u (reduce_slabs_kernel, from zero).  The epilogue's
   1 / (sa sb) is a power of two.
 * `a`, the absolute floor of a subnormal lo half: |lo| < 2^-14 is rounded to the spacing 2^-24, an absolute 2^-25 whatever x.
   launch_pow2_scale brings max|g| = m into [2^13, 2^14): scale = 2^(14-e) with m >= 2^(e-1), so 2^-25 / scale <= 2^-38 m per
   gradient value, times the sum of |other operand| over the terms.  m is taken from `want`; (1 + 2^-10) covers the device's own m.
   The weights of a dgrad are split UNSCALED (b_scale = 1): He-normal filters of ~2^-5 have |x - hi| < 2^-16, so their lo half is
   always subnormal: 2^-25 per weight, times sum |g| over the terms (first order: |want g|).

No constant here is fitted to a GPU run.  tests/test_backward_cpu.py holds the float64 adjoints against plain autograd to 1e-12,
runs a NumPy float32 emulation of this arithmetic (emulate) inside HALF of every bound, and shows which listed case catches which
seeded defect of the emulation.

Adam (adam_kernel, apply_adam): adam_c below derives the constant of its bound.
"""
import numpy as np

import pointwise as pw
from wct_tf_amd.weights import ENCODER_CONVS, decoder_plan, RELU_LEVEL

U = 2.0 ** -24
ENC = ENCODER_CONVS[1:]                                   # csrc/api.h: enc[i], i = 0 is conv1_2
POOL_AFTER = (1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0)         # ENC_POOL_AFTER
TAP = (0, 2, 0, 3, 0, 0, 0, 4, 0, 0, 0, 5)                # ENC_TAP
LOSS_WEIGHTS = (1.0, 0.7, 1e-4)                           # feature, pixel, tv: all three seeds live
# Every case is judged twice.  With all three seeds live the bound at the decoded image carries the feature path: five (relu2_1) or
# seven split GEMMs and conv1_1 through |W|, and the abs-chain of zero-mean He filters outgrows the signed one by ~sqrt(9 Cin) per
# layer, so from relu2_1 on that bound is as large as the gradient itself or larger: it sees neither a dropped slab (0.77 at 64x64)
# nor a missing quarter of the upsample adjoint (0.04; tests/test_backward_cpu.py measures both).  With the feature seed off (0 * d
# is an exact zero all the way down) the decoder's own chain is left, on which the bound is 10 .. 1000 roundings wide and sees every
# listed decoder defect.  The encoder's adjoints are seen on the TIES case below, whose non-negative encoder does not inflate the bound.
SEEDS = {'all': LOSS_WEIGHTS, 'dec': (0.0, 0.7, 1e-4)}
A_G = 2.0 ** -38 * (1 + 2.0 ** -10)                       # per unit of max|g|
A_W = 2.0 ** -25

# (relu, B, H, W): the smallest shapes at which each thing can go wrong (see tests/test_gpu_backward.py)
CASES = [
    ('relu1_1', 1, 3, 5), ('relu1_1', 2, 12, 10), ('relu1_1', 3, 17, 33),
    ('relu1_1', 1, 64, 64), ('relu1_1', 1, 70, 90), ('relu1_1', 3, 34, 46),
    ('relu2_1', 1, 4, 12), ('relu2_1', 2, 16, 12), ('relu2_1', 1, 64, 64),
    ('relu3_1', 1, 8, 12), ('relu3_1', 2, 16, 24),
]
# One more, on tie_weights(): the decoded image is constant, so every 2x2 window of conv1_2's output is a four-way tie between
# positive values, and the encoder's filters are non-negative, so its abs-chain IS its chain and the bound stays sharp through the
# second encoder pass: the case that sees which maximum the pool adjoint picks.
TIES = ('relu2_1', 1, 8, 8)
CASES.append(TIES)


def case_id(c):
    return '%s-%dx%dx%d' % c


def case_weights(case):
    """He-normal synthetic weights for the relu target of `case`; tie_weights() for TIES."""
    from wct_tf_amd.weights import synthetic_weights
    return tie_weights() if tuple(case) == TIES else synthetic_weights(42, relu_targets=[case[0]])


def tie_weights():
    """relu2_1: conv1_1, conv1_2, conv2_1 take the weighted mean of their inputs (|He filter| normalised per output channel, no bias);
    the output conv of the decoder is all bias, which the training forward does not clip."""
    from wct_tf_amd.weights import synthetic_weights
    w = synthetic_weights(42, relu_targets=['relu2_1'])
    enc = dict(w['encoder'])
    for name, _, cout in ENCODER_CONVS[:3]:
        a = np.abs(enc[name][0])
        enc[name] = (np.float32(a / a.sum(axis=(0, 1, 2), keepdims=True)), np.zeros(cout, np.float32))
    dec = list(w['decoder']['relu2_1'])
    dec[-1] = (np.zeros_like(dec[-1][0]), np.float32([1.5, 1.25, 1.75]))
    return {'encoder': enc, 'decoder': {'relu2_1': dec}}


def case_images(b, h, w):
    from wct_tf_amd.weights import synthetic_image
    return np.stack([synthetic_image(500 + 7 * h + w + i, h, w) / 255. for i in range(b)]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# split-K geometry (conv_wgrad_splits / launch_conv_wgrad restated)
# ---------------------------------------------------------------------------------------------------------------------
def wgrad_slabs(p):
    """(nsplit asked for, ksplit, slabs launched, length of the last slab) for P = B H W."""
    nsplit = min(max(p // 2048, 1), 128)
    ksplit = (-(-p // nsplit) + 31) // 32 * 32
    ns = -(-p // ksplit)
    return nsplit, ksplit, ns, p - (ns - 1) * ksplit


def fold_adds(h, w):
    return (3 if h == 3 else 2) * (3 if w == 3 else 2)


def bias_adds(rows, c):
    nslab = min(rows, 256)
    per = -(-rows // nslab)
    rg = 256 // min(c, 256)
    return -(-per // rg) + (rg - 1) + nslab


def tau_gemm(k, mf, splits):
    return splits * 2.0 ** -22 + (2.0 ** -22 if splits == 2 else 0.0) + 2.0 * mf * k * U * (1 + 2.0 ** -10)


# ---------------------------------------------------------------------------------------------------------------------
# forward state: what wct_train_step saves, rebuilt per image
# ---------------------------------------------------------------------------------------------------------------------
class GpuOps(object):
    """The op-level entry points of the library.  `helper` is a second context whose relu1_1 decoder is replaced by
    [identity, (w_last, b_last)] to reach conv_last_kernel (as tests/test_gpu_pointwise.py::test_conv_last does)."""

    def __init__(self, ctx, helper):
        self.ctx, self.helper = ctx, helper

    r16 = staticmethod(pw.h16)

    def encode(self, img, relu):
        return self.ctx.encode(img, relu)

    def first(self, img):
        return self.ctx.encode(img, 'relu1_1')

    def conv16(self, x, w, b, up):
        return self.ctx.conv3x3_f16(x, w, b, relu=True, upsample=up, algo=1)

    def conv32(self, x, w, b):
        return self.ctx.conv3x3(x, w, b, relu=True)

    def pool(self, x):
        return self.ctx.maxpool(x)

    def last(self, x, w, b):
        ident = pw.identity_conv64()
        assert np.array_equal(self.helper.conv3x3_f16(x, ident[0], ident[1], relu=True, algo=0), x)      # the hand-over
        self.helper.set_decoder('relu1_1', [ident, (w, b)])
        return np.stack([self.helper.decode(xi, 'relu1_1') for xi in x])


class CpuOps(object):
    """rounded=True: the fp16-operand / fp32-accumulate forward of the device emulated with float64 sums (a stand-in where there is
    no GPU: any forward state will do for the backward pass).  rounded=False: plain float64, nothing rounded."""

    def __init__(self, enc, rounded=True):
        self.enc, self.rounded = enc, rounded
        self.fw, self.fb = pw.fold_first(enc)

    def r16(self, a):
        return pw.h16(a) if self.rounded else np.asarray(a, np.float64)

    def r32(self, a):
        return np.float32(a) if self.rounded else a

    def first(self, img):
        return self.r32(np.maximum(pw._conv64(img, self.fw, self.fb, False), 0))

    def conv16(self, x, w, b, up):
        return self.r16(self.conv32(x, w, b, up))

    def conv32(self, x, w, b, up=False):
        return self.r32(np.maximum(pw._conv64(self.r16(x), self.r16(w), b, up), 0))

    def pool(self, x):
        return pw.pool_same(x)

    def last(self, x, w, b):
        return self.r32(pw._conv64(self.r16(x), self.r16(w), b, False))

    def encode(self, img, relu):
        lvl = RELU_LEVEL[relu]
        cur = self.first(img)
        if lvl == 1:
            return cur
        cur = self.r16(cur)
        for i, (name, _, _) in enumerate(ENC):
            w, b = self.enc[name]
            if TAP[i] == lvl:
                return self.conv32(cur, w, b)
            cur = self.conv16(cur, w, b, False)
            if POOL_AFTER[i]:
                cur = self.pool(cur)


def build_state(ops, weights, relu, x):
    """Every array a train step on the batch x [B][H][W][3] keeps, in the driver's order (csrc/api_train.hip)."""
    lvl = RELU_LEVEL[relu]
    enc, dec = weights['encoder'], weights['decoder'][relu]
    n = len(x)
    st = {'relu': relu, 'x': x, 'F': np.stack([ops.encode(x[i], relu) for i in range(n)])}
    cur = ops.r16(st['F'])
    st['dec_in'], st['dec_out'], st['dec_up'] = [], [], []
    up, it = False, iter(dec)
    for kind, cin, cout, _ in decoder_plan(relu):
        if kind == 'U':
            up = True
            continue
        w, b = next(it)
        st['dec_in'].append(cur)
        st['dec_up'].append(up)
        if cout == 3:
            st['D'] = ops.last(cur, w, b)
            st['dec_out'].append(None)
        else:
            cur = ops.conv16(cur, w, b, up)
            st['dec_out'].append(cur)
        up = False
    first = np.stack([ops.first(st['D'][i]) for i in range(n)])          # the decoded image is NOT clipped in training
    st['enc'] = []
    if lvl == 1:
        st['e0'], st['Fp'] = None, first
        return st
    st['e0'] = cur = ops.r16(first)
    tap = TAP.index(lvl)
    for i in range(tap + 1):
        w, b = enc[ENC[i][0]]
        if i == tap:
            st['Fp'] = np.stack([ops.conv32(cur[j], w, b) for j in range(n)])
            st['enc'].append({'i': i, 'out': None, 'pooled': None})
        else:
            out = ops.conv16(cur, w, b, False)
            pooled = np.stack([ops.pool(out[j]) for j in range(n)]) if POOL_AFTER[i] else None
            st['enc'].append({'i': i, 'out': out, 'pooled': pooled})
            cur = out if pooled is None else pooled
    return st


def losses_from_state(st, lw=LOSS_WEIGHTS):
    """(feature, pixel, tv) as mse_kernel / tv_kernel / finish_sum_kernel compute them: float32 difference, square or absolute
    value, sum in double, one cast to float."""
    fw, pxw, tvw = (np.float64(np.float32(v)) for v in lw)

    def mse(a, b, wt):
        d = np.float32(a) - np.float32(b)
        return np.float32(np.sum(np.float64(d) ** 2) * (wt / d.size))
    d = np.float32(st['D'])
    tv = np.sum(np.float64(np.abs(d[:, 1:] - d[:, :-1]))) + np.sum(np.float64(np.abs(d[:, :, 1:] - d[:, :, :-1])))
    return mse(st['Fp'], st['F'], fw), mse(st['D'], st['x'], pxw), np.float32(tv * (tvw / len(d)))


# ---------------------------------------------------------------------------------------------------------------------
# the adjoints in float64
# ---------------------------------------------------------------------------------------------------------------------
def dgrad_pad(g, w):
    """gp[b][y'][x'][ci] = sum_{tap, co} g[b][y' - ky][x' - kx][co] w[ky][kx][ci][co] over the padded grid (H + 2) x (W + 2)."""
    b, h, wd, co = g.shape
    g2 = np.pad(g, ((0, 0), (2, 2), (2, 2), (0, 0)))
    out = np.zeros((b * (h + 2) * (wd + 2), w.shape[2]), np.result_type(g, w))
    for ky in range(3):
        for kx in range(3):
            out += np.ascontiguousarray(g2[:, 2 - ky:4 - ky + h, 2 - kx:4 - kx + wd]).reshape(-1, co) @ w[ky, kx].T
    return out.reshape(b, h + 2, wd + 2, -1)


def fold(gp):
    """Adjoint of the 1-px reflect pad: padded row 0 folds onto image row 1, padded row H + 1 onto image row H - 2; same for columns."""
    t = np.array(gp)
    for ax in (1, 2):
        t = np.moveaxis(t, ax, 0)
        n = t.shape[0] - 2
        t[2] += t[0]
        t[n - 1] += t[n + 1]
        t = np.moveaxis(t[1:n + 1], 0, ax)
    return np.ascontiguousarray(t)


def upsample(x):
    return np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)


def wgrad(x, up, g):
    """dW[ky][kx][ci][co] = sum_{b,y,x} pad(x)[b][y + ky][x + kx][ci] g[b][y][x][co]."""
    if up:
        x = upsample(x)
    b, h, wd, co = g.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode='reflect')
    out = np.empty((3, 3, x.shape[3], co), np.result_type(x, g))
    gm = g.reshape(-1, co)
    for ky in range(3):
        for kx in range(3):
            out[ky, kx] = np.ascontiguousarray(xp[:, ky:ky + h, kx:kx + wd]).reshape(-1, x.shape[3]).T @ gm
    return out


def up_adjoint(g):
    b, h, w, c = g.shape
    return g.reshape(b, h // 2, 2, w // 2, 2, c).sum(axis=(2, 4))


def pool_winners(pre, last=False):
    """Index 0..3 (dy * 2 + dx) of the maximum of every 2x2 window: the first in row-major order (last=True: the last)."""
    b, h, w, c = pre.shape
    assert h % 2 == 0 and w % 2 == 0                 # a train step takes H, W that are multiples of the level's stride
    blk = pre.reshape(b, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 5, 2, 4).reshape(b, h // 2, w // 2, c, 4)
    return 3 - blk[..., ::-1].argmax(-1) if last else blk.argmax(-1)


def pool_adjoint(arg, g):
    b, ho, wo, c = g.shape
    out = np.zeros((b, ho, wo, c, 4), g.dtype)
    np.put_along_axis(out, arg[..., None], g[..., None], -1)
    return out.reshape(b, ho, wo, c, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(b, 2 * ho, 2 * wo, c)


def tv_signs(d):
    """sum of the signed unit terms of d tv / d D, signs from the float32 differences of D."""
    d = np.float32(d)
    out = np.zeros(d.shape, np.float64)
    dy, dx = np.sign(d[:, 1:] - d[:, :-1]), np.sign(d[:, :, 1:] - d[:, :, :-1])
    out[:, :-1] -= dy
    out[:, 1:] += dy
    out[:, :, :-1] -= dx
    out[:, :, 1:] += dx
    return out


class Track(object):
    """A gradient tensor on its way down the chain: float64 value g and the bound e of the device's error in it, element by element."""

    def __init__(self, g, e):
        self.g, self.e = g, e

    def lin(self, f, fabs, tau=0.0, a=0.0):
        """A linear stage f with abs-operator fabs and constant tau: e_out = |f| e_in + tau |f| |g_in| + a."""
        return Track(f(self.g), fabs(self.e) + tau * fabs(np.abs(self.g)) + a)

    def mask(self, act):
        m = np.asarray(act) > 0
        return Track(self.g * m, self.e * m)

    def dgrad(self, w):
        """launch_conv_dgrad: split GEMM over the padded grid, then the fold."""
        w = np.float64(w)
        wa = np.abs(w)
        h, wd, cout = self.g.shape[1:]
        floor = A_G * np.abs(self.g).max() * dgrad_pad(np.ones_like(self.g), wa) + A_W * dgrad_pad(np.abs(self.g), np.ones_like(wa))
        t = self.lin(lambda v: dgrad_pad(v, w), lambda v: dgrad_pad(v, wa), tau_gemm(9 * max(cout, 4), 3, 2), floor)
        return t.lin(fold, fold, fold_adds(h, wd) * U)


def backward(st, weights, lw=LOSS_WEIGHTS):
    """[((dW, bound), (db, bound))] per decoder conv, in float64, from the saved state `st`."""
    relu = st['relu']
    enc, dec = weights['encoder'], weights['decoder'][relu]
    fw, pxw, tvw = (np.float64(np.float32(v)) for v in lw)
    f64 = np.float64
    x, d, fp = f64(st['x']), f64(st['D']), f64(st['Fp'])
    n, h, w = x.shape[:3]
    g = 2 * fw / fp.size * (fp - f64(st['F']))
    t = Track(g, 3 * U * np.abs(g)).mask(st['Fp'])
    for k in range(len(st['enc']) - 1, -1, -1):
        es = st['enc'][k]
        t = t.dgrad(enc[ENC[es['i']][0]][0])
        if k > 0:
            pv = st['enc'][k - 1]
            if pv['pooled'] is not None:
                arg = pool_winners(pv['out'])
                t = t.lin(lambda v: pool_adjoint(arg, v), lambda v: pool_adjoint(arg, v))
            t = t.mask(pv['out'])
        else:
            t = t.mask(st['e0'])
    f1 = f64(pw.fold_first(enc)[0])
    t = t.lin(lambda v: dgrad_pad(v, f1), lambda v: dgrad_pad(v, np.abs(f1)), 577 * U)
    t = t.lin(fold, fold, fold_adds(h, w) * U)
    pix, tv = 2 * pxw / d.size * (d - x), tvw / n * tv_signs(st['D'])
    t = Track(t.g + pix + tv, t.e + 5 * U * (np.abs(t.g) + np.abs(pix) + np.abs(tv)))
    out = [None] * len(dec)
    for k in range(len(dec) - 1, -1, -1):
        wk = dec[k][0]
        cin, cout = wk.shape[2:]
        xin, up = f64(st['dec_in'][k]), st['dec_up'][k]
        if cout != 3:
            t = t.mask(st['dec_out'][k])
        ga = np.abs(t.g)
        px = ga.shape[0] * ga.shape[1] * ga.shape[2]
        db = (t.g.sum(axis=(0, 1, 2)), t.e.sum(axis=(0, 1, 2)) + bias_adds(px, cout) * U * ga.sum(axis=(0, 1, 2)))
        _, ksplit, ns, _ = wgrad_slabs(px)
        ax = np.abs(xin)
        dw = (wgrad(xin, up, t.g), wgrad(ax, up, t.e + (tau_gemm(min(ksplit, px), 2, 1) + ns * U) * ga + A_G * ga.max()))
        out[k] = (dw, db)
        if k > 0:
            t = t.dgrad(wk)
            if up:
                t = t.lin(up_adjoint, up_adjoint, 3 * U)
    return out


def judge_layer(got, ref):
    """(worst err / bound, its index, rel L2) of one dW or db against (want, bound)."""
    want, bound = ref
    r, at = pw.judge(got, want, bound, 1.0)
    return r, at, float(np.linalg.norm(np.float64(got) - want) / max(np.linalg.norm(want), 1e-300))


# ---------------------------------------------------------------------------------------------------------------------
# float32 emulation of the device's backward arithmetic, with seeded defects
# ---------------------------------------------------------------------------------------------------------------------
DEFECTS = ['fold_corner', 'fold_row', 'mask_below', 'up_term', 'pool_last', 'tap_T', 'slab_last', 'k_tail', 'pad_leak', 'bias_group']
f32 = np.float32


def _pow2_scale(g):
    m = float(np.abs(g).max())
    if not (0 < m < 1e30):
        return 1.0
    return float(np.ldexp(1.0, 14 - np.frexp(f32(m))[1]))


def _split(x):
    hi = pw.h16(x)
    return np.float64(hi), np.float64(pw.h16(x - hi))


def gemm32(a, b, sa, sb, a_exact, slabs, defect=None):
    """gemm_f16x2_kernel: a [M][K], b [K][N] float32; slabs = [(kbeg, kend)].  Per slab an fp32 accumulator takes, per k-step of 32
    and 16-wide MFMA, lo hi (if a is split), hi lo, hi hi, each an exact sum of 16 products; the slabs are added in order."""
    ah, al = _split(f32(a * f32(sa)))
    bh, bl = _split(f32(b * f32(sb)))
    inv = f32(1.0 / (sa * sb))
    total = np.zeros((a.shape[0], b.shape[1]), f32)
    for si, (kbeg, kend) in enumerate(slabs):
        if defect == 'slab_last' and si == len(slabs) - 1 and si > 0:
            continue
        acc = np.zeros((a.shape[0], b.shape[1]), np.float64)       # holds float32 values
        for k0 in range(kbeg, kend, 32):
            if defect == 'k_tail' and kend - k0 < 32:
                continue
            for c0 in range(k0, min(k0 + 32, kend), 16):
                c1 = min(c0 + 16, kend)
                if not a_exact:
                    acc = np.float64(f32(acc + al[:, c0:c1] @ bh[c0:c1]))
                acc = np.float64(f32(acc + ah[:, c0:c1] @ bl[c0:c1]))
                acc = np.float64(f32(acc + ah[:, c0:c1] @ bh[c0:c1]))
        total = total + f32(f32(acc) * inv)
    return total


def _seq_sum(terms):
    acc = np.zeros_like(terms[0], dtype=f32)
    for t in terms:
        acc = acc + f32(t)
    return acc


def fold32(gp, defect=None):
    """reflect_fold_kernel: acc += gp[ys[a]][xs[e]] for a in (y + 1, [0], [H + 1]), e likewise, from zero, in that order."""
    b, hp, wp, c = gp.shape
    h, w = hp - 2, wp - 2
    y, x = np.arange(h), np.arange(w)
    far_row = h - 1 if defect == 'fold_row' else h - 2
    ys = [(y + 1, np.ones(h, bool)), (np.zeros(h, int), y == 1), (np.full(h, h + 1), y == far_row)]
    xs = [(x + 1, np.ones(w, bool)), (np.zeros(w, int), x == 1), (np.full(w, w + 1), x == w - 2)]
    acc = np.zeros((b, h, w, c), f32)
    for ia, (yi, yok) in enumerate(ys):
        for ie, (xi, xok) in enumerate(xs):
            ok = yok[:, None] & xok[None, :]
            if defect == 'fold_corner' and ia == 1 and ie == 1:
                continue
            acc = acc + np.where(ok[None, :, :, None], gp[:, yi][:, :, xi], f32(0))
    return acc


def dgrad32(g, w, defect=None):
    b, h, wd, co = g.shape
    ci = w.shape[2]
    sc = _pow2_scale(g)
    g2 = np.pad(g, ((0, 0), (2, 2), (2, 2), (0, 0)))
    col = np.concatenate([g2[:, 2 - ky:4 - ky + h, 2 - kx:4 - kx + wd] for ky in range(3) for kx in range(3)], -1).reshape(-1, 9 * co)
    wt = np.transpose(f32(w), (0, 1, 3, 2)).reshape(9 * co, ci)
    k = 9 * co
    gp = gemm32(col, wt, sc, 1.0, False, [(0, k)], defect).reshape(b, h + 2, wd + 2, ci)
    return fold32(gp, defect)


def wgrad32(x, up, g, cout, defect=None):
    """x fp16-exact activations, g [B][H][W][ldg] (ldg = 4 for the 3-channel layer): dW [3][3][cin][cout]."""
    if up:
        x = upsample(x)
    b, h, wd, _ = g.shape
    cin = x.shape[3]
    xp = np.pad(f32(x), ((0, 0), (1, 1), (1, 1), (0, 0)), mode='reflect')
    col = np.concatenate([xp[:, ky:ky + h, kx:kx + wd] for ky in range(3) for kx in range(3)], -1).reshape(-1, 9 * cin)
    p = b * h * wd
    _, ksplit, ns, _ = wgrad_slabs(p)
    slabs = [(i * ksplit, min(p, (i + 1) * ksplit)) for i in range(ns)]
    sc = _pow2_scale(g)
    out = gemm32(np.ascontiguousarray(col.T), g.reshape(p, -1)[:, :cout], 1.0, sc, True, slabs, defect)
    return out.reshape(3, 3, cin, cout)


def bias32(g, defect=None):
    """colsum_rows_kernel + reduce_slabs_kernel."""
    c = g.shape[-1]
    rows = g.size // c
    nslab = min(rows, 256)
    per = -(-rows // nslab)
    rg = 256 // min(c, 256)
    steps = -(-per // rg)
    buf = np.zeros((nslab * per, c), f32)
    buf[:rows] = g.reshape(rows, c)
    buf = np.concatenate([buf.reshape(nslab, per, c), np.zeros((nslab, steps * rg - per, c), f32)], 1).reshape(nslab, steps, rg, c)
    grp = _seq_sum([buf[:, i] for i in range(steps)])                                  # [nslab][rg][c]
    last = rg - 1 if defect == 'bias_group' and rg > 1 else rg
    part = _seq_sum([grp[:, k] for k in range(last)])                                  # [nslab][c]
    return _seq_sum([part[k] for k in range(nslab)])


def first_dgrad32(g, fw):
    """conv_first_dgrad_kernel: per padded pixel and channel one fp32 register over tap (valid ones), then the 64 channels."""
    b, h, w, _ = g.shape
    g2 = np.pad(f32(g), ((0, 0), (2, 2), (2, 2), (0, 0)))
    acc = np.zeros((b, h + 2, w + 2, 3), f32)
    for ky in range(3):
        for kx in range(3):
            gs = g2[:, 2 - ky:4 - ky + h, 2 - kx:4 - kx + w]
            for co in range(64):
                acc = acc + gs[..., co:co + 1] * f32(fw[ky, kx, :, co])
    return acc


def emulate(st, weights, lw=LOSS_WEIGHTS, defect=None):
    """[(dW, db)] per decoder conv as the device computes them (float32), from the saved state."""
    relu = st['relu']
    enc, dec = weights['encoder'], weights['decoder'][relu]
    fw, pxw, tvw = (f32(v) for v in lw)
    x, d, fp, ft = f32(st['x']), f32(st['D']), f32(st['Fp']), f32(st['F'])
    n = len(x)
    g = f32(f32(2) * fw / f32(fp.size)) * (fp - ft)
    g = np.where(fp > 0, g, f32(0))
    for k in range(len(st['enc']) - 1, -1, -1):
        es = st['enc'][k]
        g = dgrad32(g, enc[ENC[es['i']][0]][0], defect if defect in ('fold_corner', 'fold_row') else None)
        if k > 0:
            pv = st['enc'][k - 1]
            if pv['pooled'] is not None:
                g = pool_adjoint(pool_winners(pv['out'], last=defect == 'pool_last'), g)
            g = np.where(pv['out'] > 0, g, f32(0))
        else:
            g = np.where(st['e0'] > 0, g, f32(0))
    g = fold32(first_dgrad32(g, pw.fold_first(enc)[0]), defect)
    g = g + f32(f32(2) * pxw / f32(d.size)) * (d - x)
    g = g + f32(tvw / f32(n)) * f32(tv_signs(d))
    out = [None] * len(dec)
    for k in range(len(dec) - 1, -1, -1):
        wk = f32(dec[k][0])
        cin, cout = wk.shape[2:]
        xin, up = st['dec_in'][k], st['dec_up'][k]
        if cout != 3:
            act = st['dec_out'][k]
            if defect == 'mask_below' and cin == cout and not up:
                act = xin                                                       # DEFECT: the mask of the layer below
            g = np.where(act > 0, g, f32(0))
        db = bias32(g, defect)
        if cout == 3:                                                           # pad3to4 / transpose_w(cout_pad = 4)
            leak = defect == 'pad_leak'                                         # DEFECT: the fourth channel of BOTH operands is not zero
            g = np.concatenate([g, g[..., :1] if leak else np.zeros_like(g[..., :1])], -1)
            wk = np.concatenate([wk, wk[..., :1] if leak else np.zeros_like(wk[..., :1])], -1)
        dw = wgrad32(xin, up, g, cout, defect)
        out[k] = (dw, db)
        if k > 0:
            if defect == 'tap_T':                                               # DEFECT: tap (0, 1) read as (1, 0)
                wk = wk.copy()
                wk[0, 1] = wk[1, 0]
            g = dgrad32(g, wk, defect)
            if up:
                b, h, w, c = g.shape
                q = g.reshape(b, h // 2, 2, w // 2, 2, c)
                g = (q[:, :, 0, :, 0] + q[:, :, 0, :, 1]) + (q[:, :, 1, :, 0] + (f32(0) * q[:, :, 1, :, 1] if defect == 'up_term' else q[:, :, 1, :, 1]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------
def adam_c(b1, b2, t):
    """The constant c(b1, b2, t) of  |w_dev - w_ref| <= u |w_ref| + c u S + (sqrt(t) 2^-63 / eps) S  after step t, in units of u = 2^-24,
    S = lr_t M / (sqrt(v) + eps) with M_t = b1 M_{t-1} + (1 - b1) |g_t| (the magnitude of m: m itself may cancel).

      m = b1 m + (1 - b1) g:  1 - b1 rounded (u), two products (u each), one add (u): <= 3u M per step; the carried error is
          multiplied by b1 < 1 while M only grows by the same recurrence, so after t steps <= 3 t u M.
      v = b2 v + (1 - b2) g g: 1 - b2, two products, the other product, one add: 4u per step on non-negative terms, 4 t u v after t
          steps; the square root halves it: 2 t u.  (g g underflows below |g| ~ 1e-19: at most 2^-126 absolute per step even when
          flushed, sqrt(t 2^-126) = sqrt(t) 2^-63 on the root, against eps in the denominator: the last term above.)
      sqrtf: 1 ulp = 2u.  + eps: u.  the division: 1 ulp = 2u.  lr_t * m: u.  (w - step rounds to u |w|: the first term.)
      lr_t on the host, lr * sqrtf(1 - powf(b2, t)) / (1 - powf(b1, t)): powf errs by <= 1 ulp = 2u of b^t, which 1 - b^t magnifies to
          2u b^t / (1 - b^t) (the subtraction of two floats within a factor of two is exact, otherwise u); the root halves the b2 term;
          sqrtf (u, correctly rounded on the host), the product and the division (u each).
    """
    p1, p2 = b1 ** t, b2 ** t
    lr = (2 * p2 / (1 - p2) + 1) / 2 + (2 * p1 / (1 - p1) + 1) + 3
    return 3 * t + 2 * t + 2 + 1 + 2 + 1 + lr


def adam_ref(w, g, m, v, mabs, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """One float64 Adam step from the float32 w, g and the float64 moments: (w_new, m, v, M, u |w_new|, bound of the step's error).
    The first bound is the rounding of the stored weight, which no arithmetic can halve; the CPU test halves the second alone."""
    b1, b2, eps, lr = (np.float64(f32(z)) for z in (b1, b2, eps, lr))
    w, g = np.float64(w), np.float64(g)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    mabs = b1 * mabs + (1 - b1) * np.abs(g)
    lr_t = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    den = np.sqrt(v) + eps
    wn = w - lr_t * m / den
    s = lr_t * mabs / den
    return wn, m, v, mabs, U * np.abs(wn), (adam_c(b1, b2, t) * U + np.sqrt(t) * 2.0 ** -63 / eps) * s


def adam32(w, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8, fma=False):
    """adam_kernel / apply_adam in float32; fma=True contracts every multiply-add (one rounding of the exact float64 value)."""
    w, g, m, v, b1, b2, eps, lr = (f32(z) for z in (w, g, m, v, b1, b2, eps, lr))
    lr_t = f32(lr * np.sqrt(f32(1) - f32(np.power(b2, f32(t)))) / (f32(1) - f32(np.power(b1, f32(t)))))
    one = f32(1)
    with np.errstate(under='ignore'):
        if fma:
            d = np.float64
            m = f32(d(b1) * d(m) + d(f32((one - b1) * g)))
            v = f32(d(b2) * d(v) + d(f32((one - b2) * g)) * d(g))
        else:
            m = b1 * m + (one - b1) * g
            v = b2 * v + (one - b2) * g * g
        w = w - lr_t * m / (np.sqrt(v) + eps)
    return w, m, v


def adam_gradients(seed, n):
    """Magnitudes 1e-12 .. 1e3 with both signs, exact zeros, and values below 1e-19 whose square underflows in fp32."""
    rng = np.random.default_rng(seed)
    g = 10.0 ** rng.uniform(-12, 3, n) * rng.choice([-1.0, 1.0], n)
    kind = rng.random(n)
    g[kind < 0.1] = 0
    tiny = (kind >= 0.1) & (kind < 0.2)
    g[tiny] = 10.0 ** rng.uniform(-30, -19.5, int(tiny.sum())) * rng.choice([-1.0, 1.0], int(tiny.sum()))
    return f32(g)
