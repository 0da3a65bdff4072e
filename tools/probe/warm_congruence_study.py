"""CPU study for the video warm start: which arithmetic does the congruence A' = V0^T A V0 need?

A warm solve rotates the content covariance A into the eigenvector basis V0 of an earlier, similar frame, solves A' from the
identity and composes V = V0 V'.  The congruence perturbs the eigenvalues by ~sqrt(C) eps ||A|| in float32, and the cut-off
logic of the spectral tail (kept / dropped at 1e-5) is sensitive to exactly that on graded and N << C spectra.  This script
takes the content covariances of the hard goldens (tests/golden/wct_np_hard.npz, wct_np_hard512.npz, wct_np_cross512.npz),
builds V0 from a PERTURBED copy of each (2 % and 5 % of the style sample's features mixed into the content), forms A' in

    f32     float32 products (what csrc/warm.hip runs: v_mfma_f32_32x32x2_f32, fp32 accumulation)
    f16x2   operands split into fp16 hi + lo at a power-of-two scale, hi hi + hi lo + lo hi accumulated in float32 (cov_f16x2)
    f64     float64 products, rounded to float32 at the end

and pushes each through the wct_np transform (content side from (eigenvalues of A', V = V0 V'), style side exact), scoring
rel_err against the reference output stored in the golden (the sampled rows of the digest goldens).  `cold` is the same model
with V0 = I, i.e. the path as it is.  Two readings of the content eigenvalues are scored: `trk` takes them from A' (the solver's
tracked matrix), `rfr` re-derives them as diag(V^T A V) in float32 (what launch_refresh does for graded spectra).

    python tools/probe/warm_congruence_study.py > profiles/warm_congruence_study.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.make_golden import (CROSS512_CASE, HARD512_CASES, cross512_inputs, digest_selectors,  # noqa: E402
                                hard512_inputs)

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def rel_err(a, b):
    return float(np.linalg.norm(np.float64(a) - np.float64(b)) / np.linalg.norm(np.float64(b)))


def cov32(x):
    """[N][C] float32 features -> the C x C covariance as the device holds it (float32), and the centred rows"""
    xc = np.float64(x) - np.float64(x).mean(0)
    return np.float32(xc.T @ xc / (len(x) - 1)), xc


def split16(m):
    s = 2.0 ** (14 - np.ceil(np.log2(max(np.abs(m).max(), 1e-30))))
    v = np.float32(m) * np.float32(s)
    hi = np.float32(np.float16(v))
    lo = np.float32(np.float16(v - hi))
    return hi, lo, np.float32(s)


def mm16(a, b):
    ah, al, sa = split16(a)
    bh, bl, sb = split16(b)
    return (ah @ bh + ah @ bl + al @ bh) / (sa * sb)


def congruence(a, v0, how):
    if how == 'f64':
        return np.float32(np.float64(v0).T @ np.float64(a) @ np.float64(v0))
    mm = mm16 if how == 'f16x2' else (lambda p, q: np.float32(p) @ np.float32(q))
    r = np.float32(mm(np.ascontiguousarray(v0.T), np.float32(mm(a, v0))))
    return np.float32(np.triu(r) + np.triu(r, 1).T)          # the kernel computes the tiles g <= h and mirrors


def transform(a, xc, v, lam, fs, alpha):
    """wct_np (ops.py:92-140) with the content side from (lam, v); the style side exact"""
    keep = lam > 1e-5
    tw = (np.float64(v[:, keep]) * (np.float64(lam[keep]) + 1e-5) ** -0.5) @ np.float64(v[:, keep]).T
    s = np.float64(fs)
    ms = s.mean(0)
    sc = s - ms
    ws, es = np.linalg.eigh(sc.T @ sc / (len(s) - 1))
    ks = ws > 1e-5
    tcs = (es[:, ks] * np.sqrt(ws[ks] + 1e-5)) @ es[:, ks].T
    return np.float32(alpha * ((xc @ tw.T) @ tcs.T + ms) + (1 - alpha) * xc), int(keep.sum())


def study(name, fc, fs, alpha, score):
    c = fc.shape[-1]
    x, s = fc.reshape(-1, c), fs.reshape(-1, c)
    a, xc = cov32(x)
    rows = []
    for mix in (0.0, 0.02, 0.05):
        other = np.resize(s, x.shape)                         # the other sample's features, cycled to the content's rows
        v0 = np.eye(c, dtype=np.float32) if mix == 0.0 else np.float32(np.linalg.eigh(np.float64(cov32((1 - mix) * x + mix * other)[0]))[1])
        for how in (('cold',) if mix == 0.0 else ('f32', 'f16x2', 'f64')):
            ap = a if how == 'cold' else congruence(a, v0, how)
            lam, vp = np.linalg.eigh(np.float64(ap))
            v = np.float32(np.float64(v0) @ vp)               # compose (exact solve: the study isolates the congruence)
            lam_r = np.float32(np.einsum('ij,ij->j', v, np.float32(a) @ v))
            lam64 = np.linalg.eigvalsh(np.float64(a))
            e_trk, k_trk = transform(a, xc, v, np.float32(lam), s, alpha)
            e_rfr, k_rfr = transform(a, xc, v, lam_r, s, alpha)
            rows.append((name, c, len(x), mix, how, np.abs(np.sort(lam) - lam64).max() / lam64.max(), k_trk, score(e_trk), k_rfr, score(e_rfr)))
    return rows


def main():
    out = []
    z = np.load(os.path.join(GOLDEN, 'wct_np_hard.npz'))
    for n in sorted({k.split('/')[0] for k in z.files}):
        ref = z[n + '/out']
        out += study(n, z[n + '/content'], z[n + '/style'], float(z[n + '/alpha']), lambda o, ref=ref: rel_err(o.reshape(ref.shape), ref))
    z5 = np.load(os.path.join(GOLDEN, 'wct_np_hard512.npz'))
    for case in HARD512_CASES:
        fc, fs = hard512_inputs(case)
        sel = digest_selectors(case[:7])[0]
        out += study(case[0], fc, fs, case[4], lambda o, sel=sel, ref=z5[case[0] + '/rows']: rel_err(o[sel], ref))
    zc = np.load(os.path.join(GOLDEN, 'wct_np_cross512.npz'))
    fc, fs = cross512_inputs()
    sel = digest_selectors(CROSS512_CASE)[0]
    out += study(CROSS512_CASE[0], fc, fs, CROSS512_CASE[4], lambda o: rel_err(o[sel], zc[CROSS512_CASE[0] + '/rows']))
    print('# congruence A\' = V0^T A V0 in three arithmetics, pushed through wct_np; rel_err against the golden output (budget 1e-3)')
    print('# dlam: max |eig(A\') - eig(A)| / ||A||; kept: eigenvalues above the 1e-5 cut-off; trk: eigenvalues of A\'; rfr: diag(V^T A V)')
    print('%-28s %4s %5s %5s %-6s %9s %5s %9s %5s %9s' % ('case', 'C', 'N', 'mix', 'arith', 'dlam', 'kept', 'err trk', 'kept', 'err rfr'))
    for r in out:
        print('%-28s %4d %5d %5.2f %-6s %9.2e %5d %9.2e %5d %9.2e' % r)


if __name__ == '__main__':
    main()
