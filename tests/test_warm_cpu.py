"""Video warm start, the parts that need no GPU: the ABI declarations and their bindings, the refusals of the CLI and of the
Python layer (raised before any library call), and a float64 NumPy model of rotate / solve / compose / Newton-Schulz that pins
the algebra and the orientation of V (eigenvectors in COLUMNS: A = V diag(lam) V^T, A' = V0^T A V0, V = V0 V')."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, rel_err

SMALL = ['relu3_1', 'relu2_1', 'relu1_1']
# name -> the documented argument list (include/wct_hip.h), by type
SYMBOLS = {
    'wct_warm_create': ('int', ['wct_ctx*', 'const int*', 'int', 'wct_warm**']),
    'wct_warm_free': ('void', ['wct_ctx*', 'wct_warm*']),
    'wct_warm_reset': ('int', ['wct_ctx*', 'wct_warm*']),
    'wct_warm_basis': ('int', ['wct_ctx*', 'const wct_warm*', 'int', 'int*', 'float*']),
    'wct_stylize_prepared_warm': ('int', ['wct_ctx*', 'const uint8_t*', 'int', 'int', 'const wct_style*', 'const int*', 'int', 'float',
                                          'unsigned', 'wct_warm*', 'uint8_t*']),
    'wct_stylize_prepared_batch_dev_warm': ('int', ['wct_ctx*', 'const uint8_t*', 'int', 'int', 'int', 'const wct_style*', 'const int*',
                                                    'int', 'float', 'unsigned', 'wct_warm*', 'uint8_t*']),
    'wct_transform_warm': ('int', ['wct_ctx*', 'const float*', 'int', 'const float*', 'int', 'int', 'float', 'unsigned', 'wct_warm*',
                                   'int', 'float*', 'int*']),
}


@pytest.fixture(scope='module')
def lib():
    from wct_tf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_header_declares_the_warm_symbols_with_the_documented_arguments(lib):
    from wct_tf_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wct_hip.h')).read(), flags=re.S)
    assert 'typedef struct wct_warm wct_warm;' in header
    bound = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    for name, (ret, want) in SYMBOLS.items():
        m = re.search(r'^\s*%s\s+%s\s*\(([^;]*)\)\s*;' % (ret, name), header, re.M)
        assert m, name
        got = [re.sub(r'\s*\b\w+$', '', a.strip()).replace(' *', '*') for a in m.group(1).split(',')]     # drop the parameter names
        assert got == want, (name, got)
        assert name in bound and hasattr(lib, name), name
        assert len(bound[name][1]) == len(want), name
    doc = open(os.path.join(ROOT, 'include', 'wct_hip.h')).read()
    assert doc.count('stylize_video.py:112-135') >= 3          # the behaviour the entries replace


def test_calls_refuse_a_null_context(lib):
    lv = (C.c_int * 1)(1)
    out = C.c_void_p()
    assert lib.wct_warm_create(None, lv, 1, C.byref(out)) == -2
    assert b'invalid argument' in lib.wct_last_error()
    assert lib.wct_warm_reset(None, None) == -2
    v = C.c_int()
    assert lib.wct_warm_basis(None, None, 1, C.byref(v), None) == -2
    lib.wct_warm_free(None, None)                               # a no-op
    img = np.zeros((8, 8, 3), np.uint8)
    p = img.ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.wct_stylize_prepared_warm(None, p, 8, 8, None, lv, 1, C.c_float(1), 0, None, p) == -2
    assert lib.wct_stylize_prepared_batch_dev_warm(None, None, 8, 8, 1, None, lv, 1, C.c_float(1), 0, None, None) == -2
    assert lib.wct_transform_warm(None, None, 4, None, 4, 64, C.c_float(1), 0, None, 1, None, None) == -2


@pytest.mark.parametrize('extra', [['--keep-colors'], ['--swap5'], ['--adain'], ['--mask-path', 'm.png', '--mask-styles', 'a.png']])
def test_cli_refuses_warm_start_off_the_prepared_path(extra, capsys):
    from wct_tf_amd.stylize_video import build_parser, check_warm_args
    parser = build_parser()
    base = ['--relu-targets', 'relu1_1', '--in-path', 'clip', '--out-path', 'o', '--warm-start']
    if '--mask-path' not in extra:
        base += ['--style-path', 's.png']
    with pytest.raises(SystemExit):
        check_warm_args(parser, parser.parse_args(base + extra))
    assert '--warm-start does not combine with %s' % extra[0] in capsys.readouterr().err


def test_cli_takes_warm_start_on_the_prepared_path():
    from wct_tf_amd.stylize_video import build_parser, check_warm_args
    parser = build_parser()
    args = parser.parse_args(['--relu-targets', 'relu1_1', '--in-path', 'clip', '--out-path', 'o', '--style-path', 's.png', '--warm-start',
                              '--passes', '2'])
    check_warm_args(parser, args)
    assert args.warm_start is True
    assert parser.parse_args(['--relu-targets', 'relu1_1', '--in-path', 'c', '--out-path', 'o']).warm_start is False


class _NoLibrary(object):
    """stands in for a Context: any library call through it is an error of the test"""
    h = 1

    def __getattr__(self, name):
        raise AssertionError('the library was reached: %s' % name)


def _model(ctx):
    from wct_tf_amd.wct import WCT
    model = WCT.__new__(WCT)                  # no __init__: no GPU context exists
    model.sess, model.relu_targets, model.wct_mode, model.ss_patch_size, model.ss_stride = ctx, SMALL, 'tf', 3, 1
    return model


IMG = np.zeros((16, 16, 3), np.uint8)


def test_python_refusals_come_before_the_library():
    from wct_tf_amd.context import Context, PreparedStyle, WarmState
    ctx = _NoLibrary()
    model = _model(ctx)
    h = PreparedStyle(ctx, C.c_void_p(12345), IMG, (1, 2, 3))
    w = WarmState(ctx, C.c_void_p(54321), (1, 2, 3))
    frames = np.stack([IMG] * 3)
    for call in (lambda: model.predict(IMG, IMG, warm=w), lambda: model.predict_frames(frames, IMG, warm=w)):
        with pytest.raises(ValueError, match='PreparedStyle'):       # a warm state with an image instead of a handle
            call()
    for call in (lambda: model.predict(IMG, h, adain=True, warm=w), lambda: model.predict_frames(frames, h, adain=True, warm=w)):
        with pytest.raises(ValueError, match='AdaIN'):
            call()
    with pytest.raises(ValueError, match='swap5'):
        model.predict(IMG, h, swap5=True, warm=w)
    with pytest.raises(TypeError, match='WarmState'):
        model.predict(IMG, h, warm=object())
    other = WarmState(_NoLibrary(), C.c_void_p(1), (1, 2, 3))
    with pytest.raises(ValueError, match='another context'):
        model.predict_frames(frames, h, warm=other)
    with pytest.raises(ValueError, match='relu levels'):
        model.predict(IMG, h, warm=WarmState(ctx, C.c_void_p(2), (1, 2)))
    with pytest.raises(TypeError, match='not a wct_warm pointer'):
        model.predict(IMG, h, warm=WarmState(ctx, 777, (1, 2, 3)))
    closed = WarmState(ctx, None, (1, 2, 3))
    with pytest.raises(ValueError, match='closed'):
        model.predict(IMG, h, warm=closed)
    with pytest.raises(ValueError, match='closed'):
        closed.reset()
    # the context's own entry points
    real = Context.__new__(Context)            # no __init__: no library, no GPU context
    real.h, real.lib = 1, _NoLibrary()
    wr = WarmState(real, C.c_void_p(3), (1, 2, 3))
    hr = PreparedStyle(real, C.c_void_p(4), IMG, (1, 2, 3))
    with pytest.raises(ValueError, match='AdaIN'):
        real.stylize_prepared(IMG, hr, SMALL, adain=True, warm=wr)
    with pytest.raises(ValueError, match='relu levels'):
        real.stylize_prepared_batch(frames, hr, SMALL[:2], warm=wr)
    with pytest.raises(ValueError, match='needs the level'):
        real.transform(np.zeros((4, 64), np.float32), np.zeros((4, 64), np.float32), 1.0, 0, warm=wr)
    with pytest.raises(ValueError, match='relu levels'):
        real.transform(np.zeros((4, 512), np.float32), np.zeros((4, 512), np.float32), 1.0, 0, warm=wr, level=4)
    for o in (h, w, other, wr, hr):
        o.h = None                             # (nothing to free in this test)
    real.h = None


def test_numpy_model_of_rotate_solve_compose_reproduces_the_oracle(monkeypatch):
    """float64 throughout: V0 from a perturbed copy of the content (5 % of the style's rows mixed in), stored in float32 and
    re-orthonormalised by one Newton-Schulz step; A' = V0^T A V0; eigh(A') -> (lam, V'); V = V0 V'; the whitening matrix from
    (lam, V) with wct_np's cut-off and gains.  Must give oracle.wct_np to 1e-10 -- the conventions of csrc/warm.hip.
    (oracle.wct_np rounds its result to float32, ops.py:140, which alone is 2.6e-8: the comparison takes the oracle's own float64
    result from in front of that cast, and checks that the cast of it is what the oracle returned.)"""
    import oracle
    from oracle import wct_oracle
    z = np.load(os.path.join(GOLDEN, 'wct_np_reference.npz'))
    fc, fs, alpha = np.float64(z['c64_default/content']), np.float64(z['c64_default/style']), 0.6
    seen, unflatten = [], wct_oracle._unflatten
    monkeypatch.setattr(wct_oracle, '_unflatten', lambda mat, shape: seen.append(mat) or unflatten(mat, shape))
    returned = oracle.wct_np(fc, fs, alpha)
    want = unflatten(seen[-1], fc.shape[1:])
    assert want.dtype == np.float64 and np.array_equal(np.float32(want), returned)
    assert rel_err(returned, z['c64_default/out']) < 1e-5                          # (and the oracle is the golden's reference)
    c = fc.shape[-1]
    x, s = fc.reshape(-1, c), fs.reshape(-1, c)
    xc = x - x.mean(0)
    a = xc.T @ xc / (len(x) - 1)
    pert = 0.95 * x + 0.05 * np.resize(s, x.shape)
    pc = pert - pert.mean(0)
    v0 = np.float64(np.float32(np.linalg.eigh(pc.T @ pc / (len(x) - 1))[1]))       # as a state stores it: float32
    assert np.abs(v0.T @ v0 - np.eye(c)).max() > 1e-9
    v0 = v0 @ (3 * np.eye(c) - v0.T @ v0) / 2                                      # Newton-Schulz: V (3 I - V^T V) / 2
    assert np.abs(v0.T @ v0 - np.eye(c)).max() < 1e-13
    ap = v0.T @ a @ v0                                                             # rotate
    assert np.abs(ap - np.diag(np.diag(ap))).max() < 0.2 * np.abs(a - np.diag(np.diag(a))).max()     # nearly diagonal
    lam, vp = np.linalg.eigh(ap)                                                   # solve, from the identity
    v = v0 @ vp                                                                    # compose
    assert np.abs(v.T @ a @ v - np.diag(lam)).max() < 1e-10 * lam.max()
    keep = lam > 1e-5
    tw = (v[:, keep] * (lam[keep] + 1e-5) ** -0.5) @ v[:, keep].T
    sc = s - s.mean(0)
    ws, es = np.linalg.eigh(sc.T @ sc / (len(s) - 1))
    ks = ws > 1e-5
    tcs = (es[:, ks] * np.sqrt(ws[ks] + 1e-5)) @ es[:, ks].T
    got = alpha * ((xc @ tw.T) @ tcs.T + s.mean(0)) + (1 - alpha) * xc
    assert rel_err(got.reshape(want.shape), want) < 1e-10
