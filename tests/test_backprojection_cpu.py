"""Back-projection sampling without a device: the host tables of Pillow's resize (sr3_hip.diffusion.resample_tables) against Pillow itself;
the NumPy restatements of the operator and of the step that tests/test_gpu_backprojection.py checks the kernels against; the contraction
the step relies on; the refusals of the three C-ABI entries (sr3_resample_f32, sr3_backproject_scratch_bytes, sr3_backproject_step) before
they launch anything; and the config plumbing ("backprojection" in a phase's beta_schedule block / set_backprojection).

The restatements (`oracle_resample`, `oracle_backproject_step`) are the contract of csrc/backproject.hip: fp32 operations, one rounding
each (np.float32 arithmetic), the horizontal pass first, taps ascending, the accumulator starting from +0."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from helpers import ROOT, SCHEDS, opt_for

F = np.float32
KEYS = ('a', 'b', 'c1', 'c2', 'sigma')
EPS24 = 2.0 ** -24


# ---- the oracles ------------------------------------------------------------------------------------------------------------------

def tables_2d(in_hw, out_hw, resample='bicubic'):
    """(bounds_h, weights_h, bounds_v, weights_v) of the resize in_hw = (H, W) -> out_hw = (OH, OW); horizontal = the width axis"""
    from sr3_hip.diffusion import resample_tables
    return resample_tables(in_hw[1], out_hw[1], resample) + resample_tables(in_hw[0], out_hw[0], resample)


def matrix64(bounds, weights, in_size):
    """the float64 matrix [out, in] the two tables stand for"""
    m = np.zeros((bounds.shape[0], in_size), dtype=np.float64)
    for o, (f, c) in enumerate(bounds):
        m[o, f:f + c] = weights[o, :c].astype(np.float64)
    return m


def _pass(x, bounds, weights):
    """one pass along the LAST axis: acc = +0; for t ascending: acc = acc + x[first + t] * w[t], fp32, each operation rounded on its own"""
    x = np.asarray(x, dtype=F)
    out = np.zeros(x.shape[:-1] + (bounds.shape[0],), dtype=F)
    for o, (f, c) in enumerate(bounds):
        acc = np.zeros(x.shape[:-1], dtype=F)
        for t in range(int(c)):
            acc = acc + x[..., int(f) + t] * F(weights[o, t])
        out[..., o] = acc
    assert out.dtype == F
    return out


def oracle_resample(x, tabs):
    """x [..., H, W] -> [..., OH, OW]: the horizontal pass into an fp32 intermediate, then the vertical pass"""
    bh, wh, bv, wv = tabs
    t = _pass(x, bh, wh)
    return np.ascontiguousarray(np.swapaxes(_pass(np.swapaxes(t, -1, -2), bv, wv), -1, -2))


def oracle_backproject(x0, y, down, up, lam, iters):
    """`iters` rounds of r = y - D(x0); x0 = x0 + lam * U(r) in fp32 -> (x0, [r of every round])"""
    x0, y, lam = np.asarray(x0, dtype=F), np.asarray(y, dtype=F), F(lam)
    rs = []
    for _ in range(iters):
        r = y - oracle_resample(x0, down)
        x0 = x0 + lam * oracle_resample(r, up)
        rs.append(r)
    assert x0.dtype == F
    return x0, rs


def oracle_backproject_step(x, eps, z, y, down, up, lam, iters, tabs, j, clip, hist=None):
    """One back-projected step in the kernels' operations and association.  tabs: dict of fp32 arrays a, b, c1, c2, sigma (and c3 when
    hist is given), read at row j.  -> (x', x0 after the rounds) -- the latter is hist' where there is a history"""
    x, eps = np.asarray(x, dtype=F), np.asarray(eps, dtype=F)
    a, b, c1, c2, sg = (F(tabs[k][j]) for k in KEYS)
    x0 = a * x - b * eps
    if clip:
        x0 = np.clip(x0, F(-1.0), F(1.0))
    x0, _ = oracle_backproject(x0, y, down, up, lam, iters)
    mean = c1 * x0 + c2 * x
    if hist is not None:
        mean = mean + F(tabs['c3'][j]) * np.asarray(hist, dtype=F)
    zz = np.zeros_like(x) if z is None else np.asarray(z, dtype=F)
    out = mean + zz * sg
    assert out.dtype == F
    return out, x0


# ---- the tables against Pillow -------------------------------------------------------------------------------------------------------

PIL_SHAPES = [((24, 40), (3, 5)), ((18, 30), (9, 15)), ((18, 30), (6, 10)), ((16, 16), (4, 4)), ((3, 5), (24, 40)), ((4, 4), (16, 16))]


def _pillow_rule(in_size, out_size, support):
    """(first, count) per output as ImagingResample's precompute_coeffs clips them, restated with Python floats"""
    scale = in_size / out_size
    sup = support * max(scale, 1.0)
    rows = []
    for xx in range(out_size):
        c = (xx + 0.5) * scale
        lo = max(int(c - sup + 0.5), 0)
        hi = min(int(c + sup + 0.5), in_size)
        rows.append((lo, hi - lo))
    return rows, int(np.ceil(sup)) * 2 + 1


@pytest.mark.parametrize('resample', ['bicubic', 'bilinear'])
@pytest.mark.parametrize('in_hw,out_hw', PIL_SHAPES, ids=['%dx%d-%dx%d' % (a + b) for a, b in PIL_SHAPES])
def test_tables_against_pillow(in_hw, out_hw, resample):
    """The float64 product Dv x Dh^T of the table matrices against Image.resize on a mode-F image.  Pillow accumulates a pass in double
    and rounds its result to fp32 (2^-24 relative); the tables' weights are fp32 (2^-24 relative each): per pass the difference is at
    most (n_taps + 2) 2^-24 sum|w| max|in|, and the vertical pass carries the horizontal one's through sum|w_v|."""
    from PIL import Image
    bh, wh, bv, wv = tables_2d(in_hw, out_hw, resample)
    support = 2.0 if resample == 'bicubic' else 1.0
    for b, w, i, o in ((bh, wh, in_hw[1], out_hw[1]), (bv, wv, in_hw[0], out_hw[0])):
        assert b.dtype == np.int32 and b.shape == (o, 2) and w.dtype == F and w.shape[0] == o
        rows, ksize = _pillow_rule(i, o, support)
        assert w.shape[1] == ksize and [tuple(r) for r in b.tolist()] == rows
        assert b[0, 0] == 0 and b[-1, 0] + b[-1, 1] == i and b[:, 1].min() >= 1 and b[:, 1].max() <= ksize
        assert np.all((b[:, 0] >= 0) & (b[:, 0] + b[:, 1] <= i))
        for r in range(o):
            assert np.all(w[r, b[r, 1]:] == 0)
            assert abs(float(w[r].astype(np.float64).sum()) - 1.0) <= (b[r, 1] + 1) * EPS24 * float(np.abs(w[r]).sum())
    x = np.random.default_rng(sum(in_hw) + 7 * sum(out_hw)).uniform(-1.0, 1.0, in_hw).astype(F)
    method = Image.BICUBIC if resample == 'bicubic' else Image.BILINEAR
    ref = np.asarray(Image.fromarray(x).resize((out_hw[1], out_hw[0]), method), dtype=np.float64)
    assert ref.shape == tuple(out_hw)
    got = matrix64(bv, wv, in_hw[0]) @ x.astype(np.float64) @ matrix64(bh, wh, in_hw[1]).T
    sh, sv = float(np.abs(wh).sum(axis=1).max()), float(np.abs(wv).sum(axis=1).max())
    e_h = (int(bh[:, 1].max()) + 2) * EPS24 * sh * float(np.abs(x).max())
    bound = sv * e_h + (int(bv[:, 1].max()) + 2) * EPS24 * sv * sh * float(np.abs(x).max())
    err = float(np.abs(got - ref).max())
    print('%s %s -> %s: max |tables - Pillow| = %.3e (bound %.3e)' % (resample, in_hw, out_hw, err, bound))
    assert err <= bound
    # and the fp32 restatement stays within the same bound of its own float64 matrices
    assert float(np.abs(oracle_resample(x, (bh, wh, bv, wv)).astype(np.float64) - got).max()) <= bound


def test_resample_tables_refuse_bad_arguments():
    from sr3_hip.diffusion import resample_tables
    for args, word in (((0, 4), 'in_size'), ((4, 0), 'out_size'), ((4.0, 2), 'in_size'), ((True, 2), 'in_size'), ((4, 2, 'lanczos'), 'lanczos')):
        with pytest.raises(ValueError, match=word):
            resample_tables(*args)
    b, w = resample_tables(5, 5)      # the identity geometry: the centre tap alone carries weight
    assert np.allclose(matrix64(b, w, 5), np.eye(5), atol=1e-7)


# ---- the contraction -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('resample', ['bicubic', 'bilinear'])
@pytest.mark.parametrize('lr', [(4, 4), (3, 5), (16, 16)], ids=['4x4', '3x5', '16x16'])
@pytest.mark.parametrize('s', [2, 3, 4, 8])
def test_one_iteration_contracts_the_residual(s, lr, resample):
    """r' = y - D(x0 + U r) = (I - DU) r: the map of one strength-1 round on the LR residual is I - (Dv Uv) (x) (Dh Uh).  Its 2-norm, in
    float64 from the tables, is below 1 -- and the fp32 oracle's residual shrinks by it every round, up to rounding: D(x0) carries at
    most (n_h + n_v + 4) 2^-24 sum|w_h| sum|w_v| max|x0| per LR value (the two passes' roundings), once for the residual the round
    started from and once for the one it ends with, hence the factor 2, times sqrt(values) in the 2-norm."""
    hr = (lr[0] * s, lr[1] * s)
    down, up = tables_2d(hr, lr, resample), tables_2d(lr, hr, resample)
    mh = matrix64(down[0], down[1], hr[1]) @ matrix64(up[0], up[1], lr[1])
    mv = matrix64(down[2], down[3], hr[0]) @ matrix64(up[2], up[3], lr[0])
    norm = float(np.linalg.norm(np.eye(lr[0] * lr[1]) - np.kron(mv, mh), 2))
    rho = float(np.abs(np.linalg.eigvals(np.eye(lr[0] * lr[1]) - np.kron(mv, mh))).max())
    print('s = %d, LR %s, %s: ||I - DU (x) DU||_2 = %.4f (spectral radius %.4f)' % (s, lr, resample, norm, rho))
    assert rho <= norm < 1.0
    g = np.random.default_rng(10 * s + lr[1])
    x0 = np.clip(g.standard_normal((2, 3) + hr), -1, 1).astype(F)
    y = g.uniform(-1.0, 1.0, (2, 3) + lr).astype(F)
    K = 4
    x0k, rs = oracle_backproject(x0, y, down, up, 1.0, K)
    rs.append(y - oracle_resample(x0k, down))
    sh, sv = float(np.abs(down[1]).sum(axis=1).max()), float(np.abs(down[3]).sum(axis=1).max())
    slack = 2.0 * np.sqrt(lr[0] * lr[1]) * (int(down[0][:, 1].max()) + int(down[2][:, 1].max()) + 4) * EPS24 * sh * sv * max(1.0, float(np.abs(x0k).max()))
    for b in range(2):
        for c in range(3):
            n = [float(np.linalg.norm(r[b, c].astype(np.float64))) for r in rs]
            for k in range(K):
                assert n[k + 1] <= norm * n[k] + slack, (k, n, norm, slack)
    print('   residual 2-norms of plane (0, 0): %s' % ', '.join('%.3e' % float(np.linalg.norm(r[0, 0].astype(np.float64))) for r in rs))


def test_oracle_fixed_point_passes_x0_unchanged():
    """y = D(x0): r is +0 everywhere, U(r) is +0, x0 + lam 0 is x0 bit for bit"""
    hr, lr = (16, 16), (4, 4)
    down, up = tables_2d(hr, lr), tables_2d(lr, hr)
    x0 = np.random.default_rng(3).uniform(-1, 1, (1, 2) + hr).astype(F)
    y = oracle_resample(x0, down)
    got, rs = oracle_backproject(x0, y, down, up, 1.0, 3)
    assert got.tobytes() == x0.tobytes() and all(not r.any() for r in rs)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_declared():
    from sr3_hip import lib as L
    lib = L.load()
    src = open(ROOT + '/include/sr3_mi355x.h').read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name, res, nargs in (('sr3_resample_f32', C.c_int, 17), ('sr3_backproject_scratch_bytes', C.c_size_t, 5), ('sr3_backproject_step', C.c_int, 35)):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES and L.SIGNATURES[name][0] is res and len(L.SIGNATURES[name][1]) == nargs
        decl = re.search(name + r'\s*\((.*?)\)\s*;', src, flags=re.S)
        assert decl is not None and len(decl.group(1).split(',')) == nargs, name
    assert lib.sr3_version() == 1


def _p(k):
    """a made-up, 16-byte aligned, non-NULL address: the entries below refuse before they touch memory"""
    return C.c_void_p(k << 24)


RS_NAMES = ('src', 'planes', 'height', 'width', 'dst', 'oh', 'ow', 'bh', 'wh', 'kh', 'bv', 'wv', 'kv', 'tmp', 'bh_host', 'bv_host')


def _resample_args(**kw):
    a = dict(src=_p(1), planes=6, height=8, width=12, dst=_p(2), oh=2, ow=3, bh=_p(3), wh=_p(4), kh=17, bv=_p(5), wv=_p(6), kv=17,
             tmp=_p(7), bh_host=None, bv_host=None)
    a.update(kw)
    return [a[k] for k in RS_NAMES] + [None]


def _host(rows):
    return (C.c_int * (2 * len(rows)))(*[v for r in rows for v in r])


N_SRC = 6 * 8 * 12 * 4      # bytes of the default src
RESAMPLE_REFUSALS = [
    (dict(src=None), -1, 'src'), (dict(dst=None), -1, 'dst'), (dict(tmp=None), -1, 'tmp'), (dict(bh=None), -1, 'bounds_h_dev'),
    (dict(wh=None), -1, 'weights_h_dev'), (dict(bv=None), -1, 'bounds_v_dev'), (dict(wv=None), -1, 'weights_v_dev'),
    (dict(planes=0), -1, 'planes'), (dict(height=-1), -1, 'height'), (dict(width=0), -1, 'width'), (dict(oh=0), -1, 'out_height'),
    (dict(ow=-3), -1, 'out_width'), (dict(kh=0), -1, 'ksize_h'), (dict(kv=-1), -1, 'ksize_v'),
    (dict(planes=1 << 12, height=1 << 10, width=1 << 9), -2, '2^31'), (dict(planes=1 << 11, height=1 << 10, width=4, ow=1 << 10), -2, 'tmp too large'),
    (dict(planes=1 << 11, height=4, width=4, oh=1 << 10, ow=1 << 10), -2, 'dst too large'),
    (dict(dst=_p(1)), -1, 'dst overlaps src'), (dict(dst=C.c_void_p((1 << 24) + N_SRC - 4)), -1, 'dst overlaps src'),
    (dict(tmp=_p(1)), -1, 'tmp overlaps src'), (dict(tmp=C.c_void_p((1 << 24) - 4)), -1, 'tmp overlaps src'), (dict(tmp=_p(2)), -1, 'tmp overlaps dst'),
    (dict(dst=_p(4)), -1, 'dst overlaps weights_h_dev'), (dict(tmp=_p(5)), -1, 'tmp overlaps bounds_v_dev'),
    (dict(bh_host=_host([(0, 8), (0, 12), (-1, 4)])), -1, 'bounds_h_host row 2'), (dict(bh_host=_host([(0, 8), (0, 12), (9, 4)])), -1, 'bounds_h_host row 2'),
    (dict(bh_host=_host([(0, 18), (0, 12), (8, 4)])), -1, 'bounds_h_host row 0'), (dict(bv_host=_host([(0, 8), (7, 2)])), -1, 'bounds_v_host row 1'),
    (dict(bv_host=_host([(0, 0), (4, 4)])), -1, 'bounds_v_host row 0'),
]


@pytest.mark.parametrize('case', range(len(RESAMPLE_REFUSALS)))
def test_resample_refusals_no_gpu(case):
    """every refusal of sr3_resample_f32 returns its code and names the argument, before any launch: no device is present here"""
    from sr3_hip import lib as L
    lib = L.load()
    kw, code, word = RESAMPLE_REFUSALS[case]
    assert lib.sr3_resample_f32(*_resample_args(**kw)) == code, kw
    msg = lib.sr3_last_error().decode()
    assert msg.startswith('resample') and word in msg, (kw, msg)


BP_NAMES = ('x', 'eps', 'z', 'y', 'batch', 'channels', 'height', 'width', 'scale', 'iterations', 'strength', 'dbh', 'dwh', 'dkh', 'dbv', 'dwv',
            'dkv', 'ubh', 'uwh', 'ukh', 'ubv', 'uwv', 'ukv', 'ta', 'tb', 'tc1', 'tc2', 'tsig', 'step2', 'clip', 'c3', 'hist', 'scratch', 'scratch_bytes')
BP_IMG = 2 * 3 * 8 * 12 * 4      # bytes of the default image batch


def _bp_args(**kw):
    a = dict(x=_p(1), eps=_p(2), z=None, y=_p(3), batch=2, channels=3, height=8, width=12, scale=4, iterations=2, strength=1.0,
             dbh=_p(4), dwh=_p(5), dkh=17, dbv=_p(6), dwv=_p(7), dkv=17, ubh=_p(8), uwh=_p(9), ukh=5, ubv=_p(10), uwv=_p(11), ukv=5,
             ta=_p(12), tb=_p(13), tc1=_p(14), tc2=_p(15), tsig=_p(16), step2=_p(17), clip=1, c3=None, hist=None, scratch=_p(20),
             scratch_bytes=1 << 20)
    a.update(kw)
    return [a[k] for k in BP_NAMES] + [None]


BP_REFUSALS = [
    (dict(x=None), -1, 'x_nchw'), (dict(eps=None), -1, 'eps_nchw'), (dict(y=None), -1, 'y_lr'), (dict(ta=None), -1, 'tab_a'),
    (dict(tb=None), -1, 'tab_b'), (dict(tc1=None), -1, 'tab_c1'), (dict(tc2=None), -1, 'tab_c2'), (dict(tsig=None), -1, 'tab_sigma'),
    (dict(step2=None), -1, 'step2_dev'), (dict(dbh=None), -1, 'down_bounds_h'), (dict(dwh=None), -1, 'down_weights_h'),
    (dict(dbv=None), -1, 'down_bounds_v'), (dict(dwv=None), -1, 'down_weights_v'), (dict(ubh=None), -1, 'up_bounds_h'),
    (dict(uwh=None), -1, 'up_weights_h'), (dict(ubv=None), -1, 'up_bounds_v'), (dict(uwv=None), -1, 'up_weights_v'),
    (dict(batch=0), -1, 'batch'), (dict(channels=-1), -1, 'channels'), (dict(height=0), -1, 'height'), (dict(width=-4), -1, 'width'),
    (dict(scale=1), -1, 'scale'), (dict(scale=0), -1, 'scale'), (dict(scale=-2), -1, 'scale'), (dict(scale=3), -1, 'does not divide'),
    (dict(scale=8), -1, 'does not divide'), (dict(height=6), -1, 'does not divide'),
    (dict(iterations=0), -1, 'iterations'), (dict(iterations=17), -1, 'iterations'), (dict(iterations=-1), -1, 'iterations'),
    (dict(strength=float('nan')), -1, 'strength'), (dict(strength=0.0), -1, 'strength'), (dict(strength=-0.5), -1, 'strength'),
    (dict(strength=2.0), -1, 'strength'), (dict(strength=float('inf')), -1, 'strength'),
    (dict(dkh=0), -1, 'down_ksize_h'), (dict(dkv=0), -1, 'down_ksize_v'), (dict(ukh=-1), -1, 'up_ksize_h'), (dict(ukv=0), -1, 'up_ksize_v'),
    (dict(c3=_p(18)), -1, 'c3'), (dict(hist=_p(19)), -1, 'c3'),
    (dict(c3=_p(18), hist=_p(1)), -1, 'history overlaps'), (dict(c3=_p(18), hist=_p(2)), -1, 'history overlaps'),
    (dict(c3=_p(18), hist=C.c_void_p((1 << 24) + BP_IMG - 4)), -1, 'history overlaps'),
    (dict(scratch=None), -1, 'scratch is NULL'), (dict(scratch_bytes=0), -1, 'scratch_bytes'), (dict(scratch_bytes=BP_IMG), -1, 'scratch_bytes'),
    (dict(scratch=C.c_void_p((20 << 24) + 2)), -3, 'scratch'),
    (dict(y=_p(1)), -1, 'x_nchw overlaps y_lr'), (dict(y=C.c_void_p((1 << 24) - 4)), -1, 'x_nchw overlaps y_lr'), (dict(z=_p(1)), -1, 'x_nchw overlaps z_nchw'),
    (dict(eps=_p(1)), -1, 'x_nchw overlaps eps_nchw'), (dict(scratch=_p(1)), -1, 'x_nchw overlaps scratch'), (dict(scratch=_p(2)), -1, 'scratch overlaps eps_nchw'),
    (dict(scratch=_p(3)), -1, 'scratch overlaps y_lr'), (dict(scratch=_p(9)), -1, 'scratch overlaps up_weights_h'), (dict(uwv=_p(1)), -1, 'x_nchw overlaps up_weights_v'),
    (dict(dbh=_p(1)), -1, 'x_nchw overlaps down_bounds_h'), (dict(step2=_p(1)), -1, 'x_nchw overlaps step2_dev'), (dict(ta=_p(1)), -1, 'x_nchw overlaps tab_a'),
    (dict(c3=_p(18), hist=_p(3)), -1, 'hist_nchw overlaps y_lr'), (dict(c3=_p(18), hist=_p(20)), -1, 'hist_nchw overlaps scratch'),
    (dict(step2=C.c_void_p((12 << 24) - 4)), -1, 'step2_dev overlaps tab_a'),
    (dict(batch=1 << 12, channels=2, height=1 << 9, width=1 << 9), -2, '2^31'),
]


@pytest.mark.parametrize('case', range(len(BP_REFUSALS)))
def test_backproject_step_refusals_no_gpu(case):
    """every refusal of sr3_backproject_step returns its code and names the argument, before any launch: no device is present here"""
    from sr3_hip import lib as L
    lib = L.load()
    kw, code, word = BP_REFUSALS[case]
    assert lib.sr3_backproject_step(*_bp_args(**kw)) == code, kw
    msg = lib.sr3_last_error().decode()
    assert word in msg and (msg.startswith('backproject_step') or code == -3), (kw, msg)


def test_scratch_bytes():
    from sr3_hip import lib as L
    lib = L.load()
    r4 = lambda n: (n + 3) // 4 * 4
    for B, Cc, H, W, s in ((2, 3, 8, 12, 4), (1, 3, 18, 30, 3), (16, 3, 128, 128, 8), (1, 1, 2, 2, 2), (1, 1, 6, 10, 2)):
        n = B * Cc * H * W
        assert lib.sr3_backproject_scratch_bytes(B, Cc, H, W, s) == 4 * (r4(n) + r4(n // s) + r4(n // s // s)), (B, Cc, H, W, s)
    for bad in ((0, 3, 8, 12, 4), (2, 3, 8, 12, 1), (2, 3, 8, 12, 8), (2, 3, 9, 12, 4), (1 << 12, 2, 1 << 9, 1 << 9, 2)):
        assert lib.sr3_backproject_scratch_bytes(*bad) == 0, bad


# ---- the config key and set_backprojection ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_config_key_and_set_backprojection(name):
    import model as Model
    opt = opt_for(name, gpu=False)
    m = Model.create_model(opt)
    netG = m.netG
    assert netG.backprojection is None                                     # absent key: off
    keys = set(netG.state_dict().keys())
    val = opt['model']['beta_schedule']['val']
    val['backprojection'] = {'scale': 8, 'iterations': 2, 'strength': 0.5, 'resample': 'bilinear'}
    m.set_new_noise_schedule(val, schedule_phase='val')
    assert netG.backprojection == dict(scale=8, iterations=2, strength=0.5, resample='bilinear') and netG._loop_cache == {}
    assert set(netG.state_dict().keys()) == keys
    m.set_new_noise_schedule(opt['model']['beta_schedule']['train'], schedule_phase='train')      # the other phase has no key
    assert netG.backprojection is None
    val['backprojection'] = {'scale': 4}
    m.set_new_noise_schedule(val, schedule_phase='val')
    assert netG.backprojection == dict(scale=4, iterations=1, strength=1.0, resample='bicubic')
    m.set_new_noise_schedule(opt['model']['beta_schedule']['train'], schedule_phase='train')
    val['backprojection'] = None                                           # "backprojection": null
    m.set_new_noise_schedule(val, schedule_phase='val')
    assert netG.backprojection is None
    for bad, word in (({'scale': 1}, 'scale'), ({'scale': 0}, 'scale'), ({'scale': 4.0}, 'scale'), ({'scale': True}, 'scale'),
                      ({'scale': '4'}, 'scale'), ({'strength': 0.5}, 'scale'), ({'iterations': 2}, 'scale'),
                      ({'scale': 4, 'iterations': 0}, 'iterations'), ({'scale': 4, 'iterations': 17}, 'iterations'),
                      ({'scale': 4, 'iterations': 2.0}, 'iterations'), ({'scale': 4, 'iterations': None}, 'iterations'),
                      ({'scale': 4, 'strength': 0}, 'strength'), ({'scale': 4, 'strength': 2.0}, 'strength'),
                      ({'scale': 4, 'strength': -1}, 'strength'), ({'scale': 4, 'strength': float('nan')}, 'strength'),
                      ({'scale': 4, 'strength': 'strong'}, 'strength'), ({'scale': 4, 'strength': None}, 'strength'),
                      ({'scale': 4, 'resample': 'lanczos'}, 'resample'), ({'scale': 4, 'resample': 3}, 'resample'),
                      ({'scale': 4, 'resample': None}, 'resample'), ({'scale': 4, 'block': 4}, 'block'), ({'scale': 4, 'iters': 2}, 'iters')):
        with pytest.raises(ValueError, match=word) as e:
            netG.set_new_noise_schedule(dict(SCHEDS[name], backprojection=bad), torch.device('cpu'))
        assert repr(list(bad.values())[-1]) in str(e.value) or 'required' in str(e.value) or 'unknown key' in str(e.value)
        assert netG.backprojection is None
    with pytest.raises(ValueError, match='dict'):
        netG.set_new_noise_schedule(dict(SCHEDS[name], backprojection=4), torch.device('cpu'))
    # programmatic form
    netG._loop_cache['stale'] = object()
    netG.set_backprojection(2, 3, 1.5, 'bilinear')
    assert netG.backprojection == dict(scale=2, iterations=3, strength=1.5, resample='bilinear') and netG._loop_cache == {}
    for args in ((1,), (4, 0), (4, 1, 2.0), (4, 1, 0.0), (4, 1, 1.0, 'nearest')):
        with pytest.raises(ValueError):
            netG.set_backprojection(*args)
    assert netG.backprojection == dict(scale=2, iterations=3, strength=1.5, resample='bilinear')
    netG._loop_cache['stale'] = object()
    netG.set_backprojection(None)
    assert netG.backprojection is None and netG._loop_cache == {}
    with pytest.raises(ValueError, match='back-projection is off'):
        netG.p_sample_loop((1, 3, 16, 16), backprojection_target=torch.zeros(1, 3, 4, 4))


def test_backprojection_with_tiling_consistency_or_guidance_is_not_implemented():
    import model as Model
    s = SCHEDS['sr3_tiny']
    cpu = torch.device('cpu')
    netG = Model.create_model(opt_for('sr3_tiny', gpu=False)).netG
    others = dict(tiling=({'tile': 16, 'overlap': 4}, lambda: netG.set_tiling(16, 4), lambda: netG.set_tiling(None), 'tiling'),
                  consistency=({'block': 4}, lambda: netG.set_consistency(4), lambda: netG.set_consistency(None), 'consistency'),
                  guidance=({'scale': 1.5}, lambda: netG.set_guidance(1.5), lambda: netG.set_guidance(None), 'guidance'))
    for word, (spec, on, off, attr) in others.items():
        match = 'back-projection with ' + word
        with pytest.raises(NotImplementedError, match=match):
            netG.set_new_noise_schedule(dict(s, backprojection={'scale': 4}, **{word: spec}), cpu)
        netG.set_new_noise_schedule(dict(s), cpu)
        on()                                                  # the other one first
        kept = getattr(netG, attr)
        netG._loop_cache['kept'] = 1
        with pytest.raises(NotImplementedError, match=match):
            netG.set_backprojection(4)
        assert netG.backprojection is None and getattr(netG, attr) == kept and 'kept' in netG._loop_cache
        off()
        netG.set_backprojection(4, 2)                         # back-projection first
        with pytest.raises(NotImplementedError, match=match):
            on()
        assert getattr(netG, attr) is None and netG.backprojection == dict(scale=4, iterations=2, strength=1.0, resample='bicubic')
        netG.set_backprojection(None)
    netG.set_backprojection(4)
    with pytest.raises(NotImplementedError, match='back-projection with tiling'):      # the explicit tiled loop, whatever set_tiling says
        netG.p_sample_loop_tiled(torch.zeros(1, 3, 32, 32), tile=16, overlap=4)
    # a sampler and back-projection go together on the SR3 variant, in both orders
    netG.set_sampler(4, kind='dpmpp_2m')
    assert netG.sampler['steps'] == 4 and netG.backprojection is not None
    netG.set_new_noise_schedule(dict(s, sampler={'type': 'ddim', 'steps': 4}, backprojection={'scale': 2}), cpu)
    assert netG.sampler['steps'] == 4 and netG.backprojection['scale'] == 2
    # the existing refusals keep their texts with the key present elsewhere
    with pytest.raises(NotImplementedError, match='guidance with consistency'):
        netG.set_new_noise_schedule(dict(s, consistency={'block': 4}, guidance={'scale': 1.5}, backprojection={'scale': 4}), cpu)


def test_ddpm_backprojection_under_a_sampler_is_not_implemented():
    import model as Model
    s = SCHEDS['ddpm_tiny']
    netG = Model.create_model(opt_for('ddpm_tiny', gpu=False)).netG
    with pytest.raises(NotImplementedError, match='back-projection.*t_map'):
        netG.set_new_noise_schedule(dict(s, sampler={'type': 'ddim', 'steps': 3}, backprojection={'scale': 4}), torch.device('cpu'))
    netG.set_new_noise_schedule(dict(s), torch.device('cpu'))
    netG.set_sampler(3, 0.0)
    with pytest.raises(NotImplementedError, match='back-projection.*t_map'):
        netG.set_backprojection(4)
    assert netG.backprojection is None
    netG.set_sampler(None)
    netG.set_backprojection(4)
    with pytest.raises(NotImplementedError, match='back-projection.*t_map'):
        netG.set_sampler(3, 0.0)
    assert netG.sampler is None and netG.backprojection['scale'] == 4
    with pytest.raises(NotImplementedError, match='back-projection.*t_map'):
        netG.set_sampler(3, kind='dpmpp_2m')


@pytest.mark.parametrize('name', ['ddpm_tiny', 'sr3_uncond'])
def test_unconditional_backprojection_needs_a_target(name):
    """an unconditional model has no conditioning image to down-sample: the chain is refused unless the caller brings the target (the
    refusal comes before anything touches a device)"""
    import model as Model
    netG = Model.create_model(opt_for(name, gpu=False)).netG
    netG.set_backprojection(4)
    with pytest.raises(NotImplementedError, match='backprojection_target'):
        netG.p_sample_loop((1, 3, 16, 16))
    with pytest.raises(NotImplementedError, match='backprojection_target'):
        netG.sample(1)
    netG.set_backprojection(None)
    from sr3_hip import lib as L
    with pytest.raises(L.Sr3Error):          # off again: today's refusal of a CPU model
        netG.p_sample_loop((1, 3, 16, 16))


def test_validation_hands_the_batch_lr_image_over():
    """DDPM.test: data['LR'] of shape [B, C, H / s, W / s] is the chain's target under the key; anything else means the default"""
    import model as Model
    m = Model.create_model(opt_for('sr3_tiny', gpu=False))
    seen = []
    m.netG.super_resolution = lambda x, continous=False, **kw: seen.append(kw) or x
    sr, lr = torch.zeros(2, 3, 16, 16), torch.ones(2, 3, 4, 4)
    m.data = {'SR': sr, 'LR': lr}
    m.test()
    assert seen[-1] == {}                                      # key off: the call of before, no keyword
    m.netG.set_backprojection(4)
    m.test()
    assert seen[-1]['backprojection_target'] is lr
    m.data = {'SR': sr, 'LR': torch.ones(2, 3, 16, 16)}      # (an 'LR' that is the up-sampled image itself: not a target)
    m.test()
    assert seen[-1] == {}
    m.data = {'SR': sr}
    m.test()
    assert seen[-1] == {}
