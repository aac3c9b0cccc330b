"""Back-projection sampling on the GPU (csrc/backproject.hip, EngineDiffusion.set_backprojection): sr3_resample_f32 and
sr3_backproject_step through the C ABI against the NumPy restatements of tests/test_backprojection_cpu.py (fp32 operations, one rounding
each, horizontal pass first, taps ascending), and the chains of p_sample_loop under the "backprojection" key against a loop written here
from denoise_fn forwards plus that restatement.

Shapes: the smallest that take each path -- one plane of 8 x 8; 16 x 16 -> 4 x 4 (every kernel in its 16-byte form); 24 x 40 -> 3 x 5 (33
taps with clipped borders, an LR width that is no multiple of 4 under a 16-byte image, six workgroups); 18 x 30 by 3 and by 2 (widths
that are no multiple of 4: the one-element form everywhere); the two up-samples; and one case with every tensor off a 16-byte boundary.

Only back-projected states are captured here (their warm-up takes no stream out of torch's pool, EngineDiffusion._capture); the key-less
chains these tests compare with run eagerly, so the file leaves the pool -- and the hardware queue of every stream a later test
creates -- as it found it."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util as G                                                                      # noqa: E402
from helpers import load_golden, opt_for                                                  # noqa: E402
from sr3_hip import lib as L                                                              # noqa: E402
from test_backprojection_cpu import F, KEYS, oracle_backproject_step, oracle_resample, tables_2d      # noqa: E402

GUARD = 1024      # floats of NaN around a tensor, in the same allocation

# four rows that differ; row 2 is the a = 0.9, b = 0.43 row the step tests run at; |c1|, |c2|, |c3|, |sigma| <= 1
TABLES = dict(a=[1.1, 0.7, 0.9, 0.6], b=[0.2, 0.75, 0.43, 0.7], c1=[1.0, 0.45, 0.55, 0.4], c2=[0.0, 0.5, 0.45, -0.2],
              sigma=[0.0, 0.4, 0.5, 0.25], c3=[0.0, -0.35, 0.5, -0.45])
J = 2


def _tabs():
    return {k: np.asarray(v, dtype=F) for k, v in TABLES.items()}


def _dev(t, d, mis=0):
    """`t` (numpy or torch, fp32) on the device with GUARD NaNs in front of and behind it in ONE allocation, `mis` floats off a 16-byte
    boundary: (view, whole buffer, offset)"""
    t = torch.as_tensor(t)
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), float('nan'), device=d)
    off = GUARD + mis
    assert buf.data_ptr() % 16 == 0
    buf[off:off + n].copy_(t.reshape(-1))
    return buf[off:off + n].view(t.shape), buf, off


def _guard_intact(buf, off, n):
    return bool(torch.isnan(buf[:off]).all()) and bool(torch.isnan(buf[off + n:]).all())


def _check(got, want, what):
    """|got - oracle| <= 4 * 2^-23 * max(1, |oracle|) per element (the project's gate for a step's tail); equality is what is expected"""
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    tol = 4.0 * 2.0 ** -23 * np.maximum(1.0, np.abs(want.astype(np.float64)))
    print('%s: max |diff| %.3e, %.4f %% of the elements differ' % (what, diff.max(), 100.0 * float((got != want).mean())))
    assert np.all(diff <= tol), '%s: %g' % (what, diff.max())


def _dev_tables(tabs, d):
    return [torch.from_numpy(np.ascontiguousarray(t)).to(d) for t in tabs]


# ---- 1. the operator ---------------------------------------------------------------------------------------------------------------

# (planes, (H, W), (OH, OW), misaligned)
RS_SHAPES = [(1, (8, 8), (4, 4), False), (6, (16, 16), (4, 4), False), (6, (24, 40), (3, 5), False), (3, (18, 30), (6, 10), False),
             (2, (18, 30), (9, 15), False), (6, (3, 5), (24, 40), False), (6, (4, 4), (16, 16), False), (6, (16, 16), (4, 4), True)]
RS_IDS = ['%dx%dx%d-%dx%d%s' % ((p,) + a + b + ('-misaligned' if m else '',)) for p, a, b, m in RS_SHAPES]


def _resample(x, in_hw, out_hw, tabs, d, mis=False, host=(None, None)):
    """one call on guarded buffers -> (dst on the host, (dst, tmp) guards intact, rc)"""
    planes = x.shape[0]
    xd = _dev(x, d, 1 if mis else 0)[0]
    dst, dbuf, do = _dev(np.full((planes,) + tuple(out_hw), np.nan, dtype=F), d, 2 if mis else 0)
    tmp, tbuf, to = _dev(np.full((planes, in_hw[0], out_hw[1]), np.nan, dtype=F), d, 3 if mis else 0)
    bh, wh, bv, wv = _dev_tables(tabs, d)
    rc = L.load().sr3_resample_f32(L.ptr(xd), planes, in_hw[0], in_hw[1], L.ptr(dst), out_hw[0], out_hw[1], L.ptr(bh), L.ptr(wh), wh.shape[1],
                                   L.ptr(bv), L.ptr(wv), wv.shape[1], L.ptr(tmp), host[0], host[1], G.stream())
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), torch.from_numpy(x))
    return dst.cpu().numpy(), _guard_intact(dbuf, do, dst.numel()) and _guard_intact(tbuf, to, tmp.numel()), rc


@pytest.mark.parametrize('resample', ['bicubic', 'bilinear'])
@pytest.mark.parametrize('case', RS_SHAPES, ids=RS_IDS)
def test_resample_against_oracle(case, resample):
    planes, in_hw, out_hw, mis = case
    d = G.dev()
    tabs = tables_2d(in_hw, out_hw, resample)
    x = (2.0 * np.random.default_rng(planes + sum(in_hw) + sum(out_hw)).standard_normal((planes,) + in_hw)).astype(F)
    import ctypes as C
    host = tuple((C.c_int * t.size)(*t.reshape(-1).tolist()) for t in (tabs[0], tabs[2]))      # the host copies pass the entry's check
    got, intact, rc = _resample(x, in_hw, out_hw, tabs, d, mis, host)
    assert rc == 0, L.load().sr3_last_error()
    assert intact, 'a kernel wrote outside dst or tmp'
    want = oracle_resample(x, tabs)
    _check(got, want, '%s %s %s -> %s' % (resample, planes, in_hw, out_hw))
    again, intact, rc = _resample(x, in_hw, out_hw, tabs, d, mis)
    assert rc == 0 and intact and again.tobytes() == got.tobytes()      # two runs, the same bits
    if not mis:      # the public helper is the same call
        from sr3_hip.diffusion import resample_f32
        out = resample_f32(torch.from_numpy(x[None]).to(d), out_hw, resample)
        assert out.cpu().numpy()[0].tobytes() == got.tobytes()


@pytest.mark.parametrize('case', [RS_SHAPES[2], RS_SHAPES[5], RS_SHAPES[7]], ids=[RS_IDS[2], RS_IDS[5], RS_IDS[7]])
def test_out_of_range_bounds_stay_inside(case):
    """first taps and counts far outside the source: the device clamps first into [0, in] and count into [0, min(ksize, in - first)],
    so the result is the oracle's on the clamped table and nothing outside dst and tmp is written"""
    planes, in_hw, out_hw, mis = case
    d = G.dev()
    tabs = [t.copy() for t in tables_2d(in_hw, out_hw)]
    x = np.random.default_rng(5).standard_normal((planes,) + in_hw).astype(F)
    for b, n_in, ks in ((tabs[0], in_hw[1], tabs[1].shape[1]), (tabs[2], in_hw[0], tabs[3].shape[1])):
        wild = [(-5, 1000), (n_in + 3, 4), (n_in - 1, 1 << 30), (1, -2), (-(1 << 30), 1 << 30)]
        for o in range(b.shape[0]):
            b[o] = wild[o % len(wild)]
    got, intact, rc = _resample(x, in_hw, out_hw, tabs, d, mis)
    assert rc == 0 and intact, 'a kernel wrote outside dst or tmp'
    clamped = [t.copy() for t in tabs]
    for b, n_in, ks in ((clamped[0], in_hw[1], tabs[1].shape[1]), (clamped[2], in_hw[0], tabs[3].shape[1])):
        for o in range(b.shape[0]):
            f = min(max(int(b[o, 0]), 0), n_in)
            b[o] = (f, min(max(int(b[o, 1]), 0), min(ks, n_in - f)))
    _check(got, oracle_resample(x, clamped), 'clamped tables %s -> %s' % (in_hw, out_hw))
    # ... and the entry refuses the same table when it is handed the host copy
    import ctypes as C
    host = (C.c_int * tabs[0].size)(*tabs[0].reshape(-1).tolist())
    _, intact, rc = _resample(x, in_hw, out_hw, tabs, d, mis, (host, None))
    assert rc == -1 and b'bounds_h_host row 0' in L.load().sr3_last_error()


def test_resample_refusals_launch_nothing():
    d = G.dev()
    planes, in_hw, out_hw, _ = RS_SHAPES[1]
    tabs = tables_2d(in_hw, out_hw)
    bh, wh, bv, wv = _dev_tables(tabs, d)
    x = torch.randn((planes,) + in_hw, device=d)
    dst = torch.full((planes,) + out_hw, 7.0, device=d)
    tmp = torch.full((planes, in_hw[0], out_hw[1]), 7.0, device=d)
    lib = L.load()

    def call(**kw):
        a = dict(src=x, dst=dst, tmp=tmp, planes=planes, kh=wh.shape[1], kv=wv.shape[1], bh=bh)
        a.update(kw)
        rc = lib.sr3_resample_f32(L.ptr(a['src']), a['planes'], in_hw[0], in_hw[1], L.ptr(a['dst']), out_hw[0], out_hw[1], L.ptr(a['bh']), L.ptr(wh),
                                  a['kh'], L.ptr(bv), L.ptr(wv), a['kv'], L.ptr(a['tmp']), None, None, G.stream())
        torch.cuda.synchronize()
        return rc
    for kw, code, word in ((dict(src=None), -1, b'src'), (dict(bh=None), -1, b'bounds_h_dev'), (dict(planes=0), -1, b'planes'), (dict(kh=0), -1, b'ksize_h'),
                           (dict(kv=-1), -1, b'ksize_v'), (dict(dst=x), -1, b'dst overlaps src'), (dict(tmp=x), -1, b'tmp overlaps src'),
                           (dict(tmp=dst), -1, b'tmp overlaps dst'), (dict(dst=wh), -1, b'dst overlaps weights_h_dev')):
        assert call(**kw) == code, kw
        assert word in lib.sr3_last_error()
    assert bool((dst == 7.0).all()) and bool((tmp == 7.0).all())
    assert call() == 0 and not bool((dst == 7.0).any())


# ---- 2. the step against the oracle ----------------------------------------------------------------------------------------------------

# ((B, C, H, W), scale, resample, misaligned)
STEP_SHAPES = [((1, 1, 8, 8), 2, 'bicubic', False), ((2, 3, 16, 16), 4, 'bicubic', False), ((2, 3, 24, 40), 8, 'bicubic', False),
               ((1, 3, 18, 30), 3, 'bilinear', False), ((1, 2, 18, 30), 2, 'bicubic', False), ((2, 3, 16, 16), 4, 'bicubic', True)]
STEP_IDS = ['%s-s%d-%s%s' % ('x'.join(map(str, s)), sc, rs, '-misaligned' if m else '') for s, sc, rs, m in STEP_SHAPES]


@functools.lru_cache(maxsize=None)
def _geometry(shape, s, resample):
    H, W = shape[2:]
    return tables_2d((H, W), (H // s, W // s), resample), tables_2d((H // s, W // s), (H, W), resample)


@functools.lru_cache(maxsize=None)
def _inputs(shape, s, scale=1.0):
    g = np.random.default_rng(1000 * s + sum(shape))
    B, Cc, H, W = shape
    x = (scale * g.standard_normal(shape)).astype(F)
    eps, z, h = (g.standard_normal(shape).astype(F) for _ in range(3))
    y = g.uniform(-1.0, 1.0, (B, Cc, H // s, W // s)).astype(F)
    return x, eps, z, h, y


def _run(case, d, clip, with_hist, with_z, lam, iters, inputs, j=J):
    """one call on guarded (and, for the misaligned case, shifted) copies of the inputs -> (x', hist' or None, counter) on the host"""
    shape, s, resample, mis = case
    down, up = _geometry(shape, s, resample)
    x, eps, z, h, y = inputs
    dt = {k: torch.from_numpy(v).to(d) for k, v in _tabs().items()}
    xd, xbuf, xo = _dev(x, d, 1 if mis else 0)
    ed = _dev(eps, d, 2 if mis else 0)[0]
    zd = _dev(z, d, 3 if mis else 0)[0] if with_z else None
    hd, hbuf, ho = _dev(h, d, 1 if mis else 0) if with_hist else (None, None, 0)
    yd = _dev(y, d, 1 if mis else 0)[0]
    B, Cc, H, W = shape
    nb = int(L.load().sr3_backproject_scratch_bytes(B, Cc, H, W, s))
    assert nb > 0 and nb % 4 == 0
    sd, sbuf, so = _dev(np.full((nb // 4,), np.nan, dtype=F), d, 1 if mis else 0)
    step2 = torch.tensor([-7, j], dtype=torch.int32, device=d)
    axes = []
    keep = []
    for tb in (down, up):
        t = _dev_tables(tb, d)
        keep.append(t)
        axes += [L.ptr(t[0]), L.ptr(t[1]), t[1].shape[1], L.ptr(t[2]), L.ptr(t[3]), t[3].shape[1]]
    rc = L.load().sr3_backproject_step(L.ptr(xd), L.ptr(ed), L.ptr(zd), L.ptr(yd), B, Cc, H, W, s, iters, lam, *axes,
                                       *[L.ptr(dt[k]) for k in KEYS], L.ptr(step2), clip, L.ptr(dt['c3'] if with_hist else None), L.ptr(hd),
                                       L.ptr(sd), nb, G.stream())
    torch.cuda.synchronize()
    assert rc == 0, L.load().sr3_last_error()
    assert _guard_intact(xbuf, xo, xd.numel()), 'a kernel wrote outside x'
    assert hbuf is None or _guard_intact(hbuf, ho, hd.numel()), 'a kernel wrote outside hist'
    assert _guard_intact(sbuf, so, sd.numel()), 'a kernel wrote outside the scratch'
    assert torch.equal(ed.cpu(), torch.from_numpy(eps)) and torch.equal(yd.cpu(), torch.from_numpy(y))
    return xd.cpu().numpy(), None if hd is None else hd.cpu().numpy(), step2.tolist()


@pytest.mark.parametrize('case', STEP_SHAPES, ids=STEP_IDS)
def test_backproject_step_against_oracle(case):
    shape, s, resample, mis = case
    d = G.dev()
    down, up = _geometry(shape, s, resample)
    inputs = _inputs(shape, s)
    x, eps, z, h, y = inputs
    tabs = _tabs()
    worst = 0.0
    for clip in (0, 1):
        for hi in (False, True):
            for wz in (False, True):
                for lam in (1.0, 0.5):
                    for K in (1, 3):
                        gx, gh, step2 = _run(case, d, clip, hi, wz, lam, K, inputs)
                        assert step2 == [J, J - 1]
                        wx, wx0 = oracle_backproject_step(x, eps, z if wz else None, y, down, up, lam, K, tabs, J, clip, h if hi else None)
                        what = '%s s %d clip %d hist %d z %d strength %g K %d' % (shape, s, clip, hi, wz, lam, K)
                        _check(gx, wx, what + ': x')
                        worst = max(worst, float(np.abs(gx.astype(np.float64) - wx).max()))
                        if hi:
                            _check(gh, wx0, what + ': hist')
    print('%s: measured maximum |kernel - oracle| over the cross: %.3e' % (STEP_IDS[STEP_SHAPES.index(case)], worst))
    # the tables are read at row j, not j - 1: the neighbouring row gives something else entirely
    other = oracle_backproject_step(x, eps, z, y, down, up, 1.0, 1, tabs, J - 1, 1, h)[0]
    assert np.abs(_run(case, d, 1, True, True, 1.0, 1, inputs)[0] - other).max() > 0.1
    for j in (0, 3):      # the first and the last row
        gx, gh, step2 = _run(case, d, 1, True, True, 1.0, 3, inputs, j=j)
        assert step2 == [j, j - 1]
        wx, wx0 = oracle_backproject_step(x, eps, z, y, down, up, 1.0, 3, tabs, j, 1, h)
        _check(gx, wx, 'row %d: x' % j)
        _check(gh, wx0, 'row %d: hist' % j)
    a = _run(case, d, 1, True, True, 0.5, 3, inputs)      # two runs, the same bits
    b = _run(case, d, 1, True, True, 0.5, 3, inputs)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize('clip', [0, 1])
def test_backproject_step_heavy_tailed(clip):
    """x scaled by 3: with the clamp most of x0 sits at +-1, without it |x0| reaches 10"""
    case = STEP_SHAPES[2]
    shape, s, resample, _ = case
    down, up = _geometry(shape, s, resample)
    inputs = _inputs(shape, s, 3.0)
    x, eps, z, h, y = inputs
    for lam, K in ((1.0, 3), (0.5, 1)):
        gx, gh, _ = _run(case, G.dev(), clip, True, True, lam, K, inputs)
        wx, wx0 = oracle_backproject_step(x, eps, z, y, down, up, lam, K, _tabs(), J, clip, h)
        _check(gx, wx, 'heavy-tailed clip %d strength %g K %d: x' % (clip, lam, K))
        _check(gh, wx0, 'heavy-tailed clip %d strength %g K %d: hist' % (clip, lam, K))
    if clip:
        x0 = np.clip(F(0.9) * x - F(0.43) * eps, -1, 1)
        assert 0.3 < float((np.abs(x0) == 1).mean()) < 0.9


@pytest.mark.parametrize('case', STEP_SHAPES, ids=STEP_IDS)
def test_fixed_point_passes_x0_unchanged(case):
    """y = D(x0), D by the same kernels: every round's residual is +0, U of it is +0, and the history the step leaves is x0 bit for bit"""
    from sr3_hip.diffusion import resample_f32
    shape, s, resample, mis = case
    d = G.dev()
    x, eps, z, h, _ = _inputs(shape, s)
    x0 = np.clip(F(TABLES['a'][J]) * x - F(TABLES['b'][J]) * eps, F(-1), F(1))
    y = resample_f32(torch.from_numpy(x0).to(d), (shape[2] // s, shape[3] // s), resample).cpu().numpy()
    gx, gh, _ = _run(case, d, 1, True, True, 1.0, 3, (x, eps, z, h, y))
    assert gh.tobytes() == x0.tobytes()
    t = _tabs()
    want = (t['c1'][J] * x0 + t['c2'][J] * x + t['c3'][J] * h) + z * t['sigma'][J]
    assert gx.tobytes() == want.astype(F).tobytes()


def test_step_refusals_launch_nothing():
    d = G.dev()
    case = STEP_SHAPES[1]
    shape, s, resample, _ = case
    down, up = _geometry(shape, s, resample)
    x, eps, z, h, y = (torch.from_numpy(t).to(d) for t in _inputs(shape, s))
    dt = {k: torch.from_numpy(v).to(d) for k, v in _tabs().items()}
    B, Cc, H, W = shape
    lib = L.load()
    nb = int(lib.sr3_backproject_scratch_bytes(B, Cc, H, W, s))
    scratch = torch.full((nb // 4,), 7.0, device=d)
    td, tu = _dev_tables(down, d), _dev_tables(up, d)
    keep = x.clone()
    step2 = torch.tensor([-7, J], dtype=torch.int32, device=d)
    for kw, code, word in ((dict(s=3), -1, b'does not divide'), (dict(s=1), -1, b'scale'), (dict(K=0), -1, b'iterations'), (dict(K=17), -1, b'iterations'),
                           (dict(lam=0.0), -1, b'strength'), (dict(lam=2.0), -1, b'strength'), (dict(lam=float('nan')), -1, b'strength'),
                           (dict(hist=x), -1, b'overlaps'), (dict(c3=None), -1, b'c3'), (dict(y=x), -1, b'x_nchw overlaps y_lr'),
                           (dict(scratch=None), -1, b'scratch is NULL'), (dict(nb=nb - 4), -1, b'scratch_bytes'), (dict(scratch=eps), -1, b'overlaps'),
                           (dict(scratch=h), -1, b'overlaps')):
        a = dict(s=s, K=2, lam=1.0, c3=dt['c3'], hist=h, y=y, scratch=scratch, nb=nb)
        a.update(kw)
        axes = []
        for t in (td, tu):
            axes += [L.ptr(t[0]), L.ptr(t[1]), t[1].shape[1], L.ptr(t[2]), L.ptr(t[3]), t[3].shape[1]]
        rc = lib.sr3_backproject_step(L.ptr(x), L.ptr(eps), L.ptr(z), L.ptr(a['y']), B, Cc, H, W, a['s'], a['K'], a['lam'], *axes,
                                      *[L.ptr(dt[k]) for k in KEYS], L.ptr(step2), 1, L.ptr(a['c3']), L.ptr(a['hist']), L.ptr(a['scratch']),
                                      a['nb'], G.stream())
        torch.cuda.synchronize()
        assert rc == code, kw
        assert word in lib.sr3_last_error(), (kw, lib.sr3_last_error())
    assert torch.equal(x, keep) and step2.tolist() == [-7, J] and bool((scratch == 7.0).all())


# ---- 3. the chains ---------------------------------------------------------------------------------------------------------------------------

def _model(backprojection, sampler=None):
    import model as Model
    opt = opt_for('sr3_tiny', phase='val', gpu=True)
    val = opt['model']['beta_schedule']['val']
    if backprojection is not None:
        val['backprojection'] = backprojection
    if sampler is not None:
        val['sampler'] = sampler
    m = Model.create_model(opt)
    g, sd = load_golden('sr3_tiny')
    m.netG.load_state_dict(sd, strict=True)
    m.netG.show_progress = False
    m.set_new_noise_schedule(val, schedule_phase='val')
    return m.netG, g


def _rule_tables(netG):
    """the rule's tables on the host, as the engine's own _step_rule hands them to the kernel: (dict of fp32 arrays, level table)"""
    tables, level, t_map, c3, noisy = netG._step_rule()
    tabs = {k: t.cpu().numpy() for k, t in zip(KEYS, tables)}
    if c3 is not None:
        tabs['c3'] = c3.cpu().numpy()
    return tabs, level.cpu().numpy(), c3 is not None, noisy


def _own_loop_check(netG, cond, x_T, zs, out, y):
    """The chain again, written here: per step one denoise_fn forward at the step's level on the ENGINE's image before the step (its
    previous snapshot: teacher forcing, so the per-step tolerance applies to every step) and the oracle tail; the history is carried
    by the oracle.  Every step of these chains is a snapshot (T = 8 or S = 5: stride 1)."""
    d = cond.device
    bp = netG.backprojection
    tabs, level, multistep, noisy = _rule_tables(netG)
    T = len(tabs['a'])
    B = cond.shape[0]
    assert out.shape[0] == B * (T + 1)
    down, up = _geometry(tuple(x_T.shape), bp['scale'], bp['resample'])
    hist = np.zeros(tuple(x_T.shape), dtype=F) if multistep else None
    for k, j in enumerate(reversed(range(T))):
        before = x_T if k == 0 else out[k * B:(k + 1) * B]
        lv = torch.full((B,), float(level[j + 1]), dtype=torch.float32, device=d)
        eps = netG.denoise_fn(before.contiguous(), lv, cond=cond).cpu().numpy()
        z = zs[j].cpu().numpy() if (noisy and zs is not None and j > 0) else None
        want, x0 = oracle_backproject_step(before.cpu().numpy(), eps, z, y, down, up, bp['strength'], bp['iterations'], tabs, j, 1, hist)
        hist = x0 if multistep else None
        got = out[(k + 1) * B:(k + 2) * B].cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - want).max())
        tol = 2e-5 * max(1.0, float(np.abs(want).max()))
        print('step index %d: max abs err %.3e (tolerance %.3e)' % (j, err, tol))
        assert err <= tol, (j, err, tol)


CHAINS = [('ancestral', 4, 'bicubic', 2, 1.0), ('ddim', 4, 'bicubic', 1, 1.0), ('dpmpp_2m', 4, 'bicubic', 2, 1.0), ('ddim', 2, 'bicubic', 3, 1.0)]


@pytest.mark.parametrize('rule,s,resample,K,lam', CHAINS, ids=['%s-s%d-%s-K%d-l%g' % c for c in CHAINS])
def test_chain_against_own_loop_graph_and_lr_error(rule, s, resample, K, lam):
    from sr3_hip.diffusion import backprojection_error, resample_f32
    d = G.dev()
    sampler = None if rule == 'ancestral' else {'type': rule, 'steps': 5}
    spec = {'scale': s, 'iterations': K, 'strength': lam, 'resample': resample}
    netG, g = _model(spec, sampler)
    assert netG.backprojection == spec
    cond, x_T, zs = (torch.from_numpy(g['loop/' + n]).to(d) for n in ('sr', 'x_T', 'zs'))
    B = cond.shape[0]
    y = resample_f32(cond, (16 // s, 16 // s), resample)      # the default target: the conditioning image down-sampled
    # eager; the ancestral rule with its noise injected
    netG.use_graph = False
    eager = netG.p_sample_loop(cond, continous=True, x_T=x_T, noise_seq=zs if rule == 'ancestral' else None).clone()
    key, st = next(reversed(netG._loop_cache.items()))
    assert st['backprojection'] == spec and tuple(st['y_lr'].shape) == (B, 3, 16 // s, 16 // s) and torch.equal(st['y_lr'], y)
    assert key[-4] == (s, K, lam, resample) and key[-3] is None and key[-2] is None and key[-1] is None and len(key) == 13
    assert st['step'].tolist() == [0, -1]
    _own_loop_check(netG, cond, x_T, zs if rule == 'ancestral' else None, eager, y.cpu().numpy())
    # graph replay equals the eager loop bit for bit (the ancestral rule draws its noise: same seed on both sides)
    outs = []
    for use_graph in (False, True):
        netG.use_graph = use_graph
        torch.manual_seed(17)
        outs.append(netG.p_sample_loop(cond, continous=True, x_T=x_T).clone())
    st = next(reversed(netG._loop_cache.values()))
    assert st['graph'] is not None and torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[1]).all())
    if rule != 'ancestral':
        assert torch.equal(outs[1], eager)
    on = backprojection_error(outs[1][-B:].contiguous(), y, s, resample)
    # without the key the same chain (same x_T, same seed) is further from the LR image
    netG.set_backprojection(None)
    netG.use_graph = False
    torch.manual_seed(17)
    plain = netG.p_sample_loop(cond, continous=True, x_T=x_T)
    off = backprojection_error(plain[-B:].contiguous(), y, s, resample)
    print('%s s %d %s K %d strength %g: max |D(SR) - y| with the key %.4e, without %.4e' % (rule, s, resample, K, lam, on, off))
    assert on < off


def test_backprojection_target_is_honoured():
    from sr3_hip.diffusion import backprojection_error, resample_f32
    d = G.dev()
    netG, g = _model({'scale': 4, 'iterations': 2}, {'type': 'ddim', 'steps': 5})
    cond, x_T = (torch.from_numpy(g['loop/' + n]).to(d) for n in ('sr', 'x_T'))
    B = cond.shape[0]
    own = resample_f32(cond, (4, 4))
    target = (0.5 * own + 0.2).contiguous()
    assert float((target - own).abs().max()) > 0.1
    netG.use_graph = False
    out = netG.p_sample_loop(cond, continous=True, x_T=x_T, backprojection_target=target)
    st = next(reversed(netG._loop_cache.values()))
    assert torch.equal(st['y_lr'], target)
    _own_loop_check(netG, cond, x_T, None, out, target.cpu().numpy())
    for use_graph in (False, True):
        netG.use_graph = use_graph
        res = netG.super_resolution(cond, continous=True, backprojection_target=target)[-B:].contiguous()
        assert backprojection_error(res, target, 4) < backprojection_error(res, own, 4)
    # back to the conditioning image's own down-sample on the same cached state
    res = netG.super_resolution(cond, continous=True)[-B:].contiguous()
    assert torch.equal(st['y_lr'], own) and backprojection_error(res, own, 4) < backprojection_error(res, target, 4)
    with pytest.raises(L.Sr3Error, match='backprojection_target'):
        netG.p_sample_loop(cond, backprojection_target=target[:, :, :2])
    netG.set_backprojection(3)
    with pytest.raises(L.Sr3Error, match='3.*16 x 16'):
        netG.p_sample_loop(cond)


def test_off_means_off():
    d = G.dev()
    netG, g = _model({'scale': 4})
    never, _ = _model(None)
    cond, x_T, zs = (torch.from_numpy(g['loop/' + n]).to(d) for n in ('sr', 'x_T', 'zs'))
    T = zs.shape[0]
    calls = []
    real = netG.denoise_fn.reverse_step

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    netG.denoise_fn.reverse_step = spy
    netG.use_graph = False
    netG.p_sample_loop(cond, x_T=x_T, noise_seq=zs)
    assert calls == []                                   # on: the branch of its own, not the fused step
    netG.set_backprojection(None)
    assert netG.backprojection is None and netG._loop_cache == {}
    off = netG.p_sample_loop(cond, continous=True, x_T=x_T, noise_seq=zs)
    assert len(calls) == T
    key, st = next(reversed(netG._loop_cache.items()))
    assert 'y_lr' not in st and 'backprojection' not in st and 'bp_scratch' not in st and key[-4] is None
    never.use_graph = False
    assert never.backprojection is None
    assert torch.equal(off, never.p_sample_loop(cond, continous=True, x_T=x_T, noise_seq=zs))
    del netG.denoise_fn.reverse_step
    # the same with the loop drawing its own noise, same seed on both sides
    outs = []
    for n in (netG, never):
        torch.manual_seed(5)
        outs.append(n.p_sample_loop(cond, continous=True, x_T=x_T).clone())
    assert torch.equal(outs[0], outs[1])
