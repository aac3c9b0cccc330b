"""Guided sampling on the GPU (csrc/guidance.hip, EngineDiffusion.set_guidance / set_cond_drop): sr3_abs_quantile_f32, sr3_cond_drop_f32 and
sr3_guided_step through the C ABI against the NumPy restatements of tests/test_guidance_cpu.py, the chains of p_sample_loop under the
"guidance" key against a loop written here from denoise_fn forwards plus that restatement, and the training step under "cond_drop".

Shapes of the select: 1, 2, 48, 105 and 769 values (one workgroup per image; 769 with the source off a 16-byte boundary), 65 537 and
196 608 values (beyond the 8192 values the single-workgroup form takes: 17 and 48 workgroups per image, the first with a last chunk of
one value).  The order statistic is exact, so every comparison of a quantile or a threshold is an equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util as G                                                                      # noqa: E402
from helpers import load_golden, opt_for                                                  # noqa: E402
from sr3_hip import lib as L                                                              # noqa: E402
from sr3_hip.diffusion import quantile_rank                                               # noqa: E402
from test_guidance_cpu import F, KEYS, MODES, oracle_guided_step, oracle_quantile         # noqa: E402

GUARD = 1024      # floats of NaN around a tensor, in the same allocation
PS = (0, 0.5, 0.995, 1)


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


def _ints(v, d):
    return torch.tensor(v, dtype=torch.int32, device=d)


class Scratch:
    """the select's scratch inside a larger byte buffer filled with 0xA5 (so the call has to initialise what it reads), 4096 guard bytes
    on either side"""
    PAD = 4096

    def __init__(self, batch, n, d):
        self.bytes = int(L.load().sr3_abs_quantile_scratch_bytes(batch, n))
        assert self.bytes > 0
        self.buf = torch.full((self.bytes + 2 * self.PAD,), 0xA5, dtype=torch.uint8, device=d)
        self.view = self.buf[self.PAD:self.PAD + self.bytes]

    def guard_intact(self):
        return bool((self.buf[:self.PAD] == 0xA5).all()) and bool((self.buf[self.PAD + self.bytes:] == 0xA5).all())


# ---- 1. the select ----------------------------------------------------------------------------------------------------------------------

Q_SHAPES = [(1, 1, 0), (2, 2, 0), (3, 48, 0), (2, 105, 0), (2, 769, 1), (2, 65537, 0), (1, 196608, 0)]
Q_IDS = ['%dx%d%s' % (b, n, '-misaligned' if m else '') for b, n, m in Q_SHAPES]


def _quantile(v, rank_lo, frac, d, mis=0, scratch=None):
    B, n = v.shape
    vd, vbuf, vo = _dev(v, d, mis)
    out, obuf, oo = _dev(np.full(B, np.nan, dtype=F), d)
    sc = Scratch(B, n, d) if scratch is None else scratch
    L.check(L.load().sr3_abs_quantile_f32(L.ptr(vd), B, n, rank_lo, frac, L.ptr(out), L.ptr(sc.view), sc.bytes, G.stream()))
    torch.cuda.synchronize()
    assert _guard_intact(obuf, oo, B), 'the select wrote outside out_dev'
    assert sc.guard_intact(), 'the select wrote outside its scratch'
    assert vd.cpu().numpy().tobytes() == np.asarray(v, dtype=F).tobytes()
    return out.cpu().numpy()


def _q_inputs(B, n, rank_lo):
    g = np.random.default_rng(31 * B + n)
    gauss = g.standard_normal((B, n)).astype(F)
    equal = np.full((B, n), -0.75, dtype=F)
    two = np.full((B, n), 2.5, dtype=F)              # ranks 0 .. rank_lo hold 0.5, the ranks above it 2.5: the boundary sits between v_lo and v_hi
    idx = g.permutation(n)[:rank_lo + 1]
    two[:, idx] = -0.5
    tiny = g.choice(np.array([0.0, -0.0, 1e-45, -1e-45, 3e-39, -7e-42, 1.1754942e-38], dtype=F), size=(B, n))
    one_inf = gauss.copy()
    one_inf[:, g.integers(n)] = np.inf
    heavy = (g.standard_normal((B, n)) * np.exp(3.0 * g.standard_normal((B, n)))).astype(F)
    return dict(gauss=gauss, equal=equal, two_valued=two, zeros_denormals=tiny, one_inf=one_inf, heavy=heavy)


@pytest.mark.parametrize('case', Q_SHAPES, ids=Q_IDS)
def test_abs_quantile_is_exact(case):
    B, n, mis = case
    d = G.dev()
    sc = Scratch(B, n, d)                                  # one scratch, never cleaned between the calls
    for p in PS:
        rank_lo, frac = quantile_rank(n, p)
        for name, v in _q_inputs(B, n, rank_lo).items():
            want = oracle_quantile(v, rank_lo, frac)
            got = _quantile(v, rank_lo, frac, d, mis, sc)
            assert got.tobytes() == want.tobytes(), (name, p, got, want)
            if name == 'two_valued' and rank_lo + 1 < n:
                assert want[0] == F(np.float64(0.5) + frac * 2.0)
            if name == 'one_inf' and p == 1:
                assert want[0] == np.inf
        # the same bits again
        v = _q_inputs(B, n, rank_lo)['heavy']
        assert _quantile(v, rank_lo, frac, d, mis, sc).tobytes() == _quantile(v, rank_lo, frac, d, mis).tobytes()
    # a fractional rank everywhere, also at the smallest and the largest
    for rank_lo, frac in ((0, 0.25), (max(n - 2, 0), 0.75), (n // 2, 1.0 / 3)):
        v = _q_inputs(B, n, rank_lo)['heavy']
        assert _quantile(v, rank_lo, frac, d, mis, sc).tobytes() == oracle_quantile(v, rank_lo, frac).tobytes(), (rank_lo, frac)


@pytest.mark.parametrize('case', [(2, 105, 0), (2, 65537, 0)], ids=['single', 'split'])
def test_abs_quantile_with_nans_terminates_inside_its_buffers(case):
    """a NaN is a key above inf's: the ranks below the NaNs are still exact, and whatever the values the guards stay intact"""
    B, n, mis = case
    g = np.random.default_rng(n)
    v = g.standard_normal((B, n)).astype(F)
    v[:, ::7] = np.nan
    v[0, 1] = -np.inf
    nn = int(np.isnan(v[0]).sum())
    got = _quantile(v, n - 1, 0.0, G.dev(), mis)
    assert np.all(np.isnan(got))
    rank_lo = n - nn - 2                                    # image 1: the second largest finite value, a rank below the NaNs
    fin = np.where(np.isnan(v), F(0.0), v)
    want = np.sort(np.abs(fin[1]))[nn:][rank_lo]
    assert _quantile(v, rank_lo, 0.0, G.dev(), mis)[1] == want


# ---- 2. conditioning dropout ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [48, 105])
@pytest.mark.parametrize('mis', [0, 1])
def test_cond_drop_is_a_bit_copy(n, mis):
    d = G.dev()
    g = np.random.default_rng(n)
    bits = g.integers(0, 2 ** 32, size=(3, n), dtype=np.uint64).astype(np.uint32)      # every bit pattern: NaN payloads, -0.0, denormals
    bits[0, 0], bits[1, 1], bits[2, 2] = 0x80000000, 0x7fc00001, 0xffffffff
    src = bits.view(F)
    keep = _ints([1, 0, 1], d)
    want = bits.copy()
    want[1] = 0
    lib = L.load()
    sd, sbuf, so = _dev(torch.from_numpy(src.copy()), d, mis)
    dd, dbuf, do = _dev(np.full((3, n), np.nan, dtype=F), d, 2 * mis)
    L.check(lib.sr3_cond_drop_f32(L.ptr(sd), L.ptr(keep), 3, n, L.ptr(dd), G.stream()))
    torch.cuda.synchronize()
    assert _guard_intact(dbuf, do, 3 * n) and _guard_intact(sbuf, so, 3 * n)
    assert dd.cpu().numpy().view(np.uint32).tobytes() == want.tobytes() and sd.cpu().numpy().view(np.uint32).tobytes() == bits.tobytes()
    # in place
    L.check(lib.sr3_cond_drop_f32(L.ptr(sd), L.ptr(keep), 3, n, L.ptr(sd), G.stream()))
    torch.cuda.synchronize()
    assert _guard_intact(sbuf, so, 3 * n) and sd.cpu().numpy().view(np.uint32).tobytes() == want.tobytes()
    assert keep.tolist() == [1, 0, 1]
    # a partial overlap is refused and nothing moves
    assert lib.sr3_cond_drop_f32(L.ptr(sd), L.ptr(keep), 3, n, L.ptr(sd.reshape(-1)[4:]), G.stream()) == -1
    assert b'partially' in lib.sr3_last_error()


# ---- 3. the step against the oracle --------------------------------------------------------------------------------------------------------

# ((B, C, H, W), misaligned)
SHAPES = [((2, 3, 16, 16), False), ((1, 3, 6, 10), False), ((2, 3, 8, 8), True), ((1, 3, 256, 256), False)]
IDS = ['x'.join(map(str, s)) + ('-misaligned' if m else '') for s, m in SHAPES]
# four rows that differ; row 2 is the a = 0.9, b = 0.43 row most calls run at: |x0| reaches 3, its 99.5th percentile is about 2.8
TABLES = dict(a=[1.1, 0.7, 0.9, 0.6], b=[0.2, 0.75, 0.43, 0.7], c1=[1.0, 0.45, 0.55, 0.4], c2=[0.0, 0.5, 0.45, -0.2],
              sigma=[0.0, 0.4, 0.5, 0.25], c3=[0.0, -0.35, 0.5, -0.45])
J = 2
P = 0.995


def _tabs():
    return {k: np.asarray(v, dtype=F) for k, v in TABLES.items()}


def _inputs(shape, scale=1.0):
    g = np.random.default_rng(sum(shape))
    x = (scale * g.standard_normal(shape)).astype(F)
    oc, ou, z, h = (g.standard_normal(shape).astype(F) for _ in range(4))
    return x, oc, ou, z, h


def _call(x, oc, ou, scale, z, dt, c3, hist, step2, mode, rank_lo, frac, x0, sc, thr):
    B, Cc, H, W = x.shape
    rc = L.load().sr3_guided_step(L.ptr(x), L.ptr(oc), L.ptr(ou), scale, L.ptr(z), B, Cc, H, W, *[L.ptr(dt[k]) for k in KEYS], L.ptr(c3),
                                  L.ptr(hist), L.ptr(step2), mode, rank_lo, frac, L.ptr(x0), None if sc is None else L.ptr(sc.view),
                                  0 if sc is None else sc.bytes, L.ptr(thr), G.stream())
    torch.cuda.synchronize()
    return rc


def _run(case, d, mode, guided, scale, with_hist, with_z, inputs, j=J, with_thr=True):
    """one call on guarded (and, for the misaligned case, shifted) copies of the inputs -> (x', hist' or None, thr or None, counter)"""
    shape, mis = case
    x, oc, ou, z, h = inputs
    B = shape[0]
    n = int(np.prod(shape[1:]))
    rank_lo, frac = quantile_rank(n, P)
    dt = {k: torch.from_numpy(v).to(d) for k, v in _tabs().items()}
    m = 1 if mis else 0
    xd, xbuf, xo = _dev(x, d, m)
    cd = _dev(oc, d, m)[0]
    ud = _dev(ou, d, m)[0] if guided else None
    zd = _dev(z, d, m)[0] if with_z else None
    hd, hbuf, ho = _dev(h, d, m) if with_hist else (None, None, 0)
    x0d, x0buf, x0o = _dev(np.full(shape, np.nan, dtype=F), d, m) if mode == 2 else (None, None, 0)
    sc = Scratch(B, n, d) if mode == 2 else None
    thr, tbuf, to = _dev(np.full(B, np.nan, dtype=F), d) if with_thr else (None, None, 0)
    step2 = _ints([-7, j], d)
    assert _call(xd, cd, ud, scale, zd, dt, dt['c3'] if with_hist else None, hd, step2, mode, rank_lo, frac, x0d, sc, thr) == 0, \
        L.load().sr3_last_error()
    assert _guard_intact(xbuf, xo, xd.numel()), 'the step wrote outside x'
    assert hbuf is None or _guard_intact(hbuf, ho, hd.numel()), 'the step wrote outside hist'
    assert x0buf is None or _guard_intact(x0buf, x0o, x0d.numel()), 'the step wrote outside x0_scratch'
    assert sc is None or sc.guard_intact(), 'the step wrote outside q_scratch'
    assert tbuf is None or _guard_intact(tbuf, to, B), 'the step wrote outside thr_out_dev'
    assert torch.equal(cd.cpu(), torch.from_numpy(oc)) and (ud is None or torch.equal(ud.cpu(), torch.from_numpy(ou)))
    return (xd.cpu().numpy(), None if hd is None else hd.cpu().numpy(), None if thr is None else thr.cpu().numpy(), step2.tolist())


def _check(got, want, what):
    """|got - oracle| <= 4 * 2^-23 * max(1, |oracle|) per element (the bound of tests/test_gpu_consistency.py; the kernel runs the
    oracle's operations, so the difference is printed and expected to be zero)"""
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    tol = 4.0 * 2.0 ** -23 * np.maximum(1.0, np.abs(want.astype(np.float64)))
    print('%s: max |diff| %.3e, %d elements differ' % (what, diff.max(), int((got != want).sum())))
    assert np.all(diff <= tol), '%s: %g' % (what, diff.max())


@pytest.mark.parametrize('case', SHAPES, ids=IDS)
def test_guided_step_against_oracle(case):
    shape, mis = case
    d = G.dev()
    n = int(np.prod(shape[1:]))
    rank_lo, frac = quantile_rank(n, P)
    inputs = _inputs(shape)
    x, oc, ou, z, h = inputs
    tabs = _tabs()
    combos = [(mode, gs, hi, wz) for mode in (0, 1, 2) for gs in ((False, 1.5), (True, 1.5), (True, 0.0), (True, 3.0)) for hi in (False, True)
              for wz in (False, True)]
    if n > 100000:
        combos = combos[::5]      # (the large case: the paths are the small cases'; ten combinations keep it quick)
    above = 0
    for mode, (guided, scale), hi, wz in combos:
        gx, gh, thr, step2 = _run(case, d, mode, guided, scale, hi, wz, inputs)
        assert step2 == [J, J - 1]
        wx, wh, wthr = oracle_guided_step(x, oc, ou if guided else None, scale, z if wz else None, tabs, J, mode, rank_lo, frac, h if hi else None)
        what = '%s mode %d guided %d scale %g hist %d z %d' % (shape, mode, guided, scale, hi, wz)
        assert thr.tobytes() == wthr.tobytes(), (what, thr, wthr)
        _check(gx, wx, what + ': x')
        if hi:
            _check(gh, wh, what + ': hist')
        above += int(mode == 2 and np.all(wthr > 1.0))
    assert above > 0                                       # the dynamic rule did rescale
    # rows 0 and last; the tables are read at row j, and thr_out_dev may be NULL
    for j in (0, 3):
        gx, gh, thr, step2 = _run(case, d, 2, True, 1.5, True, True, inputs, j=j, with_thr=(j == 0))
        assert step2 == [j, j - 1]
        wx, wh, wthr = oracle_guided_step(x, oc, ou, 1.5, z, tabs, j, 2, rank_lo, frac, h)
        assert thr is None or thr.tobytes() == wthr.tobytes()
        _check(gx, wx, 'row %d: x' % j)
        _check(gh, wh, 'row %d: hist' % j)
    other = oracle_guided_step(x, oc, ou, 1.5, z, tabs, J - 1, 2, rank_lo, frac, h)[0]
    assert np.abs(_run(case, d, 2, True, 1.5, True, True, inputs)[0] - other).max() > 0.1
    # two runs give the same bits
    a = _run(case, d, 2, True, 3.0, True, True, inputs)
    b = _run(case, d, 2, True, 3.0, True, True, inputs)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


# ---- 4. bit anchors ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', SHAPES[:3], ids=IDS[:3])
@pytest.mark.parametrize('with_hist', [False, True])
def test_mode_1_without_guidance_is_the_existing_step(case, with_hist):
    """out_u NULL, mode 1: sr3_p_sample_step_hist + sr3_step_decrement, bit for bit"""
    shape, mis = case
    d = G.dev()
    inputs = _inputs(shape, scale=2.0)
    x, oc, ou, z, h = inputs
    gx, gh, thr, step2 = _run(case, d, 1, False, 1.5, with_hist, True, inputs)
    assert np.all(thr == 1.0) and step2 == [J, J - 1]
    dt = {k: torch.from_numpy(v).to(d) for k, v in _tabs().items()}
    xd, ed, zd = (torch.from_numpy(t).to(d) for t in (x, oc, z))
    hd = torch.from_numpy(h).to(d) if with_hist else None
    step = _ints([J], d)
    lib = L.load()
    L.check(lib.sr3_p_sample_step_hist(L.ptr(xd), L.ptr(ed), L.ptr(zd), *[L.ptr(dt[k]) for k in KEYS], L.ptr(step), None, 0, shape[0],
                                       xd[0].numel(), 1, L.ptr(dt['c3']) if with_hist else None, L.ptr(hd), G.stream()))
    L.check(lib.sr3_step_decrement(L.ptr(step), G.stream()))
    torch.cuda.synchronize()
    assert step.tolist() == [J - 1]
    assert xd.cpu().numpy().tobytes() == gx.tobytes()
    if with_hist:
        assert hd.cpu().numpy().tobytes() == gh.tobytes()


@pytest.mark.parametrize('case', SHAPES[:3], ids=IDS[:3])
def test_mode_2_on_a_tame_image_is_mode_1(case):
    """|x0| <= 1 everywhere: s = 1, the clamp does nothing, x0 / 1 is x0 -- the same bits as the static clamp, and every threshold is 1.0"""
    shape, mis = case
    d = G.dev()
    x, oc, ou, z, h = _inputs(shape)
    inputs = (np.clip(0.3 * x, -0.6, 0.6).astype(F), np.clip(0.3 * oc, -0.2, 0.2).astype(F), np.clip(0.3 * ou, -0.2, 0.2).astype(F), z, h)
    # |x0| <= 0.9 * 0.6 + 0.43 * (0.2 + 1.5 * 0.4) = 0.884
    for guided in (False, True):
        a = _run(case, d, 2, guided, 1.5, True, True, inputs)
        b = _run(case, d, 1, guided, 1.5, True, True, inputs)
        assert np.abs(a[1]).max() <= 0.885
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert np.all(a[2] == 1.0) and np.all(b[2] == 1.0)


# ---- 5. refusals launch nothing ----------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    d = G.dev()
    shape = (2, 3, 8, 12)
    n = 3 * 8 * 12
    x, oc, ou, z, h = (torch.from_numpy(t).to(d) for t in _inputs(shape))
    dt = {k: torch.from_numpy(v).to(d) for k, v in _tabs().items()}
    x0 = torch.zeros(shape, device=d)
    sc = Scratch(2, n, d)
    thr = torch.full((2,), -3.0, device=d)
    keep_x, keep_h = x.clone(), h.clone()
    step2 = _ints([-7, J], d)
    lib = L.load()
    ok = dict(x=x, oc=oc, ou=ou, scale=1.5, z=z, c3=dt['c3'], hist=h, mode=2, rank_lo=100, frac=0.5, x0=x0, sc=sc, thr=thr)
    for kw, code, word in ((dict(oc=None), -1, b'out_c'), (dict(mode=3), -1, b'mode'), (dict(scale=float('nan')), -1, b'scale'),
                           (dict(scale=float('inf')), -1, b'scale'), (dict(rank_lo=n), -1, b'rank_lo'), (dict(rank_lo=-1), -1, b'rank_lo'),
                           (dict(frac=1.0), -1, b'frac'), (dict(x0=None), -1, b'x0_scratch'), (dict(sc=None), -1, b'scratch'),
                           (dict(hist=x), -1, b'overlaps'), (dict(c3=None), -1, b'c3'), (dict(x0=x), -1, b'x0_scratch overlaps x_nchw'),
                           (dict(x0=h), -1, b'hist_nchw overlaps x0_scratch'), (dict(ou=x), -1, b'out_u overlaps x_nchw'),
                           (dict(ou=h), -1, b'hist_nchw overlaps out_u'), (dict(x0=ou), -1, b'x0_scratch overlaps out_u')):
        a = dict(ok, **kw)
        assert _call(a['x'], a['oc'], a['ou'], a['scale'], a['z'], dt, a['c3'], a['hist'], step2, a['mode'], a['rank_lo'], a['frac'], a['x0'],
                     a['sc'], a['thr']) == code, kw
        assert lib.sr3_last_error().startswith(b'guided_step') and word in lib.sr3_last_error(), (kw, lib.sr3_last_error())
    small = Scratch(2, n, d)
    small.bytes -= 4
    assert _call(x, oc, ou, 1.5, z, dt, dt['c3'], h, step2, 2, 100, 0.5, x0, small, thr) == -1 and b'scratch_bytes' in lib.sr3_last_error()
    assert torch.equal(x, keep_x) and torch.equal(h, keep_h) and step2.tolist() == [-7, J] and thr.tolist() == [-3.0, -3.0]
    assert bool((x0 == 0).all()) and bool((sc.buf == 0xA5).all())
    # the select's own entry
    out = torch.full((2,), -3.0, device=d)
    v = x.reshape(2, n)
    for args, word in (((L.ptr(v), 2, n, n, 0.0, L.ptr(out), L.ptr(sc.view), sc.bytes), b'rank_lo'),
                       ((L.ptr(v), 2, n, 0, 1.0, L.ptr(out), L.ptr(sc.view), sc.bytes), b'frac'),
                       ((L.ptr(v), 2, n, 0, 0.0, L.ptr(out), L.ptr(sc.view), sc.bytes - 4), b'scratch_bytes'),
                       ((L.ptr(v), 2, n, 0, 0.0, L.ptr(v), L.ptr(sc.view), sc.bytes), b'out_dev')):
        assert lib.sr3_abs_quantile_f32(*args, G.stream()) == -1 and word in lib.sr3_last_error()
    torch.cuda.synchronize()
    assert out.tolist() == [-3.0, -3.0] and torch.equal(x, keep_x) and bool((sc.buf == 0xA5).all())


# ---- 6. the chains -----------------------------------------------------------------------------------------------------------------------------

def _model(guidance, sampler=None, phase='val'):
    import model as Model
    opt = opt_for('sr3_tiny', phase=phase, gpu=True)
    val = opt['model']['beta_schedule']['val']
    if guidance is not None:
        val['guidance'] = guidance
    if sampler is not None:
        val['sampler'] = sampler
    m = Model.create_model(opt)
    g, sd = load_golden('sr3_tiny')
    m.netG.load_state_dict(sd, strict=True)
    m.netG.show_progress = False
    m.set_new_noise_schedule(val, schedule_phase='val')
    return m.netG, g


def _rule_tables(netG):
    """the rule's tables on the host, as the engine's own _step_rule hands them to the kernel"""
    tables, level, t_map, c3, noisy = netG._step_rule()
    tabs = {k: t.cpu().numpy() for k, t in zip(KEYS, tables)}
    if c3 is not None:
        tabs['c3'] = c3.cpu().numpy()
    return tabs, level.cpu().numpy(), c3 is not None, noisy


def _own_loop_check(netG, cond, x_T, zs, out):
    """The chain again, written here: per step two denoise_fn forwards at the step's level (one when the scale is 1) on the ENGINE's
    image before the step (its previous snapshot: teacher forcing, so the per-step tolerance applies to every step) and the oracle
    tail; the history is carried by the oracle.  Every step of these chains is a snapshot (T = 8 or S = 5: stride 1).
    -> the oracle's thresholds per step, first step first"""
    d = cond.device
    gd = netG.guidance
    tabs, level, multistep, noisy = _rule_tables(netG)
    T = len(tabs['a'])
    B = cond.shape[0]
    assert out.shape[0] == B * (T + 1)
    mode = MODES.index(gd['threshold'])
    rank_lo, frac = quantile_rank(int(np.prod(x_T.shape[1:])), gd['percentile']) if mode == 2 else (0, 0.0)
    hist = np.zeros(tuple(x_T.shape), dtype=F) if multistep else None
    thrs = []
    for k, j in enumerate(reversed(range(T))):
        before = x_T if k == 0 else out[k * B:(k + 1) * B]
        lv = torch.full((B,), float(level[j + 1]), dtype=torch.float32, device=d)
        oc = netG.denoise_fn(before.contiguous(), lv, cond=cond).cpu().numpy()
        ou = netG.denoise_fn(before.contiguous(), lv, cond=torch.zeros_like(cond)).cpu().numpy() if gd['scale'] != 1.0 else None
        z = zs[j].cpu().numpy() if (noisy and zs is not None and j > 0) else None
        want, hist, thr = oracle_guided_step(before.cpu().numpy(), oc, ou, gd['scale'], z, tabs, j, mode, rank_lo, frac, hist)
        thrs.append(thr)
        got = out[(k + 1) * B:(k + 2) * B].cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - want).max())
        tol = 2e-5 * max(1.0, float(np.abs(want).max()))
        print('step index %d: max abs err %.3e (tolerance %.3e), thresholds %s' % (j, err, tol, thr))
        assert err <= tol, (j, err, tol)
    return thrs


def _spy_forwards(netG):
    calls = []
    real = netG.denoise_fn.forward

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    netG.denoise_fn.forward = spy
    return calls


@pytest.mark.parametrize('scale', [1.5, 1.0])
@pytest.mark.parametrize('rule', ['ancestral', 'ddim', 'dpmpp_2m'])
def test_chain_against_own_loop_and_graph(rule, scale):
    d = G.dev()
    sampler = None if rule == 'ancestral' else {'type': rule, 'steps': 5}
    netG, g = _model({'scale': scale, 'threshold': 'dynamic', 'percentile': 0.995}, sampler)
    assert netG.guidance == dict(scale=scale, threshold='dynamic', percentile=0.995)
    cond, x_T, zs = (torch.from_numpy(g['loop/' + n]).to(d) for n in ('sr', 'x_T', 'zs'))
    T = 8 if rule == 'ancestral' else 5
    # eager; the ancestral rule with its noise injected
    netG.use_graph = False
    calls = _spy_forwards(netG)
    eager = netG.p_sample_loop(cond, continous=True, x_T=x_T, noise_seq=zs if rule == 'ancestral' else None).clone()
    del netG.denoise_fn.forward
    assert len(calls) == (2 * T if scale != 1.0 else T)    # scale 1: dynamic thresholding for the price of one forward
    st = next(reversed(netG._loop_cache.values()))
    assert st['guidance'] == netG.guidance and st['step'].tolist() == [0, -1]
    assert (st['eps_u'] is None and st['cond0'] is None) == (scale == 1.0)
    assert (st['rank_lo'], st['frac']) == quantile_rank(3 * 16 * 16, 0.995)
    thrs = _own_loop_check(netG, cond, x_T, zs if rule == 'ancestral' else None, eager)
    assert np.all(thrs[0] > 1.0)                           # the first step's x0 is about x_T ~ N(0, 1): the dynamic branch ran
    assert np.allclose(st['thr'].cpu().numpy(), thrs[-1], rtol=2e-5, atol=0.0)      # (the last step's, from the engine's own forwards)
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


@pytest.mark.parametrize('rule', ['ancestral', 'ddim', 'dpmpp_2m'])
def test_scale_1_static_is_the_plain_chain_and_off_means_off(rule):
    d = G.dev()
    sampler = None if rule == 'ancestral' else {'type': rule, 'steps': 5}
    netG, g = _model({'scale': 1.0, 'threshold': 'static'}, sampler)
    never, _ = _model(None, sampler)
    assert never.guidance is None
    cond, x_T, zs = (torch.from_numpy(g['loop/' + n]).to(d) for n in ('sr', 'x_T', 'zs'))
    seq = zs if rule == 'ancestral' else None
    calls = []
    real = netG.denoise_fn.reverse_step

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    netG.denoise_fn.reverse_step = spy
    for n in (netG, never):
        n.use_graph = False
    plain = never.p_sample_loop(cond, continous=True, x_T=x_T, noise_seq=seq)
    on = netG.p_sample_loop(cond, continous=True, x_T=x_T, noise_seq=seq)
    assert calls == []                                     # on: the fourth branch, not the fused step
    assert torch.equal(on, plain)
    # off means off
    netG.set_guidance(None)
    assert netG.guidance is None and netG._loop_cache == {}
    off = netG.p_sample_loop(cond, continous=True, x_T=x_T, noise_seq=seq)
    assert len(calls) == (8 if rule == 'ancestral' else 5)
    st = next(reversed(netG._loop_cache.values()))
    key = next(reversed(netG._loop_cache.keys()))
    assert 'guidance' not in st and 'eps_u' not in st and key[-3] is None and key[-1] is None
    assert torch.equal(off, plain)
    # and replayed
    del netG.denoise_fn.reverse_step
    outs = []
    for n in (netG, never):
        n.use_graph = True
        torch.manual_seed(5)
        outs.append(n.p_sample_loop(cond, continous=True, x_T=x_T).clone())
    assert torch.equal(outs[0], outs[1])
    netG.set_guidance(1.0, 'static')
    torch.manual_seed(5)
    assert torch.equal(netG.p_sample_loop(cond, continous=True, x_T=x_T), outs[1])


# ---- 7. training with conditioning dropout -----------------------------------------------------------------------------------------------------

def _train_model(cond_drop=None):
    import model as Model
    opt = opt_for('sr3_tiny', phase='train', gpu=True)
    if cond_drop is not None:
        opt['model']['diffusion']['cond_drop'] = cond_drop
    m = Model.create_model(opt)
    g, sd = load_golden('sr3_tiny')
    m.netG.load_state_dict(sd, strict=True)
    return m.netG, g


def test_training_on_a_dropped_condition():
    d = G.dev()
    netG, g = _train_model()
    hr, sr = (torch.from_numpy(g['loop/' + n]).to(d) for n in ('hr', 'sr'))
    z, gamma = torch.from_numpy(g['train/z']).to(d), torch.from_numpy(g['train/gamma'])
    assert hr.shape[0] == 2

    def step(data, **kw):
        loss = netG.p_losses(data, noise=z, gamma=gamma, drop_seed=1234, **kw)
        torch.cuda.synchronize()
        return float(loss), netG.denoise_fn.grad_arena.clone()

    plain = step({'HR': hr, 'SR': sr})
    by_hand = sr.clone()
    by_hand[1] = 0.0
    want = step({'HR': hr, 'SR': by_hand})
    got = step({'HR': hr, 'SR': sr}, cond_keep=(1, 0))
    assert got[0] == want[0] and torch.equal(got[1], want[1])
    assert got[0] != plain[0] and not torch.equal(got[1], plain[1])
    kept = step({'HR': hr, 'SR': sr}, cond_keep=torch.tensor([1, 1]))
    assert kept[0] == plain[0] and torch.equal(kept[1], plain[1])
    assert torch.equal(sr, torch.from_numpy(g['loop/sr']).to(d))           # the batch's own conditioning image is not written
    with pytest.raises(L.Sr3Error, match='cond_keep'):
        netG.p_losses({'HR': hr, 'SR': sr}, noise=z, gamma=gamma, cond_keep=(1, 0, 1))


def test_cond_drop_draws_after_every_other_draw():
    d = G.dev()
    g = load_golden('sr3_tiny')[0]
    hr, sr = (torch.from_numpy(g['loop/' + n]).to(d) for n in ('hr', 'sr'))
    seen = {}
    for key in (None, 0.5):
        netG, _ = _train_model(key)
        assert netG.cond_drop == (0.0 if key is None else 0.5)
        real = netG.denoise_fn.train_step
        rec = []

        def spy(hr_, cond, z, ca, cb, level, *a, **kw):
            rec.append((cond.clone(), z.clone(), ca.clone()))
            return real(hr_, cond, z, ca, cb, level, *a, **kw)
        netG.denoise_fn.train_step = spy
        np.random.seed(3)
        torch.manual_seed(3)
        netG.p_losses({'HR': hr, 'SR': sr}, drop_seed=1)
        torch.cuda.synchronize()
        seen[key] = rec[0]
    assert torch.equal(seen[None][1], seen[0.5][1]) and torch.equal(seen[None][2], seen[0.5][2])      # the same (z, gamma)
    assert torch.equal(seen[None][0], sr)
    torch.manual_seed(3)
    torch.randn_like(hr)
    keep = torch.rand(2, device=d) >= 0.5                  # the draw p_losses made, after z
    assert torch.equal(seen[0.5][0], sr * keep.reshape(2, 1, 1, 1).to(sr.dtype))
