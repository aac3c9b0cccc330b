"""Zero-shot restoration on the GPU (csrc/restore.hip, EngineDiffusion.set_restore): sr3_restore_step, sr3_travel_back_f32 and
sr3_gray_f32 through the C ABI against the NumPy float32 restatement tests/restore_ref.py, bit for bit, with every operand inside NaN
bands (tests/guarded.py); and the chains of p_sample_loop under the "restore" key on the three tiny models.

Shapes: B = 2, C in {3, 1}, 8 x 8 (64 pixels: the 16-byte path, one thread per four pixels of all planes), 8 x 6 (a width that is no
multiple of 4: the one-element path) and 8 x 8 with every tensor 4 bytes off a 16-byte boundary (the one-element path again).  The
chains run at the models' own 16 x 16: the ancestral walk of the tiny schedule (8 steps; 6 for ddpm_tiny) and an 8-step DDIM walk --
for ddpm_tiny over a 16-step schedule, the shortest on which 8 steps stride (its own has 6), so the step-index -> timestep map is not
the identity."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util as G                                                                      # noqa: E402
import restore_ref as R                                                                   # noqa: E402
from guarded import Guarded, N                                                            # noqa: E402
from helpers import SCHEDS, load_golden, opt_for                                          # noqa: E402
from sr3_hip import lib as L                                                              # noqa: E402
from sr3_hip import x0_rules as X                                                         # noqa: E402

F = np.float32

# (B, C, H, W), misaligned
SHAPES = [((2, 3, 8, 8), False), ((2, 1, 8, 8), False), ((2, 3, 8, 6), False), ((2, 3, 8, 8), True)]
IDS = ['%s%s' % ('x'.join(map(str, s)), '-misaligned' if mis else '') for s, mis in SHAPES]

# four rows that differ; row 2 is the one the step tests run at; |c1|, |c2|, |c3|, |sigma| <= 1
TABLES = dict(a=[1.1, 0.7, 0.9, 0.6], b=[0.2, 0.75, 0.43, 0.7], c1=[1.0, 0.45, 0.55, 0.4], c2=[0.0, 0.5, 0.45, -0.2],
              sigma=[0.0, 0.4, 0.5, 0.25], c3=[0.0, -0.35, 0.5, -0.45])
J = 2


def _tabs():
    return {k: np.asarray(v, dtype=F) for k, v in TABLES.items()}


def _dev(t, d, mis=0):
    """`t` (numpy, fp32 or int32) on the device inside a tests/guarded.py buffer: NaN bands around a payload that is NaN too wherever
    the tensor is not, the tensor `mis` elements off the payload's (256-byte aligned) start -> (view, check) with check() true while
    nothing outside the tensor was written"""
    t = torch.from_numpy(np.ascontiguousarray(t))
    n = t.numel()
    g = Guarded((n + 4) * 4, N, d)
    flat = g.view(t.dtype)
    v = flat[mis:mis + n].view(t.shape)
    v.copy_(t)

    def check():
        raw = g.view(torch.uint8)
        return g.intact() and bool((raw[:mis * 4] == N).all()) and bool((raw[(mis + n) * 4:] == N).all())
    return v, check


def _ints(v, d):
    return torch.tensor(v, dtype=torch.int32, device=d)


def _floats(v):
    return X._floats(v)


def _operands(shape, seed):
    g = np.random.default_rng(seed)
    B, Cc, H, W = shape
    x, eps, z, h = (g.standard_normal(shape).astype(F) for _ in range(4))
    known = g.uniform(-1.0, 1.0, shape).astype(F)
    gray = g.uniform(-1.0, 1.0, (B, 1, H, W)).astype(F)
    masks = {'hard-1': (g.uniform(size=(B, 1, H, W)) < 0.5).astype(F), 'frac-1': g.uniform(size=(B, 1, H, W)).astype(F),
             'hard-C': (g.uniform(size=shape) < 0.5).astype(F), 'frac-C': g.uniform(size=shape).astype(F)}
    return x, eps, z, h, known, gray, masks


def _weights(Cc):
    return X.gray_weights('rec601' if Cc == 3 else [0.75] if Cc == 1 else 'mean', Cc)


def _call_step(d, mis, x, eps, z, op, target, mask, a, p, lam, clip, hist, j=J):
    """one sr3_restore_step on guarded copies -> (x', hist' or None, the counter) on the host; the inputs come back unchanged"""
    tabs = _tabs()
    dt = {k: torch.from_numpy(v).to(d) for k, v in tabs.items()}
    m = 1 if mis else 0
    xd, xok = _dev(x, d, m)
    ed, eok = _dev(eps, d, m)
    zd, zok = _dev(z, d, m) if z is not None else (None, lambda: True)
    hd, hok = _dev(hist, d, m) if hist is not None else (None, lambda: True)
    td, tok = _dev(target, d, m)
    md, mok = _dev(mask, d, m) if mask is not None else (None, lambda: True)
    step2 = _ints([-7, j], d)
    B, Cc, H, W = x.shape
    rc = L.load().sr3_restore_step(L.ptr(xd), L.ptr(ed), L.ptr(zd), op, L.ptr(td), L.ptr(md), 0 if mask is None else mask.shape[1],
                                   None if a is None else _floats(a), None if p is None else _floats(p), B, Cc, H, W, lam,
                                   *[L.ptr(dt[k]) for k in R.KEYS], L.ptr(step2), clip, L.ptr(dt['c3']) if hist is not None else None,
                                   L.ptr(hd), G.stream())
    assert rc == 0, L.load().sr3_last_error()
    torch.cuda.synchronize()
    assert xok() and eok() and zok() and hok() and tok() and mok(), 'a kernel wrote outside its tensors'
    assert np.array_equal(ed.cpu().numpy(), eps) and np.array_equal(td.cpu().numpy(), target)
    assert mask is None or np.array_equal(md.cpu().numpy(), mask)
    return xd.cpu().numpy(), None if hd is None else hd.cpu().numpy(), step2.tolist()


def _same(got, want, what):
    assert not np.isnan(got).any(), '%s: a NaN band was read' % what
    assert got.tobytes() == want.tobytes(), '%s: %d of %d elements differ from the restatement, max %.3e' % (
        what, int((got != want).sum()), got.size, float(np.abs(got.astype(np.float64) - want).max()))


# ---- 1. the step, bit for bit ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', SHAPES, ids=IDS)
def test_restore_step_is_the_restatement_bitwise(case):
    shape, mis = case
    d = G.dev()
    x, eps, z, h, known, gray, masks = _operands(shape, 7 + sum(shape))
    a, p = _weights(shape[1])
    tabs = _tabs()
    ops = [(0, known, masks[k], None, None, k) for k in (('hard-1', 'frac-1') if shape[1] == 1 else ('hard-1', 'frac-1', 'hard-C', 'frac-C'))]
    ops.append((1, gray, None, a, p, 'gray'))
    for op, target, mask, wa, wp, name in ops:
        for clip in (0, 1):
            for hi in (False, True):
                for wz in (False, True):
                    for lam in (1.0, 0.625):
                        gx, gh, step2 = _call_step(d, mis, x, eps, z if wz else None, op, target, mask, wa, wp, lam, clip, h if hi else None)
                        assert step2 == [J, J - 1]          # the counter ends at j - 1; slot 0 is the step's scratch copy
                        wx, wh = R.restore_step(x, eps, z if wz else None, op, target, mask, wa, wp, lam, tabs, J, clip, h if hi else None)
                        what = '%s %s clip %d hist %d z %d strength %g' % (name, shape, clip, hi, wz, lam)
                        _same(gx, wx, what + ': x')
                        if hi:
                            _same(gh, wh, what + ': hist')
    # the tables are read at row j: the other rows, and the counter follows
    for j in (0, 3):
        gx, gh, step2 = _call_step(d, mis, x, eps, z, 1, gray, None, a, p, 1.0, 1, h, j=j)
        assert step2 == [j, j - 1]
        wx, wh = R.restore_step(x, eps, z, 1, gray, None, a, p, 1.0, tabs, j, 1, h)
        _same(gx, wx, 'row %d: x' % j)
        _same(gh, wh, 'row %d: hist' % j)


def test_restore_step_properties_on_the_device():
    """what the chains rest on, at the kernel: a hard mask at strength 1 keeps the known pixels' x0 bit for bit (the history the step
    leaves is x0'), and the gray projection lands on the target within the bound of tests/restore_ref.py"""
    shape = (2, 3, 8, 8)
    d = G.dev()
    x, eps, z, h, known, gray, masks = _operands(shape, 99)
    m = masks['hard-1']
    _, gh, _ = _call_step(d, False, x, eps, z, 0, known, m, None, None, 1.0, 1, h)
    mb = np.broadcast_to(m, shape) == 1
    x0 = np.clip(F(0.9) * x - F(0.43) * eps, F(-1), F(1))
    assert np.array_equal(gh[mb], known[mb]) and np.array_equal(gh[~mb], x0[~mb])
    a, p = _weights(3)
    _, gh, _ = _call_step(d, False, x, eps, z, 1, gray, None, a, p, 1.0, 1, h)
    bound = R.gray_bound(a, p, 1.0, 1.0)      # clip on: |x0| <= 1; |y| <= 1
    resid = np.abs((a.astype(np.float64)[None, :, None, None] * gh.astype(np.float64)).sum(1, keepdims=True) - gray.astype(np.float64)).max()
    print('gray residual on the device %.3e (bound %.3e)' % (resid, bound))
    assert resid <= bound


def test_refusals_launch_nothing():
    d = G.dev()
    shape = (2, 3, 8, 8)
    x, eps, z, h, known, gray, masks = (t if isinstance(t, dict) else torch.from_numpy(t).to(d) for t in _operands(shape, 5))
    dt = {k: torch.from_numpy(v).to(d) for k, v in _tabs().items()}
    keep = x.clone()
    step2 = _ints([-7, J], d)
    lib = L.load()
    mask = torch.from_numpy(masks['hard-1']).to(d)
    a, p = _weights(3)
    for kw, word in ((dict(mc=2), b'mask_channels'), (dict(lam=0.0), b'strength'), (dict(target=x), b'overlaps'), (dict(op=3), b'op must be'),
                     (dict(hist=x), b'overlaps'), (dict(c3=None), b'c3')):
        q = dict(op=0, target=known, mc=1, lam=1.0, c3=dt['c3'], hist=h)
        q.update(kw)
        rc = lib.sr3_restore_step(L.ptr(x), L.ptr(eps), L.ptr(z), q['op'], L.ptr(q['target']), L.ptr(mask), q['mc'], _floats(a), _floats(p),
                                  *shape, q['lam'], *[L.ptr(dt[k]) for k in R.KEYS], L.ptr(step2), 1, L.ptr(q['c3']), L.ptr(q['hist']), G.stream())
        torch.cuda.synchronize()
        assert rc == -1 and word in lib.sr3_last_error(), (kw, lib.sr3_last_error())
    assert torch.equal(x, keep) and step2.tolist() == [-7, J]


# ---- 2. the jump -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('per,mis', [(192, False), (75, False), (192, True)], ids=['per192', 'per75', 'per192-misaligned'])
def test_travel_back_is_the_restatement_bitwise(per, mis):
    d = G.dev()
    g = np.random.default_rng(per + mis)
    B, rows = 2, 4
    x, z = (g.standard_normal((B, per)).astype(F) for _ in range(2))
    ra = np.asarray([0.8, 1.0, 0.6, 1.0], dtype=F)          # row 0: the jump from counter -1; rows 1 and 3: no jump defined
    rs = np.asarray([0.6, 0.0, 0.8, 0.0], dtype=F)
    to = np.asarray([2, 0, 3, 2], dtype=np.int32)
    rad, rsd, tod = (torch.from_numpy(t).to(d) for t in (ra, rs, to))
    for c in (-1, 1, 0, 2):
        xd, xok = _dev(x, d, 1 if mis else 0)
        zd, zok = _dev(z, d, 1 if mis else 0)
        step2 = _ints([-7, c], d)
        L.check(L.load().sr3_travel_back_f32(L.ptr(xd), L.ptr(zd), L.ptr(rad), L.ptr(rsd), L.ptr(tod), rows, L.ptr(step2), B, per, G.stream()))
        torch.cuda.synchronize()
        assert xok() and zok() and np.array_equal(zd.cpu().numpy(), z)
        want, cnt = R.travel_back(x, z, ra, rs, to, c)
        _same(xd.cpu().numpy(), want, 'counter %d' % c)
        assert step2.tolist() == [c, cnt] and cnt == int(to[c + 1])      # the counter lands on tab_to
        if c in (0, 2):      # an identity row: nothing moves
            assert np.array_equal(want, x) and cnt == c
    # a counter the tables have no row for touches nothing: neither x nor the counter
    xd, xok = _dev(x, d)
    zd, _ = _dev(z, d)
    for c in (rows - 1, -2):
        step2 = _ints([-7, c], d)
        L.check(L.load().sr3_travel_back_f32(L.ptr(xd), L.ptr(zd), L.ptr(rad), L.ptr(rsd), L.ptr(tod), rows, L.ptr(step2), B, per, G.stream()))
        torch.cuda.synchronize()
        assert xok() and np.array_equal(xd.cpu().numpy(), x) and step2.tolist() == [c, c]


# ---- 3. the gray image -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', SHAPES + [((2, 4, 8, 8), False), ((1, 2, 5, 7), False)], ids=IDS + ['2x4x8x8', '1x2x5x7'])
def test_gray_is_the_restatement_bitwise(case):
    shape, mis = case
    d = G.dev()
    B, Cc, H, W = shape
    src = np.random.default_rng(sum(shape)).standard_normal(shape).astype(F)
    a = _weights(Cc)[0]
    sd, sok = _dev(src, d, 1 if mis else 0)
    od, ook = _dev(np.full((B, 1, H, W), np.nan, dtype=F), d, 1 if mis else 0)
    L.check(L.load().sr3_gray_f32(L.ptr(sd), B, Cc, H, W, _floats(a), L.ptr(od), G.stream()))
    torch.cuda.synchronize()
    assert sok() and ook() and np.array_equal(sd.cpu().numpy(), src)
    _same(od.cpu().numpy(), R.gray(src, a), 'gray %s' % (shape,))
    if not mis:      # the public helper is the same call
        w = 'rec601' if Cc == 3 else [0.75] if Cc == 1 else 'mean'
        assert torch.equal(X.gray_f32(torch.from_numpy(src).to(d), w).cpu(), od.cpu())


# ---- 4. the chains -----------------------------------------------------------------------------------------------------------------------

MODELS = ('sr3_tiny', 'sr3_uncond', 'ddpm_tiny')
DDIM_SCHED = {'ddpm_tiny': dict(SCHEDS['ddpm_tiny'], n_timestep=16)}      # (8 steps that stride: see the module's docstring)
_models = {}


def _model(name, walk):
    """the model on the GPU with the golden weights under `walk` ('ancestral' | 'ddim'), restore off; made once per (name, walk)"""
    if (name, walk) not in _models:
        import model as Model
        opt = opt_for(name, phase='val', gpu=True)
        val = dict(opt['model']['beta_schedule']['val'])
        if walk == 'ddim':
            val = dict(DDIM_SCHED.get(name, val), sampler={'type': 'ddim', 'steps': 8})
        m = Model.create_model(opt)
        _, sd = load_golden(name)
        m.netG.load_state_dict(sd, strict=True)
        m.netG.show_progress = False
        m.netG.set_new_noise_schedule(val, G.dev())
        _models[(name, walk)] = m.netG
    netG = _models[(name, walk)]
    netG.set_restore(None)
    netG.use_graph = True
    return netG


SEEDS = [11, 12]


def _chain(netG, cond, **kw):
    """the chain's last images [B, C, H, W] (the unconditional DDPM loop returns them; the others return every snapshot)"""
    out = netG.p_sample_loop(cond, continous=True, item_seeds=SEEDS, **kw)
    return out[-len(SEEDS):].clone()


def _inputs(name, d):
    g, _ = load_golden(name)
    sr = torch.from_numpy(g['loop/sr']).to(d)
    cond = sr if name == 'sr3_tiny' else tuple(sr.shape)
    known = torch.from_numpy(np.random.default_rng(3).uniform(-0.9, 0.9, tuple(sr.shape)).astype(F)).to(d)
    return cond, known, tuple(sr.shape)


@pytest.mark.parametrize('walk', ['ancestral', 'ddim'])
@pytest.mark.parametrize('name', MODELS)
def test_mask_chains(name, walk):
    d = G.dev()
    netG = _model(name, walk)
    cond, known, shape = _inputs(name, d)
    B, Cc, H, W = shape
    assert netG.sampler is None or (netG.sampler['steps'] == 8 and (name != 'ddpm_tiny' or netG._sampler_tau.tolist() != list(range(8))))
    plain = _chain(netG, cond)
    netG.set_restore('mask')
    # an all-zero mask is the plain chain: w = 0 gives x0 exactly, and the unfused step is the fused one
    zero = _chain(netG, cond, restore_target=(known, torch.zeros((B, 1, H, W), device=d)))
    assert torch.equal(zero, plain)
    # an all-one hard mask at strength 1 returns `known` bit for bit (the last row: c1 = 1, c2 = 0, sigma = 0)
    c1, c2, sg = (float(t[0]) for t in netG._step_rule()[0][2:5])
    assert (c1, c2, sg) == (1.0, 0.0, 0.0)
    ones = _chain(netG, cond, restore_target=(known, torch.ones(shape, device=d)))
    assert torch.equal(ones, known)
    # a half mask: the known pixels are `known`'s bit for bit, the rest differ from it
    mask = torch.zeros((B, 1, H, W), device=d)
    mask[:, :, :, :W // 2] = 1.0
    outs = []
    for use_graph in (False, True):          # graph replay equals eager, bit for bit
        netG.use_graph = use_graph
        outs.append(_chain(netG, cond, restore_target=(known, mask)))
    st = next(reversed(netG._loop_cache.values()))
    assert st['graph'] is not None and st['restore'] == netG.restore and st['rs_mc'] == 1 and st['replays'] == (8 if walk == 'ddim' else netG.num_timesteps)
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[1]).all())
    mb = mask.expand(shape) == 1
    assert torch.equal(outs[1][mb], known[mb]) and bool((outs[1][~mb] != known[~mb]).all())
    assert X.restore_error(outs[1], netG.restore, (known, mask)) == 0.0
    assert not torch.equal(outs[1][~mb], plain[~mb])      # (and the free pixels follow the known ones: not the plain chain's either)
    # a per-channel mask on the same state: the graph is captured again for it
    mask3 = mask.expand(shape).clone()
    mask3[:, 1] = 1.0 - mask3[:, 1]
    out3 = _chain(netG, cond, restore_target=(known, mask3))
    assert st['rs_mc'] == Cc and torch.equal(out3[mask3 == 1], known[mask3 == 1])
    netG.set_restore(None)
    assert torch.equal(_chain(netG, cond), plain)


@pytest.mark.parametrize('walk', ['ancestral', 'ddim'])
@pytest.mark.parametrize('name', MODELS)
def test_gray_chains(name, walk):
    d = G.dev()
    netG = _model(name, walk)
    cond, known, shape = _inputs(name, d)
    B = shape[0]
    netG.set_restore('gray', 1.0, 'rec601')
    a, p = (np.asarray(netG.restore[k], dtype=F) for k in ('weights', 'pinv'))
    y = X.gray_f32(known, 'rec601')                       # the target: the gray of a colour image in [-0.9, 0.9]
    assert torch.equal(y.cpu(), torch.from_numpy(R.gray(known.cpu().numpy(), a)))
    outs = []
    for use_graph in (False, True):
        netG.use_graph = use_graph
        outs.append(_chain(netG, cond, restore_target=y))
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[1]).all())
    assert torch.equal(_chain(netG, cond, restore_target=known), outs[1])      # a colour target is reduced with the same kernel
    # The bound of tests/restore_ref.py for |x0| <= 1 (the loop clamps) and |y| <= 0.9, enlarged by the last row's c1 rounding: the
    # result is fl(c1[0] x0'), so a . x - y = c1 (a . x0' - y) + (c1 - 1) y + (one rounding of each c1 x0'_c).  Here c1[0] == 1.0
    # exactly (asserted), the product rounds nothing and the factor is 1: the bound itself.
    c1, c2, sg = (float(t[0]) for t in netG._step_rule()[0][2:5])
    assert (c1, c2, sg) == (1.0, 0.0, 0.0)
    bound = R.gray_bound(a, p, 1.0, 0.9)
    bound = abs(c1) * bound + abs(c1 - 1.0) * 0.9 + (0.0 if c1 == 1.0 else R.EPS * float(np.abs(a).sum()) * 3.0)
    res = outs[1].cpu().numpy().astype(np.float64)
    err = np.abs((a.astype(np.float64)[None, :, None, None] * res).sum(1, keepdims=True) - y.cpu().numpy().astype(np.float64)).max()
    print('%s %s: gray error %.3e (bound %.3e)' % (name, walk, err, bound))
    assert err <= bound
    # restore_error measures with sr3_gray_f32: one more fp32 channel sum (3 products, 2 sums of magnitude <= 1)
    assert X.restore_error(outs[1], netG.restore, y) <= bound + 3 * R.EPS * float(np.abs(a).sum()) * 3.0
    netG.set_restore(None)
    plain = _chain(netG, cond)
    assert float((X.gray_f32(plain, 'rec601') - y).abs().max()) > 1e-2      # the projection is what did it
    if name == 'sr3_tiny':      # a conditional model's default target: the conditioning image's gray
        netG.set_restore('gray', 1.0, 'rec601')
        out = _chain(netG, cond)
        ymax = float(X.gray_f32(cond, 'rec601').abs().max())
        assert X.restore_error(out, netG.restore, cond) <= R.gray_bound(a, p, 1.0, ymax) + 3 * R.EPS * float(np.abs(a).sum()) * 3.0


@pytest.mark.parametrize('name', MODELS)
def test_travelled_walk(name):
    """travel = {length: 2, repeats: 3} on 8 steps: 24 replays of the one captured step, reproducible from the same seeds, and equal to
    the eager walk; the known pixels still come back bit for bit"""
    d = G.dev()
    netG = _model(name, 'ddim')
    cond, known, shape = _inputs(name, d)
    B, Cc, H, W = shape
    mask = torch.zeros((B, 1, H, W), device=d)
    mask[:, :, H // 2:] = 1.0
    plain_mask = None
    for eta in (0.0, 1.0):          # (eta 0 draws nothing in a step: the jumps' z is the chain's only noise)
        netG.set_sampler(8, eta)
        netG.set_restore('mask')
        plain_mask = _chain(netG, cond, restore_target=(known, mask))
        netG.set_restore('mask', travel={'length': 2, 'repeats': 3})
        a = _chain(netG, cond, restore_target=(known, mask))
        st = next(reversed(netG._loop_cache.values()))
        assert st['replays'] == 24 and st['step'].tolist()[1] == -1 and len(st['rs_walk']) == 12
        b = _chain(netG, cond, restore_target=(known, mask))
        assert st['replays'] == 24 and torch.equal(a, b)
        netG.use_graph = False
        assert torch.equal(_chain(netG, cond, restore_target=(known, mask)), a)
        netG.use_graph = True
        mb = mask.expand(shape) == 1
        assert torch.equal(a[mb], known[mb]) and not torch.equal(a[~mb], plain_mask[~mb]) and bool(torch.isfinite(a).all())
    if name != 'ddpm_tiny':      # every snapshot of a travelled walk is an index's last visit: the shape is the plain walk's
        netG.set_restore('mask', travel={'length': 3, 'repeats': 2})
        out = netG.p_sample_loop(cond, continous=True, item_seeds=SEEDS, restore_target=(known, mask))
        assert out.shape[0] == B * (8 + 1)
    netG.set_sampler(8, 0.0)


def test_ddpm_under_ddim_first_step_is_forward_full_then_the_restatement():
    d = G.dev()
    netG = _model('ddpm_tiny', 'ddim')
    _, known, shape = _inputs('ddpm_tiny', d)
    B, Cc, H, W = shape
    S = 8
    tables, level, t_map, c3, noisy = netG._step_rule()
    assert t_map is not None and c3 is None and not noisy and t_map.tolist() != list(range(S))
    netG.set_restore('mask', 0.75)
    mask = torch.from_numpy(np.random.default_rng(8).uniform(size=(B, 1, H, W)).astype(F)).to(d)
    x_T = torch.from_numpy(load_golden('ddpm_tiny')[0]['loop/x_T']).to(d)
    netG.use_graph = False
    netG.p_sample_loop(shape, x_T=x_T, restore_target=(known, mask))
    st = next(reversed(netG._loop_cache.values()))
    st['img'].copy_(x_T)
    st['step'].fill_(S - 1)
    netG._one_step(st)
    torch.cuda.synchronize()
    assert st['step'].tolist() == [S - 1, S - 2]
    step = _ints([S - 1], d)
    eps = netG.denoise_fn(x_T, None, step_dev=step, full=True, t_map=t_map)
    assert tuple(eps.shape) == shape
    # ... which is the forward at the walk's timestep, not at the step index
    t = int(t_map[S - 1])
    assert t == 15 and torch.equal(eps, netG.denoise_fn(x_T, torch.full((B,), t, dtype=torch.long, device=d)))
    tabs = {k: v.cpu().numpy() for k, v in zip(R.KEYS, tables)}
    want, _ = R.restore_step(x_T.cpu().numpy(), eps.cpu().numpy(), None, 0, known.cpu().numpy(), mask.cpu().numpy(), None, None, 0.75, tabs,
                             S - 1, 1)
    _same(st['img'].cpu().numpy(), want, 'the first step of ddpm_tiny under ddim')
