"""The second-order multistep sampler (DPM-Solver++(2M)) on the GPU: the tail with history through the three entries that carry it
(sr3_p_sample_step_hist, sr3_reverse_step_hist, sr3_tiled_step_hist) against torch-fp32 / float64 restatements and against each other,
the chain of p_sample_loop (graph replay, eager, a host float64 chain, the per-chain zero-fill of the history) and the refusals.
Tiny fixtures, batch 2 or 3; everything goes through the C ABI or the drop-in package.

The tail:  x0 = a x - b eps ; clamp(-1, 1) if clip ; x' = ((c1 x0 + c2 x) + c3 h) + sigma z ; h <- x0, every product and sum rounded
separately in fp32.  Tolerances: bit equality wherever two forms run the same operations; the project's per-step 2e-5 * max(1, |ref|_inf)
 against float64 where a UNet forward or a blend is involved; 1e-6 absolute for the bare op (worked out in its test)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import DESCS, CONDITIONAL, load_golden, opt_for              # noqa: E402
import gpu_util as G                                                     # noqa: E402
from sr3_hip import lib as L                                             # noqa: E402
from sr3_hip.tiling import TileGrid                                      # noqa: E402

GUARD = 1024      # floats of NaN behind a tensor, in the same allocation
NAMES = ['sr3_tiny', 'ddpm_tiny']
KEYS = ('a', 'b', 'c1', 'c2', 'sigma', 'c3')


def build(name, sampler=None):
    import model as Model
    opt = opt_for(name, phase='val', gpu=True)
    if sampler is not None:
        opt['model']['beta_schedule']['val']['sampler'] = sampler
    m = Model.create_model(opt)
    g, sd = load_golden(name)
    m.netG.load_state_dict(sd, strict=True)
    m.netG.show_progress = False
    if sampler is not None:
        m.set_new_noise_schedule(opt['model']['beta_schedule']['val'], schedule_phase='val')
    return m, g


def _guarded(t, dev):
    """`t` on the device with GUARD NaNs behind it in ONE allocation: (view, whole buffer)."""
    n = t.numel()
    buf = torch.full((n + GUARD,), float('nan'), device=dev, dtype=t.dtype)
    buf[:n].copy_(t.reshape(-1))
    return buf[:n].view(t.shape), buf


def _guard_intact(buf, n):
    return bool(torch.isnan(buf[n:]).all())


def _ints(v, d):
    return torch.tensor(v, dtype=torch.int32, device=d)


def _rows(tabs, t, like):
    """row t (an int, or one int per image) of every table, shaped to broadcast over `like`"""
    idx = torch.as_tensor(t, dtype=torch.long).reshape(-1)
    return {k: v[idx].reshape(-1, *([1] * (like.dim() - 1))) for k, v in tabs.items()}


def tail32(x, eps, z, h, tabs, t, clip):
    """The tail in torch fp32 on the CPU, one rounding per operation, in the kernels' association.  -> (x', h')"""
    r = _rows(tabs, t, x)
    x0 = r['a'] * x - r['b'] * eps
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    mean = r['c1'] * x0 + r['c2'] * x
    if h is not None:
        mean = mean + r['c3'] * h
    return mean + (torch.zeros_like(x) if z is None else z) * r['sigma'], x0


def tail64(x, eps, z, h, tabs, t, clip):
    """The same in float64 (of the fp32 tables and inputs)."""
    r = _rows({k: v.double() for k, v in tabs.items()}, t, x)
    x, eps = x.double(), eps.double()
    x0 = r['a'] * x - r['b'] * eps
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    out = r['c1'] * x0 + r['c2'] * x
    if h is not None:
        out = out + r['c3'] * h.double()
    if z is not None:
        out = out + r['sigma'] * z.double()
    return out, x0


def _step_hist(x, eps, z, tabs, clip, c3, hist, step_dev=None, tps=None, step_host=0):
    B = x.shape[0]
    rc = L.load().sr3_p_sample_step_hist(L.ptr(x), L.ptr(eps), L.ptr(z), *[L.ptr(tabs[k]) for k in KEYS[:5]], L.ptr(step_dev), L.ptr(tps),
                                         int(step_host), B, x[0].numel(), clip, L.ptr(c3), L.ptr(hist), G.stream())
    torch.cuda.synchronize()
    return rc


# ---- 1. the op ------------------------------------------------------------------------------------------------------------------

# four rows; |a|, |b| <= 0.9, the others <= 0.5 (the 1e-6 bound below rests on these magnitudes); c3 of both signs and one exact zero
OP_TABLES = dict(a=[0.9, 0.7, 0.85, 0.6], b=[0.8, 0.75, 0.5, 0.7], c1=[0.5, 0.45, -0.3, 0.4], c2=[0.3, 0.5, 0.45, -0.2],
                 sigma=[0.0, 0.4, 0.5, 0.25], c3=[0.0, -0.35, 0.5, -0.45])


@pytest.fixture(scope='module')
def op_case():
    tabs = {k: torch.tensor(v, dtype=torch.float32) for k, v in OP_TABLES.items()}
    cases = {}
    for shape in ((3, 3, 5, 7), (3, 3, 4, 8)):
        g = torch.Generator().manual_seed(sum(shape))
        x, z, h = ((0.5 * torch.randn(shape, generator=g)).clamp(-1.0, 1.0) for _ in range(3))
        eps = torch.randn(shape, generator=g).clamp(-2.0, 2.0)
        cases[shape] = (x, eps, z, h)
    return tabs, cases


@pytest.mark.parametrize('clip', [1, 0])
@pytest.mark.parametrize('with_z', [True, False])
@pytest.mark.parametrize('shape', [(3, 3, 5, 7), (3, 3, 4, 8)])
def test_op_against_fp32_and_float64(op_case, shape, with_z, clip):
    """sr3_p_sample_step_hist at 3 x 3 x 5 x 7 (105 elements per image: the one-element-per-thread form, images that start off every
    vector boundary) and 3 x 3 x 4 x 8 (the four-element form), the step taken from the host, from a device counter and per image:
    x' and hist bit-equal to the torch-fp32 restatement and within 1e-6 of float64.

    The 1e-6: |x|, |z|, |h| <= 1, |eps| <= 2 and the table magnitudes above bound every intermediate (a x 0.9, b eps 1.6, x0 2.5,
    c1 x0 1.25, c2 x 0.5, their sum 1.75, c3 h 0.5, the sum 2.25, sigma z 0.5, x' 2.75); one rounding is at most 2^-24 of its
    result, and x0's 3.0e-7 enters x' times |c1| <= 0.5: 1.5e-7 + 2^-24 * (1.25 + 0.5 + 1.75 + 0.5 + 2.25 + 0.5 + 2.75) = 7.2e-7 for x',
    3.0e-7 for hist."""
    d = G.dev()
    tabs, cases = op_case
    x, eps, z, h = cases[shape]
    if not with_z:
        z = None
    dt = {k: v.to(d) for k, v in tabs.items()}
    B = shape[0]
    lib = L.load()
    clipped = 0
    for mode, t in (('host', 2), ('dev', 1), ('per', [3, 0, 2])):
        xd, xbuf = _guarded(x, d)
        hd, hbuf = _guarded(h, d)
        ed, zd = eps.to(d), None if z is None else z.to(d)
        kw = dict(step_host=t) if mode == 'host' else dict(step_dev=_ints([t], d)) if mode == 'dev' else \
            dict(tps=torch.tensor(t, dtype=torch.int64, device=d))
        assert _step_hist(xd, ed, zd, dt, clip, dt['c3'], hd, **kw) == 0
        assert _guard_intact(xbuf, xd.numel()) and _guard_intact(hbuf, hd.numel())
        want_x, want_h = tail32(x, eps, z, h, tabs, t, clip)
        assert torch.equal(xd.cpu(), want_x), '%s: x differs from the fp32 restatement' % mode
        assert torch.equal(hd.cpu(), want_h), '%s: hist differs from the fp32 restatement' % mode
        x64, h64 = tail64(x, eps, z, h, tabs, t, clip)
        ex, eh = float((xd.cpu().double() - x64).abs().max()), float((hd.cpu().double() - h64).abs().max())
        print('%s %s z=%s clip=%d: |x - x64| %.2e, |hist - h64| %.2e' % (shape, mode, with_z, clip, ex, eh))
        assert ex <= 1e-6 and eh <= 1e-6
        r = _rows(tabs, t, x)
        clipped += int(((r['a'] * x - r['b'] * eps).abs() > 1.0).sum())
        if clip:
            assert float(hd.abs().max()) <= 1.0
        # without the history it is sr3_p_sample_step_ex, bit for bit
        xa, xb = x.to(d).clone(), x.to(d).clone()
        assert _step_hist(xa, ed, zd, dt, clip, None, None, **kw) == 0
        L.check(lib.sr3_p_sample_step_ex(L.ptr(xb), L.ptr(ed), L.ptr(zd), *[L.ptr(dt[k]) for k in KEYS[:5]], L.ptr(kw.get('step_dev')),
                                         L.ptr(kw.get('tps')), int(kw.get('step_host', 0)), B, x[0].numel(), clip, G.stream()))
        torch.cuda.synchronize()
        assert torch.equal(xa, xb) and torch.equal(xa.cpu(), tail32(x, eps, z, None, tabs, t, clip)[0])
    assert 0 < clipped < 3 * x.numel()                      # the clamp binds on part of the elements


def test_op_refusals_launch_nothing(op_case):
    d = G.dev()
    tabs, cases = op_case
    x, eps, z, h = (t.to(d) for t in cases[(3, 3, 4, 8)])
    dt = {k: v.to(d) for k, v in tabs.items()}
    keep_x, keep_e, keep_h = x.clone(), eps.clone(), h.clone()
    lib = L.load()
    n = x.numel()
    both = torch.cat([x.reshape(-1), x.reshape(-1)])          # a buffer to overlap x's twin partially
    for c3, hist, what in ((dt['c3'], None, b'together'), (None, h, b'together'), (dt['c3'], x, b'overlaps'), (dt['c3'], eps, b'overlaps')):
        assert _step_hist(x, eps, z, dt, 1, c3, hist, step_host=1) == -1
        assert what in lib.sr3_last_error()
    assert _step_hist(both[:n].view_as(x), eps, z, dt, 1, dt['c3'], both[n - 4:2 * n - 4].view_as(x), step_host=1) == -1
    assert b'overlaps' in lib.sr3_last_error()
    assert torch.equal(x, keep_x) and torch.equal(eps, keep_e) and torch.equal(h, keep_h) and torch.equal(both[:n], keep_x.reshape(-1))


# ---- 2. fused = unfused -----------------------------------------------------------------------------------------------------------

def _solver_tables(netG, d):
    """The tables of a 4-step dpmpp_2m sampler on the model's schedule, with a made-up sigma so that z matters."""
    netG.set_sampler(4, kind='dpmpp_2m')
    tabs = {k: getattr(netG, '_sampler_' + k) for k in KEYS}
    tabs['sigma'] = torch.tensor([0.0, 0.3, 0.2, 0.1], device=d)
    assert bool((tabs['c3'][1:-1] != 0).all())
    return tabs


@pytest.mark.parametrize('clip', [True, False])
@pytest.mark.parametrize('name', NAMES)
def test_reverse_step_hist_one_call_equals_three(name, clip):
    """sr3_reverse_step_hist (the history in the output conv's epilogue) against sr3_unet_forward + sr3_p_sample_step_hist +
    sr3_step_decrement on the same inputs, as tests/test_gpu_unet.py does for the step without history: eps, the new image, the history
    and the counter bit-equal at every step index of a 4-step walk (DDPM: conditioned through the t_map); and with neither c3 nor
    hist it is sr3_reverse_step_ex, bit for bit."""
    from sr3_hip import engine as E
    m, g = build(name)
    d = G.dev()
    netG, un = m.netG, m.netG.denoise_fn
    lib = L.load()
    cond = torch.from_numpy(g['loop/sr']).to(d) if CONDITIONAL[name] else None
    zs = torch.from_numpy(g['loop/zs']).to(d)
    xs = torch.from_numpy(g['step/x']).to(d)
    B = xs.shape[0]
    assert B == 2
    tabs = _solver_tables(netG, d)
    five = tuple(tabs[k] for k in KEYS[:5])
    level = netG._sampler_level
    ddpm = DESCS[name]['variant'] == 'ddpm'
    t_map = netG._sampler_tau if ddpm else None
    h0 = (0.5 * torch.randn(xs.shape, generator=torch.Generator().manual_seed(8))).to(d)
    for j in (3, 2, 1, 0):
        # three calls
        step1 = _ints([j], d)
        if ddpm:
            eps3 = un(xs, torch.full((B,), int(netG._sampler_tau[j]), dtype=torch.long, device=d), cond=cond)
        else:
            eps3 = un(xs, None, cond=cond, level_table=level, step_dev=step1)
        x3, h3 = xs.clone(), h0.clone()
        assert _step_hist(x3, eps3, zs[j], tabs, int(clip), tabs['c3'], h3, step_dev=step1) == 0
        L.check(lib.sr3_step_decrement(L.ptr(step1), G.stream()))
        # one call
        step2 = _ints([-77, j], d)
        x1, xbuf = _guarded(xs, d)
        h1, hbuf = _guarded(h0, d)
        eps1 = torch.full_like(xs, float('nan'))
        un.reverse_step(x1, zs[j], five, step2, cond=cond, level_table=level, clip_denoised=clip, eps_out=eps1, t_map=t_map,
                        c3=tabs['c3'], hist=h1)
        torch.cuda.synchronize()
        assert torch.equal(eps1, eps3), 'eps differs at step index %d' % j
        assert torch.equal(x1, x3), 'image differs at step index %d' % j
        assert torch.equal(h1, h3), 'history differs at step index %d' % j
        assert step2.tolist() == [j, j - 1] and step1.tolist() == [j - 1]
        assert _guard_intact(xbuf, x1.numel()) and _guard_intact(hbuf, h1.numel())
        # the history is this step's x0, and where c3 != 0 the incoming one moved the image
        want_x, want_h = tail32(xs.cpu(), eps3.cpu(), zs[j].cpu(), h0.cpu(), {k: v.cpu() for k, v in tabs.items()}, j, clip)
        assert torch.equal(h1.cpu(), want_h) and torch.equal(x1.cpu(), want_x)
        x_no = xs.clone()
        un.reverse_step(x_no, zs[j], five, _ints([0, j], d), cond=cond, level_table=level, clip_denoised=clip, t_map=t_map)
        assert torch.equal(x_no, x1) == (float(tabs['c3'][j]) == 0.0)
    # nulls: the new entry and the one that forwards to it, through the C ABI
    ws = E.Workspace()
    un.ensure_derived()
    wsbuf, need = ws.get(un.plan, B, d)
    cc = 0 if cond is None else cond.shape[1]
    outs = []
    for fn, extra in ((lib.sr3_reverse_step_ex, ()), (lib.sr3_reverse_step_hist, (None, None))):
        for j in (3, 1, 0):
            step2 = _ints([-77, j], d)
            x1, eps1 = xs.clone(), torch.full_like(xs, float('nan'))
            L.check(fn(un.plan.handle, L.ptr(x1), L.ptr(cond), cc, L.ptr(un.freq), L.ptr(level), L.ptr(step2), L.ptr(un.weights()),
                       L.ptr(wsbuf), need, L.ptr(zs[j]), *[L.ptr(t) for t in five], int(clip), L.ptr(eps1), B, G.stream(), L.ptr(t_map),
                       *extra))
            torch.cuda.synchronize()
            assert step2.tolist() == [j, j - 1]
            outs.append((x1, eps1))
    for (xa, ea), (xb, eb) in zip(outs[:3], outs[3:]):
        assert torch.equal(xa, xb) and torch.equal(ea, eb) and bool(torch.isfinite(xa).all())


def test_reverse_step_hist_refusals_launch_nothing():
    m, g = build('sr3_tiny')
    d = G.dev()
    netG, un = m.netG, m.netG.denoise_fn
    cond = torch.from_numpy(g['loop/sr']).to(d)
    xs = torch.from_numpy(g['step/x']).to(d)
    tabs = _solver_tables(netG, d)
    five = tuple(tabs[k] for k in KEYS[:5])
    x, h, eps = xs.clone(), torch.zeros_like(xs), torch.zeros_like(xs)
    step2 = _ints([-77, 2], d)
    for kw in (dict(c3=tabs['c3'], hist=None), dict(c3=None, hist=h), dict(c3=tabs['c3'], hist=x), dict(c3=tabs['c3'], hist=eps),
               dict(c3=tabs['c3'], hist=h[:1]), dict(c3=tabs['c3'], hist=h.double())):
        with pytest.raises(L.Sr3Error):
            un.reverse_step(x, None, five, step2, cond=cond, level_table=netG._sampler_level, eps_out=eps, **kw)
    torch.cuda.synchronize()
    assert torch.equal(x, xs) and step2.tolist() == [-77, 2] and not h.any() and not eps.any()


# ---- 3. tiled -----------------------------------------------------------------------------------------------------------------------

def blend64(tiles, grid, B):
    """float64 restatement of the blend of sr3_tiled_step (as in tests/test_gpu_tiling.py, which keeps its own copy): tiles
    [B * ny * nx, C, th, tw] -> eps [B, C, H, W].  A pixel one tile covers takes that tile's value as it is; the others the weighted
    mean over the covering tiles."""
    tiles = np.asarray(tiles, dtype=np.float64)
    Cc = tiles.shape[1]
    num = np.zeros((B, Cc, grid.H, grid.W))
    den = np.zeros((grid.H, grid.W))
    cnt = np.zeros((grid.H, grid.W), dtype=np.int64)
    one = np.zeros((B, Cc, grid.H, grid.W))
    w2 = np.outer(grid.wy.astype(np.float64), grid.wx.astype(np.float64))
    for iy in range(grid.ny):
        for ix in range(grid.nx):
            sy, sx = grid.slices(iy, ix)
            den[sy, sx] += w2
            cnt[sy, sx] += 1
            for b in range(B):
                t = tiles[grid.tile_index(b, iy, ix)]
                num[b, :, sy, sx] += w2 * t
                one[b, :, sy, sx] = t
    return np.where(cnt == 1, one, num / den)


def _tiled_step_hist(x, eps_tiles, grid, z, tabs, step2, clip, eps_out, c3, hist):
    d = x.device
    B, Cc, h, w = x.shape
    oy, ox = _ints(grid.oy, d), _ints(grid.ox, d)
    wy, wx = torch.from_numpy(grid.wy).to(d), torch.from_numpy(grid.wx).to(d)
    hy, hx = (C.c_int * grid.ny)(*grid.oy), (C.c_int * grid.nx)(*grid.ox)
    rc = L.load().sr3_tiled_step_hist(L.ptr(x), L.ptr(eps_tiles), B, Cc, h, w, L.ptr(oy), grid.ny, L.ptr(ox), grid.nx, L.ptr(wy), L.ptr(wx),
                                      grid.th, grid.tw, hy, hx, L.ptr(z), *[L.ptr(tabs[k]) for k in KEYS[:5]], L.ptr(step2), clip,
                                      L.ptr(eps_out), G.stream(), L.ptr(c3), L.ptr(hist))
    torch.cuda.synchronize()
    return rc


def _close(got, ref, what):
    """the project's per-step tolerance (tests/test_gpu_tiling.py's, gpu_util.assert_close's default): 2e-5 * max(1, |ref|_inf)"""
    ref = ref.double().cpu()
    err = float((got.double().cpu() - ref).abs().max())
    tol = 2e-5 * max(1.0, float(ref.abs().max()))
    print('%s: max abs err %.3e (tolerance %.3e)' % (what, err, tol))
    assert err <= tol, '%s: %g > %g' % (what, err, tol)


@pytest.fixture(scope='module')
def solver_tabs():
    netG = build('sr3_tiny')[0].netG
    yield _solver_tables(netG, G.dev())


@pytest.mark.parametrize('clip', [0, 1])
def test_one_tile_with_history_is_the_untiled_pair_bit_for_bit(solver_tabs, clip):
    d = G.dev()
    tabs = solver_tabs
    g = torch.Generator().manual_seed(5)
    B, Cc, h, w = 3, 3, 16, 24
    grid = TileGrid(h, w, h, w, 0)
    assert grid.n_tiles == 1
    x, eps, z, h0 = (torch.randn(B, Cc, h, w, generator=g).to(d) for _ in range(4))
    lib = L.load()
    for j in (0, 2):
        a, ha, step_a = x.clone(), h0.clone(), _ints([0, j], d)
        assert _tiled_step_hist(a, eps, grid, z, tabs, step_a, clip, None, tabs['c3'], ha) == 0
        b, hb, step_b = x.clone(), h0.clone(), _ints([0, j], d)
        assert _step_hist(b, eps, z, tabs, clip, tabs['c3'], hb, step_dev=step_b[1:]) == 0
        L.check(lib.sr3_step_decrement(L.ptr(step_b[1:]), G.stream()))
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(ha, hb) and int(step_a[1].item()) == int(step_b[1].item()) == j - 1
        # and without the history the new entry is the old one
        a0, s0 = x.clone(), _ints([0, j], d)
        assert _tiled_step_hist(a0, eps, grid, z, tabs, s0, clip, None, None, None) == 0
        b0 = x.clone()
        L.check(lib.sr3_p_sample_step_ex(L.ptr(b0), L.ptr(eps), L.ptr(z), *[L.ptr(tabs[k]) for k in KEYS[:5]], None, None, j, B,
                                         Cc * h * w, clip, G.stream()))
        torch.cuda.synchronize()
        assert torch.equal(a0, b0)


@pytest.mark.parametrize('geometry', [(28, 36, 16, 16, 4), (10, 15, 6, 7, 2)])
@pytest.mark.parametrize('clip', [0, 1])
def test_tiled_step_with_history_against_float64(solver_tabs, clip, geometry):
    """a 2 x 3 grid of 16 x 16 tiles with overlap 4 (and a width that is no multiple of 4: the one-pixel kernel): the blend first, then
    the tail with history, against the float64 blend followed by the float64 tail"""
    d = G.dev()
    tabs = solver_tabs
    H, W, th, tw, ov = geometry
    grid = TileGrid(H, W, th, tw, ov)
    assert (grid.ny, grid.nx) == (2, 3) or W % 4
    B, Cc = 2, 3
    g = torch.Generator().manual_seed(3)
    x, z, h0 = (torch.randn(B, Cc, H, W, generator=g) for _ in range(3))
    eps_tiles = torch.randn(B * grid.n_tiles, Cc, grid.th, grid.tw, generator=g)
    eps64 = torch.from_numpy(blend64(eps_tiles.numpy(), grid, B))
    cpu_tabs = {k: v.cpu() for k, v in tabs.items()}
    for j in (2, 1):
        xd, xbuf = _guarded(x, d)
        hd, hbuf = _guarded(h0, d)
        eo = torch.full_like(xd, float('nan'))
        step2 = _ints([-7, j], d)
        assert _tiled_step_hist(xd, eps_tiles.to(d), grid, z.to(d), tabs, step2, clip, eo, tabs['c3'], hd) == 0
        assert step2.tolist() == [j, j - 1] and _guard_intact(xbuf, xd.numel()) and _guard_intact(hbuf, hd.numel())
        _close(eo, eps64, 'blended eps')
        x64, h64 = tail64(x, eps64, z, h0, cpu_tabs, j, clip)
        _close(xd, x64, 'x after the step (j = %d, clip %d)' % (j, clip))
        _close(hd, h64, 'history after the step (j = %d, clip %d)' % (j, clip))
        # the tail behind the blend is the op's, bit for bit, on the kernel's own blended eps
        want_x, want_h = tail32(x, eo.cpu(), z, h0, cpu_tabs, j, clip)
        assert torch.equal(xd.cpu(), want_x) and torch.equal(hd.cpu(), want_h)


def test_tiled_step_hist_refusals_launch_nothing(solver_tabs):
    d = G.dev()
    tabs = solver_tabs
    grid = TileGrid(28, 36, 16, 16, 4)
    x = torch.randn(1, 3, 28, 36, device=d)
    keep = x.clone()
    et = torch.randn(grid.n_tiles, 3, 16, 16, device=d)
    h, eo = torch.zeros_like(x), torch.zeros_like(x)
    step2 = _ints([0, 2], d)
    lib = L.load()
    for c3, hist, code, what in ((tabs['c3'], None, -1, b'together'), (None, h, -1, b'together'), (tabs['c3'], x, -1, b'overlaps'),
                                 (tabs['c3'], eo, -1, b'overlaps')):
        assert _tiled_step_hist(x, et, grid, None, tabs, step2, 1, eo, c3, hist) == code
        assert what in lib.sr3_last_error()
    assert torch.equal(x, keep) and step2.tolist() == [0, 2] and not h.any() and not eo.any()


# ---- 4. the chain -------------------------------------------------------------------------------------------------------------------

def _record_steps(netG):
    """wrap netG._one_step: after every step keep (eps, image, history) of the state"""
    log, one = [], netG._one_step

    def rec(st, draw_noise=True):
        one(st, draw_noise)
        log.append((st['eps'].clone(), st['img'].clone(), st['hist'].clone()))
    netG._one_step = rec
    return log, one


@pytest.mark.parametrize('name', NAMES)
def test_chain_graph_eager_float64_and_zero_fill(name):
    """p_sample_loop under {"type": "dpmpp_2m", "steps": 6}: the eager loop against a host float64 chain that applies the float64 tail
    to the engine's own per-step eps (per-step tolerance, every step and the result), the replayed graph against the eager loop bit
    for bit, and a second chain on the cached state -- its history filled with NaN in between -- giving the same bytes."""
    S = 6
    m, g = build(name, sampler={'type': 'dpmpp_2m', 'steps': S})
    d = G.dev()
    netG = m.netG
    assert netG.sampler == dict(type='dpmpp_2m', steps=S, eta=0.0, walk='logsnr')
    assert bool((netG._sampler_c3[1:-1] != 0).all())
    cond = torch.from_numpy(g['loop/sr']).to(d) if CONDITIONAL[name] else None
    x_T = torch.from_numpy(g['loop/x_T']).to(d)
    arg = cond if cond is not None else tuple(x_T.shape)
    whole = lambda out: out if (cond is None and DESCS[name]['variant'] == 'ddpm') else out[-2:]
    # eager, recorded
    netG.use_graph = False
    log, one = _record_steps(netG)
    eager = netG.p_sample_loop(arg, continous=True, x_T=x_T).clone()
    netG._one_step = one
    assert len(log) == S and torch.equal(whole(eager), log[-1][1])
    tabs = {k: getattr(netG, '_sampler_' + k).cpu() for k in KEYS}
    x64, h64 = x_T.cpu().double(), torch.zeros(x_T.shape, dtype=torch.float64)
    for k, j in enumerate(reversed(range(S))):
        eps, img, hist = log[k]
        x64, h64 = tail64(x64, eps.cpu(), None, h64, tabs, j, True)
        _close(img, x64, '%s image after step index %d' % (name, j))
        _close(hist, h64, '%s history after step index %d' % (name, j))
    # the history matters: the same walk without it (DDIM) ends elsewhere
    netG.set_sampler(S, walk='logsnr')
    ddim = netG.p_sample_loop(arg, continous=True, x_T=x_T).clone()
    assert not torch.equal(whole(ddim), whole(eager))
    # graph replay
    netG.set_sampler(S, kind='dpmpp_2m')
    netG.use_graph = True
    first = netG.p_sample_loop(arg, continous=True, x_T=x_T).clone()
    st = next(iter(netG._loop_cache.values()))
    assert len(netG._loop_cache) == 1 and st['graph'] is not None and st['step'].tolist() == [0, -1]
    assert torch.equal(first, eager) and bool(torch.isfinite(first).all())
    # the zero-fill: whatever the last chain left in the history does not reach the next one
    st['hist'].fill_(float('nan'))
    again = netG.p_sample_loop(arg, continous=True, x_T=x_T)
    assert next(iter(netG._loop_cache.values())) is st
    assert torch.equal(again, first)


def test_tiled_chain_under_the_multistep_sampler():
    """SR3 tiles under the new sampler: with one tile of the image's size the tiled loop is the plain loop bit for bit; on a 2 x 3 grid
    the replayed graph equals the eager loop and a NaN-filled history between two chains changes nothing."""
    m, _ = build('sr3_tiny', sampler={'type': 'dpmpp_2m', 'steps': 5})
    d = G.dev()
    netG = m.netG
    g = torch.Generator().manual_seed(6)
    sr = (torch.rand(2, 3, 16, 24, generator=g) * 2 - 1).to(d)
    x_T = torch.randn(2, 3, 16, 24, generator=g).to(d)
    plain = netG.p_sample_loop(sr, continous=True, x_T=x_T).clone()
    tiled = netG.p_sample_loop_tiled(sr, continous=True, tile=(16, 24), overlap=0, x_T=x_T)
    assert torch.equal(tiled, plain) and bool(torch.isfinite(plain).all())
    cond = (torch.rand(2, 3, 28, 36, generator=g) * 2 - 1).to(d)
    x_T = torch.randn(2, 3, 28, 36, generator=g).to(d)
    outs = []
    for use_graph in (False, True):
        netG.use_graph = use_graph
        outs.append(netG.p_sample_loop_tiled(cond, continous=True, tile=16, overlap=4, tile_batch=5, x_T=x_T).clone())
    st = next(reversed(netG._loop_cache.values()))
    assert st.get('grid') is not None and st['graph'] is not None and st['hist'].shape == x_T.shape
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[1]).all())
    st['hist'].fill_(float('nan'))
    assert torch.equal(netG.p_sample_loop_tiled(cond, continous=True, tile=16, overlap=4, tile_batch=5, x_T=x_T), outs[1])


def test_ddpm_tiles_under_the_multistep_sampler_are_refused():
    m, g = build('ddpm_tiny', sampler={'type': 'dpmpp_2m', 'steps': 4})
    netG = m.netG
    assert netG.sampler['type'] == 'dpmpp_2m'
    with pytest.raises(NotImplementedError):
        netG.p_sample_loop_tiled((2, 3, 28, 36), tile=16, overlap=4)
    with pytest.raises(NotImplementedError):
        netG.set_tiling(16, 4)
    assert netG._loop_cache == {} and netG.tiling is None
