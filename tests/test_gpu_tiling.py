"""Tiled sampling on the GPU (csrc/tiled.hip, EngineDiffusion.p_sample_loop_tiled): everything through the C ABI or the drop-in package,
references in float64 on the CPU (blend64 below restates the blend; this file keeps its own copy, so no other test module can move it).

Layout used throughout: image 28 x 36, tile 16, overlap 4 -> origins [0, 12] x [0, 10, 20], six tiles per image; the x origins sit off
every vector alignment."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util as G                                # noqa: E402
from helpers import SCHEDS, load_golden, opt_for      # noqa: E402
from sr3_hip import lib as L                        # noqa: E402
from sr3_hip.tiling import TileGrid                 # noqa: E402

GUARD = 4096      # floats of NaN behind a tensor, in the same allocation
H, W, TILE, OVERLAP = 28, 36, 16, 4


def blend64(tiles, grid, B):
    """float64 restatement of the blend of sr3_tiled_step: tiles [B * ny * nx, C, th, tw] -> (eps [B, C, H, W], cover count [H, W]).
    A pixel one tile covers takes that tile's value as it is; the others the weighted mean over the covering tiles."""
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
    return np.where(cnt == 1, one, num / den), cnt


def _guarded(t, dev, fill=None):
    """`t` (or a `fill`-filled tensor of its shape) on the device with GUARD NaNs behind it in ONE allocation: (view, whole buffer)."""
    n = t.numel()
    buf = torch.full((n + GUARD,), float('nan'), device=dev, dtype=t.dtype)
    if fill is None:
        buf[:n].copy_(t.reshape(-1))
    else:
        buf[:n].fill_(fill)
    return buf[:n].view(t.shape), buf


def _guard_intact(buf, n):
    return bool(torch.isnan(buf[n:]).all())


def _model(name='sr3_tiny'):
    import model as Model
    m = Model.create_model(opt_for(name, phase='val', gpu=True))
    _, sd = load_golden(name)
    m.netG.load_state_dict(sd, strict=True)
    m.netG.show_progress = False
    return m


def _ints(v, d):
    return torch.tensor(v, dtype=torch.int32, device=d)


def _gather(src, grid, first, n, dst):
    B, Cc, h, w = src.shape
    oy, ox = _ints(grid.oy, src.device), _ints(grid.ox, src.device)      # (held until the kernel has run: a freed one's memory is reused)
    L.check(L.load().sr3_tile_gather(L.ptr(src), B, Cc, h, w, L.ptr(oy), grid.ny, L.ptr(ox), grid.nx, first, n, grid.th, grid.tw,
                                     L.ptr(dst), G.stream()))
    torch.cuda.synchronize()


def _tiled_step(x, eps_tiles, grid, z, tables, step2, clip, eps_out, host=True):
    d = x.device
    B, Cc, h, w = x.shape
    oy, ox = _ints(grid.oy, d), _ints(grid.ox, d)
    wy, wx = torch.from_numpy(grid.wy).to(d), torch.from_numpy(grid.wx).to(d)
    hy, hx = (C.c_int * grid.ny)(*grid.oy), (C.c_int * grid.nx)(*grid.ox)
    rc = L.load().sr3_tiled_step(L.ptr(x), L.ptr(eps_tiles), B, Cc, h, w, L.ptr(oy), grid.ny, L.ptr(ox), grid.nx, L.ptr(wy), L.ptr(wx),
                                 grid.th, grid.tw, hy if host else None, hx if host else None, L.ptr(z), *[L.ptr(t) for t in tables],
                                 L.ptr(step2), clip, L.ptr(eps_out), G.stream())
    torch.cuda.synchronize()
    return rc


def _tables(netG):
    return (netG.sqrt_recip_alphas_cumprod, netG.sqrt_recipm1_alphas_cumprod, netG.posterior_mean_coef1, netG.posterior_mean_coef2,
            netG._sigma)


def _tail64(x, eps, z, tables, j, clip):
    a, b, c1, c2, sg = (float(t[j].item()) for t in tables)
    x = x.double().cpu().numpy()
    x0 = a * x - b * eps
    if clip:
        x0 = np.clip(x0, -1.0, 1.0)
    return c1 * x0 + c2 * x + sg * (0.0 if z is None else z.double().cpu().numpy())


def _close(got, ref, what):
    """the project's per-step tolerance (gpu_util.assert_close's default): 2e-5 * max(1, |ref|_inf)"""
    ref = np.asarray(ref)
    err = float(np.abs(got.double().cpu().numpy() - ref).max())
    tol = 2e-5 * max(1.0, float(np.abs(ref).max()))
    print('%s: max abs err %.3e (tolerance %.3e)' % (what, err, tol))
    assert err <= tol, '%s: %g > %g' % (what, err, tol)
    return err


@pytest.fixture(scope='module')
def tables():
    """the five schedule tables of sr3_tiny on the device (the model that owns them stays alive with the fixture)"""
    netG = _model().netG
    yield _tables(netG)


# ---- 1. the gather ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('first,n', [(0, 12), (0, 5), (5, 7)])
def test_gather_is_a_bit_copy(first, n):
    d = G.dev()
    grid = TileGrid(H, W, TILE, TILE, OVERLAP)
    assert (grid.oy, grid.ox) == ([0, 12], [0, 10, 20])
    B, Cc = 2, 3
    src = torch.randn(B, Cc, H, W, generator=torch.Generator().manual_seed(1)).to(d)
    dst, buf = _guarded(torch.empty(n, Cc, TILE, TILE), d, fill=float('nan'))
    _gather(src, grid, first, n, dst)
    want = torch.stack([src[(b,) + (slice(None),) + grid.slices(iy, ix)] for b, iy, ix in map(grid.tile_of, range(first, first + n))])
    assert torch.equal(dst, want)
    assert _guard_intact(buf, dst.numel()), 'the kernel wrote behind the tile batch'


def test_gather_scalar_path_and_refusals():
    """a tile width that is no multiple of 4 (the one-element kernel), and what the entry refuses before it launches anything"""
    d = G.dev()
    grid = TileGrid(10, 15, 6, 7, 2)
    src = torch.randn(2, 3, 10, 15, generator=torch.Generator().manual_seed(2)).to(d)
    n = 2 * grid.n_tiles
    dst, buf = _guarded(torch.empty(n, 3, grid.th, grid.tw), d, fill=float('nan'))
    _gather(src, grid, 0, n, dst)
    want = torch.stack([src[(b,) + (slice(None),) + grid.slices(iy, ix)] for b, iy, ix in map(grid.tile_of, range(n))])
    assert torch.equal(dst, want) and _guard_intact(buf, dst.numel())
    lib = L.load()
    oy, ox = _ints(grid.oy, d), _ints(grid.ox, d)
    keep = dst.clone()
    for args, code in (((None, 2, 3, 10, 15, L.ptr(oy), grid.ny, L.ptr(ox), grid.nx, 0, n, 6, 7, L.ptr(dst)), -1),
                       ((L.ptr(src), 2, 3, 10, 15, L.ptr(oy), grid.ny, L.ptr(ox), grid.nx, 0, n + 1, 6, 7, L.ptr(dst)), -1),
                       ((L.ptr(src), 2, 3, 10, 15, L.ptr(oy), grid.ny, L.ptr(ox), grid.nx, -1, 2, 6, 7, L.ptr(dst)), -1),
                       ((L.ptr(src), 2, 3, 10, 15, L.ptr(oy), grid.ny, L.ptr(ox), grid.nx, 0, n, 11, 7, L.ptr(dst)), -1),
                       ((L.ptr(src), 1 << 16, 3, 1 << 8, 1 << 8, L.ptr(oy), grid.ny, L.ptr(ox), grid.nx, 0, n, 6, 7, L.ptr(dst)), -2)):
        assert lib.sr3_tile_gather(*args, G.stream()) == code, args
        assert lib.sr3_last_error()
    torch.cuda.synchronize()
    assert torch.equal(dst, keep)


# ---- 2. the fused tail ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def tail_case():
    g = torch.Generator().manual_seed(3)
    grid = TileGrid(H, W, TILE, TILE, OVERLAP)
    B, Cc = 2, 3
    x = torch.randn(B, Cc, H, W, generator=g)
    eps_tiles = torch.randn(B * grid.n_tiles, Cc, TILE, TILE, generator=g)
    z = torch.randn(B, Cc, H, W, generator=g)
    eps64, cnt = blend64(eps_tiles.numpy(), grid, B)
    return grid, x, eps_tiles, z, eps64, cnt


@pytest.mark.parametrize('with_z', [True, False])
@pytest.mark.parametrize('clip', [0, 1])
@pytest.mark.parametrize('j', [0, 3, 7])
def test_fused_tail_against_float64(tail_case, tables, j, clip, with_z):
    d = G.dev()
    grid, x, eps_tiles, z, eps64, cnt = tail_case
    et = eps_tiles.to(d)
    zd = z.to(d) if with_z else None
    outs = []
    for run in range(2):
        xd, xbuf = _guarded(x, d)
        eo, ebuf = _guarded(torch.empty_like(x), d, fill=float('nan'))
        step2 = _ints([-7, j], d)
        assert _tiled_step(xd, et, grid, zd, tables, step2, clip, eo) == 0
        assert int(step2[1].item()) == j - 1
        assert _guard_intact(xbuf, xd.numel()) and _guard_intact(ebuf, eo.numel())
        outs.append((xd.clone(), eo.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), 'two runs on the same inputs differ'
    got_x, got_eps = outs[0]
    _close(got_eps, eps64, 'blended eps')
    _close(got_x, _tail64(x, eps64, zd, tables, j, clip), 'x after the step (j = %d, clip %d, z %s)' % (j, clip, with_z))
    # a pixel one tile covers carries that tile's eps bit for bit
    single = torch.from_numpy(cnt == 1)
    assert single.any() and not single.all()
    exact = torch.from_numpy(eps64).float()          # (where one tile covers, blend64 holds the fp32 value itself)
    assert torch.equal(got_eps.cpu()[:, :, single], exact[:, :, single])


def test_fused_tail_scalar_path(tables):
    """an image width that is no multiple of 4 takes the one-pixel kernel: same arithmetic"""
    d = G.dev()
    g = torch.Generator().manual_seed(4)
    grid = TileGrid(10, 15, 6, 7, 2)
    B, Cc = 2, 3
    x = torch.randn(B, Cc, 10, 15, generator=g)
    eps_tiles = torch.randn(B * grid.n_tiles, Cc, grid.th, grid.tw, generator=g)
    z = torch.randn(B, Cc, 10, 15, generator=g)
    xd, xbuf = _guarded(x, d)
    eo, ebuf = _guarded(torch.empty_like(x), d, fill=float('nan'))
    step2 = _ints([0, 5], d)
    assert _tiled_step(xd, eps_tiles.to(d), grid, z.to(d), tables, step2, 1, eo) == 0
    eps64, _ = blend64(eps_tiles.numpy(), grid, B)
    _close(eo, eps64, 'blended eps (scalar path)')
    _close(xd, _tail64(x, eps64, z, tables, 5, 1), 'x after the step (scalar path)')
    assert step2.tolist() == [5, 4] and _guard_intact(xbuf, xd.numel()) and _guard_intact(ebuf, eo.numel())


def test_fused_tail_refusals_launch_nothing(tables):
    d = G.dev()
    grid = TileGrid(H, W, TILE, TILE, OVERLAP)
    B, Cc = 1, 3
    x = torch.randn(B, Cc, H, W, device=d)
    keep = x.clone()
    et = torch.randn(B * grid.n_tiles, Cc, TILE, TILE, device=d)
    step2 = _ints([0, 3], d)
    lib = L.load()
    assert _tiled_step(x, None, grid, None, tables, step2, 1, None) == -1 and b'null' in lib.sr3_last_error()
    assert _tiled_step(x, et, grid, None, tables, None, 1, None) == -1

    class Bad(object):      # a grid with one field replaced
        def __init__(self, **kw):
            self.__dict__.update(grid.__dict__)
            self.__dict__.update(kw)
    assert _tiled_step(x, et, Bad(th=H + 4), None, tables, step2, 1, None) == -1 and b'larger than the image' in lib.sr3_last_error()
    assert _tiled_step(x, et, Bad(tw=W + 4), None, tables, step2, 1, None) == -1
    for oy in ([0, 12, 12], [4, 12], [0, 8], [12, 0]):
        assert _tiled_step(x, et, Bad(oy=oy, ny=len(oy)), None, tables, step2, 1, None) == -1, oy
        assert b'origins' in lib.sr3_last_error()
    assert _tiled_step(x, et, Bad(ox=[0, 20], nx=2), None, tables, step2, 1, None) == -1 and b'gap' in lib.sr3_last_error()
    oy, ox = _ints(grid.oy, d), _ints(grid.ox, d)
    wy, wx = torch.from_numpy(grid.wy).to(d), torch.from_numpy(grid.wx).to(d)
    rc = lib.sr3_tiled_step(L.ptr(x), L.ptr(et), 1 << 12, 2, 1 << 9, 1 << 9, L.ptr(oy), 2, L.ptr(ox), 3, L.ptr(wy), L.ptr(wx), 16, 16, None,
                            None, None, *[L.ptr(t) for t in tables], L.ptr(step2), 1, None, G.stream())
    assert rc == -2 and b'2^31' in lib.sr3_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, keep) and step2.tolist() == [0, 3]


# ---- 3. one tile is today's step ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('clip', [0, 1])
def test_one_tile_is_todays_step_bit_for_bit(tables, clip):
    d = G.dev()
    g = torch.Generator().manual_seed(5)
    B, Cc, h, w = 3, 3, 16, 24
    grid = TileGrid(h, w, h, w, 0)
    assert grid.n_tiles == 1
    x = torch.randn(B, Cc, h, w, generator=g).to(d)
    eps = torch.randn(B, Cc, h, w, generator=g).to(d)
    z = torch.randn(B, Cc, h, w, generator=g).to(d)
    for j in (0, 4):
        a, step_a = x.clone(), _ints([0, j], d)
        assert _tiled_step(a, eps, grid, z, tables, step_a, clip, None) == 0
        b, step_b = x.clone(), _ints([0, j], d)
        lib = L.load()
        L.check(lib.sr3_p_sample_step_ex(L.ptr(b), L.ptr(eps), L.ptr(z), *[L.ptr(t) for t in tables], L.ptr(step_b[1:]), None, 0, B,
                                         Cc * h * w, clip, G.stream()))
        L.check(lib.sr3_step_decrement(L.ptr(step_b[1:]), G.stream()))
        torch.cuda.synchronize()
        assert torch.equal(a, b) and int(step_a[1].item()) == int(step_b[1].item()) == j - 1


# ---- 4. the degenerate loop -----------------------------------------------------------------------------------------------------

def test_degenerate_loop_is_the_plain_loop():
    d = G.dev()
    netG = _model().netG
    g, _ = load_golden('sr3_rect')
    sr, x_T, zs = (torch.from_numpy(g['16x24/loop/' + n]).to(d) for n in ('sr', 'x_T', 'zs'))
    plain = netG.p_sample_loop(sr, continous=True, x_T=x_T, noise_seq=zs)
    tiled = netG.p_sample_loop_tiled(sr, continous=True, tile=(16, 24), overlap=0, x_T=x_T, noise_seq=zs)
    assert torch.equal(tiled, plain)
    ref = torch.from_numpy(g['16x24/loop/ret_continous'])
    assert tiled.shape == ref.shape and (tiled.cpu() - ref).abs().max().item() <= 1e-4
    # a tile larger than the image is the same single tile
    assert torch.equal(netG.p_sample_loop_tiled(sr, continous=True, tile=32, overlap=0, x_T=x_T, noise_seq=zs), plain)
    # the captured form, fixed seed
    torch.manual_seed(11)
    a = netG.p_sample_loop_tiled(sr, continous=True, tile=(16, 24), overlap=0)
    torch.manual_seed(11)
    b = netG.p_sample_loop(sr, continous=True)
    assert torch.equal(a, b)
    assert any(k[-1] is not None and v['graph'] is not None for k, v in netG._loop_cache.items())


# ---- 5. the tiled step against its parts -----------------------------------------------------------------------------------------

def _last_state(netG):
    return next(reversed(netG._loop_cache.values()))


def _parts_step(netG, st, x, cond, z, j, grid):
    """One step's expectation from its parts: eps per tile from the existing forward at batch 1 on the sliced tile, the float64
    blend, the float64 tail.  x, cond, z: the engine's own state before the step (device tensors)."""
    B = x.shape[0]
    tiles = np.empty((B * grid.n_tiles,) + (x.shape[1], grid.th, grid.tw))
    for b in range(B):
        for iy in range(grid.ny):
            for ix in range(grid.nx):
                sy, sx = grid.slices(iy, ix)
                xt = x[b:b + 1, :, sy, sx].contiguous()
                ct = None if cond is None else cond[b:b + 1, :, sy, sx].contiguous()
                tiles[grid.tile_index(b, iy, ix)] = netG._eps(xt, j, ct)[0].double().cpu().numpy()
    eps64, _ = blend64(tiles, grid, B)
    return eps64, _tail64(x, eps64, z, _tables(netG), j, True)


def test_tiled_step_against_its_parts_and_chunkings_agree():
    d = G.dev()
    netG = _model().netG
    T = SCHEDS['sr3_tiny']['n_timestep']
    g = torch.Generator().manual_seed(6)
    B = 2
    cond = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).to(d)
    x_T = torch.randn(B, 3, H, W, generator=g).to(d)
    zs = torch.randn(T, B, 3, H, W, generator=g).to(d)
    grid = TileGrid(H, W, TILE, TILE, OVERLAP, 4)
    ends = {}
    for tb in (5, 12, 1):
        out = netG.p_sample_loop_tiled(cond, continous=True, tile=TILE, overlap=OVERLAP, tile_batch=tb, x_T=x_T, noise_seq=zs)
        assert out.shape == (B * (T + 1), 3, H, W)          # (T = 8: every step is a snapshot)
        ends[tb] = out
        st = _last_state(netG)
        assert [n for _, n in st['chunks']] == {5: [5, 5, 2], 12: [12], 1: [1] * 12}[tb]
    # teacher forcing over the tile_batch = 5 chain: state before step i = snapshot of the step before it
    out = ends[5]
    for k, i in enumerate(reversed(range(T))):
        before = x_T if k == 0 else out[k * B:(k + 1) * B]
        z = zs[i] if i > 0 else None
        eps64, x64 = _parts_step(netG, None, before, cond, z, i, grid)
        _close(out[(k + 1) * B:(k + 2) * B], x64, 'step %d' % i)
    for tb in (12, 1):
        drift = (ends[tb] - ends[5])[-B:].abs().max().item()
        print('tile_batch %d against 5: final drift %.2e' % (tb, drift))
        assert drift <= 1e-4, (tb, drift)


# ---- 6. captured against eager ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('sampler', [None, (4, 0.0), (4, 1.0)])
def test_captured_chain_equals_eager(sampler):
    d = G.dev()
    netG = _model().netG
    if sampler is not None:
        netG.set_sampler(*sampler)
    cond = (torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(7)) * 2 - 1).to(d)
    outs = []
    for use_graph in (True, False):
        netG.use_graph = use_graph
        torch.manual_seed(21)
        outs.append(netG.p_sample_loop_tiled(cond, continous=True, tile=TILE, overlap=OVERLAP, tile_batch=5))
    steps = SCHEDS['sr3_tiny']['n_timestep'] if sampler is None else sampler[0]
    n_snap = sum(1 for i in range(steps) if i % (1 | (steps // 10)) == 0)
    assert outs[0].shape == (2 * (1 + n_snap), 3, H, W) and bool(torch.isfinite(outs[0]).all())
    assert torch.equal(outs[0], outs[1])
    st = _last_state(netG)
    assert st['graph'] is not None and st['step'].tolist()[1] == -1
    if sampler is not None:
        assert st['z_used'] == (sampler[1] > 0.0)


# ---- 7. per-item streams ---------------------------------------------------------------------------------------------------------

def test_item_streams_do_not_depend_on_the_batch():
    """tile_batch = 6 = the tiles of one image: in the batch of two and alone, image 0's tiles are one chunk of six at the same
    positions, so the plan builds the same launch list (the kernel choice depends on the geometry and the batch, both equal) and
    every kernel of it computes an image's values from that image alone in a fixed order -- bitwise equal, no tolerance needed."""
    d = G.dev()
    netG = _model().netG
    cond = (torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(8)) * 2 - 1).to(d)
    both = netG.p_sample_loop_tiled(cond, continous=True, tile=TILE, overlap=OVERLAP, tile_batch=6, item_seeds=[101, 202])
    alone = netG.p_sample_loop_tiled(cond[:1], continous=True, tile=TILE, overlap=OVERLAP, tile_batch=6, item_seeds=[101])
    assert torch.equal(both[0::2], alone)
    assert not torch.equal(both[-2], both[-1])


# ---- 8. the DDPM variant ----------------------------------------------------------------------------------------------------------

def test_ddpm_tiny_tiled():
    d = G.dev()
    netG = _model('ddpm_tiny').netG
    T = SCHEDS['ddpm_tiny']['n_timestep']
    shape = (2, 3, 24, 24)
    torch.manual_seed(31)
    out = netG.p_sample_loop_tiled(shape, tile=16, overlap=8)
    assert tuple(out.shape) == shape and bool(torch.isfinite(out).all())
    grid = TileGrid(24, 24, 16, 16, 8, 2)
    assert (grid.oy, grid.ox) == ([0, 8], [0, 8])
    # step-wise parity over the first two steps, driving the loop's own state
    st = _last_state(netG)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(shape, generator=g).to(d)
    st['img'].copy_(x)
    st['step'].fill_(T - 1)
    for i in (T - 1, T - 2):
        z = torch.randn(shape, generator=g).to(d)
        st['z'].copy_(z)
        before = st['img'].clone()
        netG._one_step(st, draw_noise=False)
        torch.cuda.synchronize()
        got, got_eps = st['img'].clone(), st['eps'].clone()
        assert int(st['step'][1].item()) == i - 1
        eps64, x64 = _parts_step(netG, st, before, None, z, i, grid)
        _close(got_eps, eps64, 'ddpm eps, step %d' % i)
        _close(got, x64, 'ddpm x, step %d' % i)
    netG.set_sampler(3, 0.0)
    with pytest.raises(NotImplementedError, match='t_map'):
        netG.p_sample_loop_tiled(shape, tile=16, overlap=8)


# ---- 9. the drop-in ----------------------------------------------------------------------------------------------------------------

def test_dropin_routes_large_items_through_the_tiled_loop():
    import model as Model
    d = G.dev()
    opt = opt_for('sr3_tiny', phase='val', gpu=True)
    opt['model']['beta_schedule']['val']['tiling'] = {'tile': 16, 'overlap': 4, 'batch': 4}
    m = Model.create_model(opt)
    _, sd = load_golden('sr3_tiny')
    m.netG.load_state_dict(sd, strict=True)
    m.netG.show_progress = False
    m.set_new_noise_schedule(opt['model']['beta_schedule']['val'], schedule_phase='val')
    assert m.netG.tiling == dict(tile=(16, 16), overlap=4, batch=4)
    T = SCHEDS['sr3_tiny']['n_timestep']
    n_snap = sum(1 for i in range(T) if i % (1 | (T // 10)) == 0)
    g = torch.Generator().manual_seed(10)
    big = torch.rand(1, 3, H, W, generator=g) * 2 - 1
    m.feed_data({'HR': big.clone(), 'SR': big})
    m.test(continous=True)
    assert tuple(m.SR.shape) == (1 + n_snap, 3, H, W) and bool(torch.isfinite(m.SR).all())
    assert torch.equal(m.SR[0].cpu(), big[0])
    assert [k[-1] for k in m.netG._loop_cache] == [((16, 16), 4, 4)]
    m.test(continous=False)
    assert tuple(m.SR.shape) == (3, H, W)
    small = torch.rand(1, 3, 16, 16, generator=g) * 2 - 1
    m.feed_data({'HR': small.clone(), 'SR': small})
    m.test(continous=True)
    assert tuple(m.SR.shape) == (1 + n_snap, 3, 16, 16)
    assert [k[-1] for k in m.netG._loop_cache] == [((16, 16), 4, 4), None]      # the plain loop's key carries no tiling
    # one axis inside the tile: a single tile on that axis, not a refusal
    wide = torch.rand(1, 3, 16, W, generator=g) * 2 - 1
    m.feed_data({'HR': wide.clone(), 'SR': wide})
    m.test(continous=False)
    assert tuple(m.SR.shape) == (3, 16, W) and bool(torch.isfinite(m.SR).all())
    st = next(reversed(m.netG._loop_cache.values()))
    assert (st['grid'].ny, st['grid'].nx, st['grid'].th) == (1, 3, 16)
    # refusals raise and leave the input as it was
    x = big.to(d)
    keep = x.clone()
    with pytest.raises(ValueError, match='overlap'):
        m.netG.p_sample_loop_tiled(x, tile=16, overlap=16)
    with pytest.raises(ValueError, match='multiples of 4'):
        m.netG.p_sample_loop_tiled(x, tile=18, overlap=4)
    with pytest.raises(ValueError):
        m.netG.p_sample_loop_tiled(x, tile=16, overlap=4, tile_batch=-2)
    assert torch.equal(x, keep)
