"""Tiled sampling without a device: the tile layout (sr3_hip.tiling), the blend as a float64 restatement, and the config plumbing
("tiling" in a phase's beta_schedule block / set_tiling)."""
import numpy as np
import pytest
import torch

from helpers import SCHEDS, opt_for


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


def test_axis_origins_exhaustive():
    from sr3_hip.tiling import axis_origins
    for L in range(4, 97, 4):
        for t in (8, 16, 24, 32):
            for o in range(t):
                org = axis_origins(L, t, o)
                n = len(org)
                if L <= t:
                    assert org == [0], (L, t, o)
                    continue
                assert org[0] == 0 and org[-1] == L - t, (L, t, o, org)
                assert all(b > a for a, b in zip(org, org[1:])), (L, t, o, org)
                covered = np.zeros(L, dtype=bool)
                for a in org:
                    covered[a:a + t] = True
                assert covered.all(), (L, t, o, org)
                assert all(a + t - b >= o for a, b in zip(org, org[1:])), (L, t, o, org)
                # minimal: n - 1 tiles of size t with overlaps >= o span at most t + (n - 2) (t - o) < L
                assert n >= 2 and t + (n - 2) * (t - o) < L, (L, t, o, org)


def test_axis_origins_pinned_and_refusals():
    from sr3_hip.tiling import axis_origins
    assert axis_origins(36, 16, 4) == [0, 10, 20]
    assert axis_origins(28, 16, 4) == [0, 12]
    assert axis_origins(16, 16, 4) == [0] and axis_origins(12, 16, 0) == [0]
    for bad in ((36, 16, 16), (36, 16, -1), (36, 0, 0), (36, 16.0, 4)):
        with pytest.raises(ValueError):
            axis_origins(*bad)


def test_axis_window():
    from sr3_hip.tiling import axis_window
    for t in (8, 16, 24, 32):
        for o in range(t):
            w = axis_window(t, o)
            assert w.dtype == np.float32 and w.shape == (t,)
            assert (w > 0).all() and (w <= 1).all()
            assert np.array_equal(w, w[::-1])
            i = np.arange(t)
            inner = (i >= o) & (t - 1 - i >= o)                  # at distance > o from both ends: i + 1 > o and t - i > o
            assert (w[inner] == 1).all()
            ref = np.minimum(1.0, np.minimum((i + 1.0) / (o + 1.0), (t - i) / (o + 1.0))).astype(np.float32)
            assert np.array_equal(w, ref)
        assert (axis_window(t, 0) == 1).all()


def test_tile_grid_layout_and_refusals():
    from sr3_hip.tiling import TileGrid, axis_window
    g = TileGrid(28, 36, 16, 16, 4, 4)
    assert (g.oy, g.ox, g.th, g.tw, g.ny, g.nx, g.n_tiles) == ([0, 12], [0, 10, 20], 16, 16, 2, 3, 6)
    assert np.array_equal(g.wy, axis_window(16, 4)) and np.array_equal(g.wx, axis_window(16, 4))
    assert [g.tile_index(b, iy, ix) for b in range(2) for iy in range(2) for ix in range(3)] == list(range(12))
    assert g.tile_of(7) == (1, 0, 1) and g.slices(1, 2) == (slice(12, 28), slice(20, 36))
    one = TileGrid(16, 36, 32, 16, 4, 4)             # the tile covers the height: one tile of the image's size on that axis
    assert (one.th, one.oy, one.ny, one.nx) == (16, [0], 1, 3) and (one.wy == 1).all()
    for bad in (dict(tile_h=16.0, tile_w=16), dict(tile_h=0, tile_w=16), dict(tile_h=-16, tile_w=16), dict(tile_h=True, tile_w=16)):
        with pytest.raises(ValueError):
            TileGrid(28, 36, overlap=4, divisor=4, **bad)
    with pytest.raises(ValueError, match='overlap'):
        TileGrid(28, 36, 16, 16, 16, 4)
    with pytest.raises(ValueError, match='multiples of 4'):
        TileGrid(28, 36, 18, 16, 4, 4)


@pytest.mark.parametrize('shape', [(28, 36, 16, 16, 4), (24, 24, 16, 16, 8), (40, 20, 16, 24, 0), (33, 47, 16, 12, 5)])
def test_blend_restatement(shape):
    from sr3_hip.tiling import TileGrid
    H, W, th, tw, o = shape
    g = TileGrid(H, W, th, tw, o)
    B, Cc = 2, 3
    # a constant field blends to the same constant
    for c in (1.0, -0.37, 123.456):
        out, cnt = blend64(np.full((B * g.n_tiles, Cc, g.th, g.tw), c), g, B)
        assert np.abs(out - c).max() <= 1e-15 * abs(c)
    assert cnt.min() >= 1 and (o == 0 or cnt.max() > 1)
    # tiles cut from one smooth field blend back to it
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    field = np.stack([np.stack([np.sin(0.11 * yy + b) * np.cos(0.07 * xx - c) + 0.01 * yy for c in range(Cc)]) for b in range(B)])
    tiles = np.empty((B * g.n_tiles, Cc, g.th, g.tw))
    for b in range(B):
        for iy in range(g.ny):
            for ix in range(g.nx):
                sy, sx = g.slices(iy, ix)
                tiles[g.tile_index(b, iy, ix)] = field[b, :, sy, sx]
    out, _ = blend64(tiles, g, B)
    assert np.abs(out - field).max() <= 1e-14


@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_config_key_and_set_tiling(name):
    import model as Model
    opt = opt_for(name, gpu=False)
    m = Model.create_model(opt)
    netG = m.netG
    assert netG.tiling is None
    keys = set(netG.state_dict().keys())
    val = opt['model']['beta_schedule']['val']
    val['tiling'] = {'tile': 16, 'overlap': 4, 'batch': 4}
    m.set_new_noise_schedule(val, schedule_phase='val')
    assert netG.tiling == dict(tile=(16, 16), overlap=4, batch=4) and netG._loop_cache == {}
    assert set(netG.state_dict().keys()) == keys
    m.set_new_noise_schedule(opt['model']['beta_schedule']['train'], schedule_phase='train')      # an absent key: whole-image steps
    assert netG.tiling is None
    val['tiling'] = {'tile': [16, 32]}
    m.set_new_noise_schedule(val, schedule_phase='val')
    assert netG.tiling == dict(tile=(16, 32), overlap=0, batch=None)
    m.set_new_noise_schedule(opt['model']['beta_schedule']['train'], schedule_phase='train')
    val['tiling'] = None                                                   # "tiling": null
    m.set_new_noise_schedule(val, schedule_phase='val')                    # (the reference's phase switch re-reads the block)
    assert netG.tiling is None
    div = netG.denoise_fn.plan.divisor
    for bad in ({'tile': 16, 'overlap': 16}, {'tile': 16, 'overlap': 20}, {'tile': 16 + div // 2, 'overlap': 0},
                {'tile': 16, 'overlap': 4, 'batch': -1}, {'tile': 16, 'overlap': 4, 'batch': 0}, {'overlap': 4}, {'tile': 0},
                {'tile': [16, 16, 16]}, {'tile': 16, 'overlap': -1}):
        with pytest.raises(ValueError):
            netG.set_new_noise_schedule(dict(SCHEDS[name], tiling=bad), torch.device('cpu'))
    # programmatic form
    netG._loop_cache['stale'] = object()
    netG.set_tiling(16, overlap=4, batch=2)
    assert netG.tiling == dict(tile=(16, 16), overlap=4, batch=2) and netG._loop_cache == {}
    with pytest.raises(ValueError):
        netG.set_tiling(16, overlap=16)
    assert netG.tiling == dict(tile=(16, 16), overlap=4, batch=2)
    netG.set_tiling(None)
    assert netG.tiling is None


def test_ddpm_tiling_under_a_sampler_is_not_implemented():
    import model as Model
    s = SCHEDS['ddpm_tiny']
    netG = Model.create_model(opt_for('ddpm_tiny', gpu=False)).netG
    with pytest.raises(NotImplementedError, match='t_map'):
        netG.set_new_noise_schedule(dict(s, sampler={'type': 'ddim', 'steps': 3}, tiling={'tile': 16, 'overlap': 4}), torch.device('cpu'))
    netG.set_new_noise_schedule(dict(s), torch.device('cpu'))
    netG.set_tiling(16, 4)
    with pytest.raises(NotImplementedError):
        netG.set_sampler(3, 0.0)
    assert netG.sampler is None
    netG.set_tiling(None)
    netG.set_sampler(3, 0.0)
    with pytest.raises(NotImplementedError):
        netG.set_tiling(16, 4)
    assert netG.tiling is None
    # the SR3 variant takes both
    sr3 = Model.create_model(opt_for('sr3_tiny', gpu=False)).netG
    sr3.set_new_noise_schedule(dict(SCHEDS['sr3_tiny'], sampler={'type': 'ddim', 'steps': 4}, tiling={'tile': 16, 'overlap': 4}),
                               torch.device('cpu'))
    assert sr3.sampler['steps'] == 4 and sr3.tiling['tile'] == (16, 16)
