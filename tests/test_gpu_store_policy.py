"""Plan option store_wt (csrc/sr3_common.h: store16): the 16-byte epilogue stores of the two Winograd kernels and of the split-K reduce
kernels written THROUGH L2 (buffer stores with sc1) instead of left dirty for the kernel boundary.  A store policy changes no value, so
every mask must give the BITS of mask 0: whole forwards at a geometry that reaches every family (and, ragged, the masked stores of both
overhangs), and the captured reverse step replayed three times -- each replay's kernels read what the kernels before them wrote through.
The Winograd kernels' dummy residual loads (a tile without a residual now reads one line, not the output it is about to write; the old
loads are a build macro) cannot be compared with the old build inside the suite: they are held, with the write-through stores on,
against the committed layer taps of the tiny networks at the tolerance of test_gpu_unet.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util as G                                # noqa: E402
from test_gpu_fullsize import make_opt              # noqa: E402
from test_gpu_unet import NAMES, build              # noqa: E402

# 32 x 32 images, 32 / 128 / 96 channels on 32^2 / 16^2 / 8^2 maps, attention at 16^2, batch 4: the two-workgroup Winograd kernel with and
# without split-K, its upsample form (one of them to 96 channels: the last 64-channel block half masked), the four-image 8 x 8 tile of the
# 8-wave kernel (split-K only, 96 channels), the split-K reduce with and without the fused GroupNorm fold
CFG = dict(which='sr3', in_channel=6, inner=32, groups=8, mults=[1, 4, 3], attn=[16], rb=1, size=32, cond=True)
B = 4
MASKS = [1, 2, 4, 7]
GEOMETRIES = {'native_32x32': (32, 32), 'ragged_24x40': (24, 40)}

_net = {}
_ref = {}


def _netG():
    if 'netG' not in _net:
        import model.networks as networks
        opt = make_opt(CFG, T=100)
        opt['phase'] = 'val'
        torch.manual_seed(23)
        netG = networks.define_G(opt).to(G.dev())
        netG.set_new_noise_schedule(opt['model']['beta_schedule']['val'], G.dev())
        netG.show_progress = False
        _net['netG'] = netG
    return _net['netG']


def _inputs(H, W):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, 6, H, W, generator=g).to(G.dev())
    lvl = (torch.rand(B, 1, generator=g) * 0.9 + 0.05).to(G.dev())
    return x, lvl


def _forward(mask, H, W):
    un = _netG().denoise_fn
    un.plan.set_geometry(H, W)
    un.plan.set_option('store_wt', mask)
    x, lvl = _inputs(H, W)
    return un(x, lvl).clone()


def _reference(geo):
    """The forward under store_wt = 0, once per geometry, with the launch list checked for the kernels this file is about."""
    if geo not in _ref:
        H, W = GEOMETRIES[geo]
        e0 = _forward(0, H, W)
        assert bool(torch.isfinite(e0).all())
        ops = [o for o in _netG().denoise_fn.plan.op_list(B) if o['kind'] == 50 and o['ksize'] == 3 and o['stride'] == 1]
        have = lambda **kw: any(all(o[k] == v for k, v in kw.items()) for o in ops)
        if geo == 'native_32x32':
            assert have(tile_cfg=13, ksplit=1, upsample=0) and any(o['tile_cfg'] == 13 and o['ksplit'] > 1 for o in ops)
            assert have(tile_cfg=13, upsample=1, cout=96) and any(o['tile_cfg'] == 13 and o['upsample'] and o['ksplit'] > 1 for o in ops)
            assert any(o['tile_cfg'] == 12 and o['h_out'] == 8 and o['cout'] == 96 and o['ksplit'] > 1 for o in ops)
        else:
            for h, w in ((24, 40), (12, 20), (6, 10)):           # overhang to the right; to the right and below (twice)
                assert have(tile_cfg=23, h_out=h, w_out=w)
            assert have(tile_cfg=23, upsample=1, cout=96) and any(o['tile_cfg'] == 23 and o['ksplit'] > 1 for o in ops)
        _ref[geo] = e0
    return _ref[geo]


@pytest.mark.parametrize('mask', MASKS)
@pytest.mark.parametrize('geo', list(GEOMETRIES))
def test_every_store_policy_gives_the_bits_of_plain_stores(geo, mask):
    e0 = _reference(geo)
    e = _forward(mask, *GEOMETRIES[geo])
    assert torch.equal(e, e0), 'store_wt = %d at %s: %d of %d elements differ, max %.3e' % (
        mask, geo, int((e != e0).sum()), e.numel(), float((e - e0).abs().max()))


def test_fused_folds_are_part_of_the_plan():
    """k_rows_fold<true> (the split-K reduce that also folds the next GroupNorm) is among the launches above: with fold_fuse off the same
    plan has more stand-alone fold launches (host only)."""
    from sr3_hip import engine as E
    p = E.Plan('sr3', 6, 3, CFG['inner'], CFG['groups'], CFG['mults'], CFG['attn'], CFG['rb'], CFG['size'])
    folds = lambda: sum(1 for o in p.op_list(B) if o['kind'] == 40)
    fused = folds()
    p.set_option('fold_fuse', 0)
    assert folds() > fused


def test_three_replays_of_the_captured_step_are_bit_identical():
    """The captured reverse step, three replays from the same state and seed: every bit on against 0.  Every kernel of a replay reads
    tensors the launch in front of it wrote through, and the next replay reads this one's image."""
    netG = _netG()
    un = netG.denoise_fn
    d = G.dev()
    H, W = GEOMETRIES['native_32x32']
    shape = (B, 3, H, W)
    g = torch.Generator().manual_seed(9)
    x0 = torch.randn(shape, generator=g)
    cond = torch.rand(shape, generator=g) * 2 - 1
    un.plan.set_geometry(H, W)
    got = {}
    for mask in (0, 7):
        un.plan.set_option('store_wt', mask)
        st = netG._loop_state(shape, shape, d)
        un.ensure_derived()
        netG._capture(st)
        st['img'].copy_(x0); st['cond'].copy_(cond); st['step'].fill_(60)
        torch.manual_seed(31)
        imgs, zs = [], []
        for _ in range(3):
            st['graph'].replay()
            imgs.append(st['img'].clone()); zs.append(st['z'].clone())
        torch.cuda.synchronize()
        assert int(st['step'][1].item()) == 57
        got[mask] = (imgs, zs)
    for i in range(3):
        assert torch.equal(got[0][1][i], got[7][1][i]), 'the two series drew different noise at replay %d' % i
        assert torch.equal(got[0][0][i], got[7][0][i]), 'replay %d differs' % i
    assert bool(torch.isfinite(got[7][0][2]).all()) and not torch.equal(got[7][0][0], got[7][0][2])


@pytest.mark.parametrize('mask', [0, 7])
@pytest.mark.parametrize('name', NAMES)
def test_layer_taps_with_the_dummy_loads_on_one_line(name, mask):
    """test_gpu_unet.py's layer taps, same arrays and tolerance: the Winograd kernels' dummy residual loads on one line, with plain stores (0)
    and with every write-through store beside them (7)."""
    m, g, sd = build(name, keep_all=1, store_wt=mask)
    un = m.netG.denoise_fn
    d = G.dev()
    x = torch.from_numpy(g['unet/x']).to(d)
    t = torch.from_numpy(g['unet/time']).to(d)
    eps = un(x, t)
    torch.cuda.synchronize()
    ws = un._ws.buf
    off0 = (-ws.data_ptr()) % 256
    Bn = x.shape[0]
    for (tname, off, C, H, W) in un.plan.taps():
        raw = ws[off0 + off: off0 + off + Bn * H * W * C * 4].view(torch.float32).view(Bn, H, W, C)
        G.assert_close(raw.permute(0, 3, 1, 2).cpu(), torch.from_numpy(g['unet/tap/' + tname]), what='%s tap %s' % (name, tname))
    G.assert_close(eps.cpu(), torch.from_numpy(g['unet/eps']), what=name + ' eps')
