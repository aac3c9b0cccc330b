"""Upsample's conv on the two-workgroup Winograd kernel (csrc/conv3x3_wino2.hip): the UP instantiation -- tiles 13 / 23 with ups = 1,
nine of the sixteen Winograd positions -- against the sixteen-position loop on the same inputs (tiles 25 / 26): the seven positions it
skips multiply an operand that is exactly zero, so outputs and statistics must be the same BITS; and against float64 at the stated
tolerance.  Plan level: option wino_up = 1 / 0 give the same eps tensor."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import DESCS, load_golden, opt_for      # noqa: E402
import gpu_util as G                                 # noqa: E402

FULL = {13: 25, 23: 26}      # the sixteen-position forms of the two tiles


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


CASES = [
    # name, tile, B, C0, C1, Hs, Ws, Cout, act, bias, film, res, ksplit, stats
    ('borders_two_chunks', 13, 2, 32, 0, 8, 8, 64, 0, True, False, False, 1, False),
    ('interior_tile_column', 13, 2, 32, 0, 8, 24, 64, 0, True, False, False, 1, False),
    ('single_chunk', 13, 2, 16, 0, 8, 8, 64, 2, True, False, False, 1, False),
    ('partial_chunk', 13, 2, 24, 0, 8, 8, 64, 2, True, True, False, 1, False),
    ('concat', 13, 2, 24, 20, 8, 8, 64, 2, True, False, False, 1, True),
    ('split_k', 13, 2, 64, 0, 16, 16, 64, 1, True, True, True, 2, True),
    ('direct_stats', 13, 2, 48, 0, 8, 16, 72, 2, True, True, True, 1, True),
    ('two_cout_blocks', 13, 2, 32, 0, 8, 8, 128, 2, True, True, True, 1, False),
    ('persistent_second_tile', 13, 3, 16, 0, 64, 64, 128, 0, False, False, False, 1, False),     # 768 tiles on <= 512 workgroup slots
    ('ragged_10x14', 23, 3, 32, 0, 5, 7, 64, 2, True, True, True, 1, True),
    ('ragged_24x18', 23, 3, 24, 8, 12, 9, 72, 2, True, False, True, 1, True),
    ('ragged_24x18_split_k', 23, 3, 64, 0, 12, 9, 64, 0, True, False, False, 2, False),
]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_nine_positions_give_the_bits_of_sixteen(case):
    name, tile, B, C0, C1, Hs, Ws, Cout, act, bias, film, res, ksplit, stats = case
    Cin = C0 + C1
    src0 = _rand(B, C0, Hs, Ws, seed=1)
    src1 = _rand(B, C1, Hs, Ws, seed=2) if C1 else None
    w = _rand(Cout, Cin, 3, 3, seed=3, scale=1.0 / math.sqrt(9 * Cin))
    kw = dict(ups=1, stride=1, act=act)
    if bias:
        kw['bias'] = _rand(Cout, seed=4)
    if act:
        kw['ss'] = torch.stack([_rand(B, Cin, seed=5) * 0.3 + 1.0, _rand(B, Cin, seed=6) * 0.3], dim=2).contiguous()
    if film:
        kw['film'] = _rand(B, Cout, seed=7)
    if res:
        kw['res0'] = _rand(B, Cout, 2 * Hs, 2 * Ws, seed=8)
    nine, st9 = G.conv_call(src0, src1, w, tile_cfg=tile, ksplit=ksplit, want_stats=stats, **kw)
    full, st16 = G.conv_call(src0, src1, w, tile_cfg=FULL[tile], ksplit=ksplit, want_stats=stats, **kw)
    assert not torch.isnan(nine).any()
    assert torch.equal(nine, full), '%s: %d elements differ, max %.3e' % (name, (nine != full).sum().item(), (nine - full).abs().max().item())
    if stats:
        assert torch.equal(st9, st16)
        assert torch.allclose(st9[:, :, 0], nine.double().sum(dim=(2, 3)), rtol=1e-9, atol=1e-9)
        assert torch.allclose(st9[:, :, 1], (nine.double() ** 2).sum(dim=(2, 3)), rtol=1e-9, atol=1e-9)
    G.assert_close(nine, G.conv_ref(src0, src1, w, **kw), what=name)


def test_tile_numbers_without_upsampling_are_the_plain_tiles():
    """Tiles 25 / 26 only mean something with ups = 1: on a map that is not upsampled they run what 13 / 23 run."""
    src0 = _rand(2, 32, 16, 16, seed=11)
    w = _rand(64, 32, 3, 3, seed=12, scale=1.0 / math.sqrt(9 * 32))
    for tile in (13, 23):
        a, _ = G.conv_call(src0, None, w, tile_cfg=tile, ksplit=1)
        b, _ = G.conv_call(src0, None, w, tile_cfg=FULL[tile], ksplit=1)
        assert torch.equal(a, b)
        G.assert_close(a, G.conv_ref(src0, None, w), what='tile %d' % tile)


def test_plan_option_wino_up_is_bit_identical():
    """ddpm_tiny: the smallest helper network whose Upsample (8 x 8 -> 16 x 16) is on the two-workgroup Winograd kernel."""
    import model as Model
    name = 'ddpm_tiny'
    m = Model.create_model(opt_for(name, phase='val', gpu=True))
    g, sd = load_golden(name)
    m.netG.load_state_dict(sd, strict=True)
    un = m.netG.denoise_fn
    d = G.dev()
    x = torch.from_numpy(g['unet/x']).to(d)
    t = torch.from_numpy(g['unet/time']).to(d)
    ups = [o for o in un.plan.op_list(x.shape[0]) if o.get('upsample')]
    assert ups and all(o['tile_cfg'] == 13 for o in ups)
    e_up = un(x, t).clone()
    assert un.plan.set_option('wino_up', 0) == 1
    ups = [o for o in un.plan.op_list(x.shape[0]) if o.get('upsample')]
    assert ups and all(o['tile_cfg'] == 25 for o in ups)
    e_full = un(x, t).clone()
    assert un.plan.set_option('wino_up', 1) == 0
    assert torch.equal(e_up, e_full)
    G.assert_close(e_up.cpu(), torch.from_numpy(g['unet/eps']), what=name + ' eps')
    assert DESCS[name]['image_size'] == 16
