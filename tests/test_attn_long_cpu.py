"""Plan option attn_long (key-blocked attention beyond the LDS score strip): host-only inspection of the launch list, and the oracle
pinned to the reference at 1280 and 2304 attention tokens (tests/golden/sr3_long.npz, tools/make_golden_long.py).
CPU only: nothing here launches a kernel."""
import numpy as np
import pytest
import torch

from helpers import DESCS, SCHEDS, load_golden, opt_for
from oracle import sr3_oracle as O
from sr3_hip import engine as E
from sr3_hip import lib as L

FULL = ('sr3', 6, 3, 64, 32, [1, 2, 4, 8, 8], [16], 2, 128)      # the headline SR3 16 -> 128 network
B = 2
TOL = 2e-6     # same torch CPU ops in a different call order (tests/test_geometry_cpu.py)


def _close(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    d = np.abs(a - b).max()
    assert d <= TOL * max(1.0, np.abs(b).max()), d


@pytest.mark.parametrize('hw', ['80x64', '96x96'])
def test_oracle_matches_the_reference_at_long_token_counts(hw):
    """Yardstick (passes without the feature): the fixture is the reference's own output at 1280 / 2304 attention tokens."""
    g, _ = load_golden('sr3_long')
    _, sd = load_golden('sr3_tiny')
    d, tab = DESCS['sr3_tiny'], O.schedule_tables(SCHEDS['sr3_tiny'])
    k = hw + '/'
    x = torch.from_numpy(g[k + 'unet/x'])
    H, W = (int(v) for v in hw.split('x'))
    assert x.shape == (1, 6, H, W) and (H // 2) * (W // 2) in (1280, 2304)
    with torch.no_grad():
        eps = O.unet_forward(sd, d, x, torch.from_numpy(g[k + 'unet/time']))
        _close(eps.numpy(), g[k + 'unet/eps'])
        # the step's inputs are the halves of unet/x: condition = channels 0-2, x_t = channels 3-5
        r = O.p_sample(sd, d, tab, x[:, 3:].contiguous(), int(g[k + 'step/t']), torch.from_numpy(g[k + 'step/z']),
                       condition_x=x[:, :3].contiguous())
        _close(r.numpy(), g[k + 'step/out'])


def test_a_fresh_plan_still_refuses_384x384():
    """Yardstick: the option is off by default and the default plan's refusal is today's."""
    p = E.Plan(*FULL)
    p.set_geometry(384, 384)
    with pytest.raises(L.Sr3Error, match=r'48 x 48 level has 2304 tokens, more than the attention kernel holds in LDS'):
        p.workspace_bytes(1)
    assert p.num_ops(1) == -1


def _sig(lst):
    return [(o['kind'], o['ksize'], o['stride'], o['upsample'], o['cin'], o['cout']) for o in lst if o['kind'] in (10, 20, 50, 60, 70)]


@pytest.mark.parametrize('hw', [(256, 384), (384, 384), (400, 304), (512, 512)], ids=lambda g: '%dx%d' % g)
def test_long_geometries_build_with_the_option(hw):
    h, w = hw
    p = E.Plan(*FULL)
    sq, sq_flops = p.op_list(B), p.forward_flops(B)
    p.set_option('attn_long', 1)
    p.set_geometry(h, w)
    assert p.workspace_bytes(B) > 0 and p.num_ops(B) > 0
    ops = p.op_list(B)
    assert _sig(ops) == _sig(sq)
    attn_ops = [o for o in ops if o['kind'] == 60]
    assert attn_ops
    # attention sits at the 1/8-resolution level of this network (attn_res 16) and in the middle block (1/16): the former is beyond
    # the score strip at every one of these sizes and runs the key-blocked kernel, the latter (<= 1024 tokens) keeps the strip kernels
    n8, n16 = (h // 8) * (w // 8), (h // 16) * (w // 16)
    assert sorted(set(o['h_out'] for o in attn_ops)) == [n16, n8] and n8 > 1088 and n16 <= 1024
    for o in attn_ops:
        assert o['tile_cfg'] == (24 if o['h_out'] == n8 else 0), o
        assert o['flops'] == 4.0 * B * o['h_out'] * o['h_out'] * o['cin']
    assert sum(1 for o in attn_ops if o['tile_cfg'] == 24) == sum(1 for o in attn_ops if o['h_out'] == n8) > 0
    attn = lambda lst: sum(o['flops'] for o in lst if o['kind'] == 60)
    r = (h * w) / (128.0 * 128.0)
    got, want = p.forward_flops(B) - attn(ops), (sq_flops - attn(sq)) * r
    assert abs(got - want) <= 1e-3 * want, (got, want)


@pytest.mark.parametrize('hw', [(128, 128), (128, 192), (256, 256)], ids=lambda g: '%dx%d' % g)
def test_the_option_changes_nothing_where_the_strip_fits(hw):
    for b in (1, 16):
        fresh = E.Plan(*FULL)
        fresh.set_geometry(*hw)
        p = E.Plan(*FULL)
        p.set_option('attn_long', 1)
        p.set_geometry(*hw)
        ops = p.op_list(b)
        assert ops == fresh.op_list(b)
        assert p.workspace_bytes(b) == fresh.workspace_bytes(b) and p.forward_flops(b) == fresh.forward_flops(b)
        assert all(o['tile_cfg'] != 24 for o in ops)


def test_set_option_round_trip_and_refusal():
    p = E.Plan(*FULL)
    ws = p.workspace_bytes(1)
    gen = p.generation
    assert p.set_option('attn_long', 1) == 0
    assert p.generation != gen and p.options['attn_long'] == 1
    p.set_geometry(384, 384)
    assert p.workspace_bytes(1) > 0
    gen = p.generation
    assert p.set_option('attn_long', 0) == 1
    assert p.generation != gen
    with pytest.raises(L.Sr3Error, match=r'48 x 48 level has 2304 tokens') as ei:
        p.workspace_bytes(1)
    assert 'long_attention' in str(ei.value)              # the Python side names the config key
    assert p.num_ops(1) == -1
    assert b'long_attention' not in p.lib.sr3_last_error()      # ... the library's own message is unchanged
    p.set_geometry(128, 128)                  # the plan stays usable
    assert p.workspace_bytes(1) == ws
    assert p.set_option('attn_long', 1) == 0
    p.set_geometry(384, 384)
    assert p.num_ops(1) > 0


def test_training_workspace_is_unaffected():
    p = E.Plan(*FULL)
    native = int(p.lib.sr3_train_workspace_bytes(p.handle, 2, 3))
    assert native > 0
    p.set_option('attn_long', 1)
    assert int(p.lib.sr3_train_workspace_bytes(p.handle, 2, 3)) == native
    p.set_geometry(384, 384)
    assert int(p.lib.sr3_train_workspace_bytes(p.handle, 2, 3)) == 0
    assert b'image_size x image_size only' in p.lib.sr3_last_error()
    p.set_geometry(0, 0)
    assert int(p.lib.sr3_train_workspace_bytes(p.handle, 2, 3)) == native


@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_define_g_forwards_the_config_key(name):
    import model.networks as networks
    plans = {}
    for key in (None, False, True):
        opt = opt_for(name, phase='val', gpu=False)
        if key is not None:
            opt['model']['unet']['long_attention'] = key
        plans[key] = networks.define_G(opt).denoise_fn.plan
    assert 'attn_long' not in plans[None].options and 'attn_long' not in plans[False].options
    assert plans[True].options['attn_long'] == 1
    for key, p in plans.items():
        p.set_geometry(96, 96)                # sr3_tiny: attention at 48 x 48 = 2304 tokens
        if name == 'sr3_tiny' and not key:
            assert p.num_ops(1) == -1
        elif name == 'sr3_tiny':
            assert any(o['kind'] == 60 and o['tile_cfg'] == 24 and o['h_out'] == 2304 for o in p.op_list(1))
