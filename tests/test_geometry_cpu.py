"""Plan geometry (sr3_plan_set_geometry): host-only inspection of the launch list at image sizes other than the config's
image_size, and the oracle pinned to the reference at rectangular shapes (tests/golden/sr3_rect.npz, tools/make_golden_rect.py).
CPU only: nothing here launches a kernel."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import DESCS, SCHEDS, load_golden
from oracle import sr3_oracle as O
from sr3_hip import engine as E
from sr3_hip import lib as L

FULL = ('sr3', 6, 3, 64, 32, [1, 2, 4, 8, 8], [16], 2, 128)      # the headline SR3 16 -> 128 network
GEOMETRIES = [(128, 192), (176, 128), (256, 256), (64, 64)]
B = 16


def ragged_rule(h, w):
    """The committed rule of wino_mode / wino_ragged_wins (what choose_conv asks first: csrc/plan_build.hip) for a 3x3 stride-1 conv
    on an h x w map of a plan that is NOT at its native geometry: which tile it must be reported on."""
    if w % 16 == 0 and h % 16 == 0:
        return (13,)                  # the tiles of today's rules
    if w % 16 == 0 and h % 8 == 0:
        return (13,)                  # whole multiple of the 8 x 16 tile: the plain two-workgroup kernel
    padded = -(-h // 8) * 8 * -(-w // 16) * 16
    if 4 * h * w >= padded:
        return (23,)                  # ragged: 0.24-0.57 of the fallback's time wherever the map fills >= 34 % of its tile grid
    return (1, 2, 3, 4, 5, 6, 9, 14, 15, 16, 17)      # 4 x 4 maps (12.5 %): measured 1.2x SLOWER than the fallback, which they keep


def _levels(h, w, n=5):
    return [(h >> i, w >> i) for i in range(n)]


def test_abi_has_geometry_entry_points():
    lib = L.load()
    assert 'sr3_plan_set_geometry' in L.SIGNATURES and 'sr3_plan_get_geometry' in L.SIGNATURES
    p = E.Plan(*FULL)
    h, w = C.c_int(), C.c_int()
    L.check(lib.sr3_plan_get_geometry(p.handle, C.byref(h), C.byref(w)))
    assert (h.value, w.value) == (128, 128) and p.geometry == (128, 128)


def test_native_plan_is_unchanged_by_the_setter():
    p = E.Plan(*FULL)
    ops, ws, fl = p.op_list(B), p.workspace_bytes(B), p.forward_flops(B)
    gen = p.generation
    for g in [(0, 0), (128, 128)]:
        p.set_geometry(*g)
        assert p.generation == gen
        assert p.op_list(B) == ops and p.workspace_bytes(B) == ws and p.forward_flops(B) == fl, g
    p.set_geometry(128, 192)
    assert p.generation != gen and p.geometry == (128, 192)
    assert p.op_list(B) != ops
    p.set_geometry(128, 128)
    assert p.generation == gen                # a geometry seen before gets its launch-list id back (cached graphs stay valid)
    assert p.op_list(B) == ops and p.workspace_bytes(B) == ws and p.forward_flops(B) == fl
    fresh = E.Plan(*FULL)
    assert fresh.op_list(B) == ops and fresh.workspace_bytes(B) == ws
    # no ragged tile at the native geometry, at any batch (the native launch list is today's)
    for b in (1, 2, 3, 4, 16):
        assert all(o['tile_cfg'] != 23 for o in fresh.op_list(b))


@pytest.mark.parametrize('hw', GEOMETRIES, ids=['%dx%d' % g for g in GEOMETRIES])
def test_launch_list_follows_the_geometry(hw):
    h, w = hw
    p = E.Plan(*FULL)
    sq = p.op_list(B)
    sq_flops = p.forward_flops(B)
    p.set_geometry(h, w)
    ops = p.op_list(B)
    assert p.workspace_bytes(B) > 0
    # structure: no op silently dropped.  Embedding, input conv, convs, attention, output conv appear in the same order with the
    # same channel counts as in the square plan (statistics / fold launches differ: which kernel fuses them depends on the split-K choice)
    sig = lambda lst: [(o['kind'], o['ksize'], o['stride'], o['upsample'], o['cin'], o['cout']) for o in lst if o['kind'] in (10, 20, 50, 60, 70)]
    assert sig(ops) == sig(sq)
    # every conv's output size is its level's size
    levels = _levels(h, w)
    sq_levels = _levels(128, 128)
    for o, s in zip([o for o in ops if o['kind'] in (20, 50)], [o for o in sq if o['kind'] in (20, 50)]):
        lvl = sq_levels.index((s['h_out'], s['w_out']))
        assert (o['h_out'], o['w_out']) == levels[lvl], (o, s)
    for o, s in zip([o for o in ops if o['kind'] == 60], [o for o in sq if o['kind'] == 60]):
        assert o['h_out'] * 128 * 128 == s['h_out'] * h * w          # tokens
    # flops: the contractions scale with H * W, except attention's, which scales with its square
    attn = lambda lst: sum(o['flops'] for o in lst if o['kind'] == 60)
    r = (h * w) / (128.0 * 128.0)
    got = p.forward_flops(B) - attn(ops)
    want = (sq_flops - attn(sq)) * r
    assert abs(got - want) <= 1e-3 * want, (got, want)              # (the embedding MLP does not scale: ~1e-5 of the total)
    assert abs(attn(ops) - attn(sq) * r * r) <= 1e-9 * attn(sq)
    # every 3x3 stride-1 conv is on a Winograd tile wherever the committed rule says so
    for o in ops:
        if o['kind'] == 50 and o['ksize'] == 3 and o['stride'] == 1:
            if (h, w) == (64, 64) and (o['h_out'], o['w_out']) == (8, 8) and not o['upsample']:
                assert o['tile_cfg'] == 12, o            # 8 x 8 maps, batch % 4 == 0: the four-image tile, as at the native size
            else:
                assert o['tile_cfg'] in ragged_rule(o['h_out'], o['w_out']), o
    # the A/B knob: without the ragged form those layers land on the general kernels, nothing else moves
    p.set_option('wino_ragged', 0)
    off = p.op_list(B)
    assert sig(off) == sig(ops) and all(o['tile_cfg'] != 23 for o in off)
    for a, b in zip([o for o in ops if o['kind'] == 50], [o for o in off if o['kind'] == 50]):
        assert a['tile_cfg'] == b['tile_cfg'] or a['tile_cfg'] == 23


def test_refusals_name_the_cause_and_leave_the_plan_usable():
    p = E.Plan(*FULL)
    ws = p.workspace_bytes(1)
    p.set_geometry(384, 384)                  # attention level 48 x 48 = 2304 tokens: no kernel holds that score strip
    with pytest.raises(L.Sr3Error, match=r'48 x 48 level has 2304 tokens'):
        p.workspace_bytes(1)
    assert p.num_ops(1) == -1
    with pytest.raises(L.Sr3Error, match='multiples of 16'):
        p.set_geometry(130, 128)
    assert p.lib.sr3_plan_set_geometry(p.handle, 130, 128) != 0 and b'multiples of 16' in p.lib.sr3_last_error()
    assert p.lib.sr3_plan_set_geometry(p.handle, -16, 128) != 0
    p.set_geometry(128, 128)
    assert p.workspace_bytes(1) == ws


def test_training_is_native_geometry_only():
    p = E.Plan(*FULL)
    native = int(p.lib.sr3_train_workspace_bytes(p.handle, 2, 3))
    assert native > 0
    p.set_geometry(128, 192)
    assert int(p.lib.sr3_train_workspace_bytes(p.handle, 2, 3)) == 0
    assert b'image_size x image_size only' in p.lib.sr3_last_error()
    p.set_geometry(0, 0)
    assert int(p.lib.sr3_train_workspace_bytes(p.handle, 2, 3)) == native


TOL = 2e-6     # same torch CPU ops in a different call order (tests/test_oracle_golden.py)


def _close(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    d = np.abs(a - b).max()
    assert d <= TOL * max(1.0, np.abs(b).max()), d


@pytest.mark.parametrize('hw', ['16x24', '24x16'])
def test_oracle_matches_the_reference_at_rectangular_shapes(hw):
    """Yardstick (passes without the feature): the oracle is shape-generic, the fixture is the reference's own output."""
    g, _ = load_golden('sr3_rect')
    _, sd = load_golden('sr3_tiny')
    d, tab = DESCS['sr3_tiny'], O.schedule_tables(SCHEDS['sr3_tiny'])
    k = hw + '/'
    with torch.no_grad():
        eps = O.unet_forward(sd, d, torch.from_numpy(g[k + 'unet/x']), torch.from_numpy(g[k + 'unet/time']))
        _close(eps.numpy(), g[k + 'unet/eps'])
        sr, zs = torch.from_numpy(g[k + 'loop/sr']), torch.from_numpy(g[k + 'loop/zs'])
        t = int(g[k + 'step/t'])
        r = O.p_sample(sd, d, tab, torch.from_numpy(g[k + 'step/x']), t, zs[t], condition_x=sr)
        _close(r.numpy(), g[k + 'step/out'])
        loop = O.p_sample_loop(sd, d, tab, sr, torch.from_numpy(g[k + 'loop/x_T']), zs, conditional=True, continous=True)
        _close(loop.numpy(), g[k + 'loop/ret_continous'])
    H, W = (int(v) for v in hw.split('x'))
    assert loop.shape == (2 * (1 + 8), 3, H, W)
