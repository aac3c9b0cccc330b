"""Scale-shift time conditioning (config key model.unet.scale_shift_norm), everything that needs no GPU: tests/adagn_ref.py against an
independent block of torch.nn modules; the parameter table, state dicts and cross-loading; sr3_plan_create_ex's flags; the plan without
the flag against sr3_plan_create's; and the launch list's embed join."""
import copy
import ctypes as C

import pytest
import torch
from torch import nn

import adagn_ref
from helpers import DESCS, opt_for
from oracle import sr3_oracle as O
from sr3_hip import engine as E
from sr3_hip import lib as L

FILM = {'sr3': '.noise_func.noise_func.0.', 'ddpm': '.mlp.1.'}


def _plan(name, **kw):
    d = dict(DESCS[name])
    d.update(kw.pop('desc', {}))
    return E.Plan(d['variant'], d['in_channel'], d['out_channel'], d['inner_channel'], d['norm_groups'], d['channel_mults'], d['attn_res'],
                  d['res_blocks'], d['image_size'], **kw)


# ---- the reference block -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('variant', ['sr3', 'ddpm'])
@pytest.mark.parametrize('cin,cout', [(8, 8), (8, 16)], ids=['identity_res', 'res_conv'])
def test_adagn_ref_against_torch_modules(variant, cin, cout):
    """adagn_ref.resnet_block in float64 against the same block assembled from nn.GroupNorm / nn.Linear / nn.Conv2d, written out as ADM
    writes it (out_norm, th.chunk(emb_out, 2, dim=1), out_rest)."""
    torch.manual_seed(5)
    groups, inner, B = 4, 12, 3
    gn1, c1 = nn.GroupNorm(groups, cin), nn.Conv2d(cin, cout, 3, padding=1)
    gn2, c2 = nn.GroupNorm(groups, cout), nn.Conv2d(cout, cout, 3, padding=1)
    lin = nn.Linear(inner, 2 * cout)
    rc = nn.Conv2d(cin, cout, 1) if cin != cout else nn.Identity()
    nn.ModuleList([gn1, c1, gn2, c2, lin, rc]).double()
    for m in (gn1, gn2):                      # (the default affine, ones and zeros, would hide a swap of gamma and beta)
        nn.init.normal_(m.weight, 1.0, 0.3)
        nn.init.normal_(m.bias, 0.0, 0.3)
    x, temb = torch.randn(B, cin, 6, 5, dtype=torch.float64), torch.randn(B, inner, dtype=torch.float64)
    with torch.no_grad():
        h = c1(nn.functional.silu(gn1(x)))
        emb_out = lin(temb if variant == 'sr3' else nn.functional.silu(temb))[..., None, None]
        scale, shift = torch.chunk(emb_out, 2, dim=1)
        h = gn2(h) * (1 + scale) + shift
        want = c2(nn.functional.silu(h)) + rc(x)
        p = 'blk'
        sd = {p + '.block1.block.0.weight': gn1.weight, p + '.block1.block.0.bias': gn1.bias, p + '.block1.block.3.weight': c1.weight,
              p + '.block1.block.3.bias': c1.bias, p + '.block2.block.0.weight': gn2.weight, p + '.block2.block.0.bias': gn2.bias,
              p + '.block2.block.3.weight': c2.weight, p + '.block2.block.3.bias': c2.bias, p + FILM[variant] + 'weight': lin.weight,
              p + FILM[variant] + 'bias': lin.bias}
        if cin != cout:
            sd.update({p + '.res_conv.weight': rc.weight, p + '.res_conv.bias': rc.bias})
        got = adagn_ref.resnet_block(sd, p, x, temb if variant == 'ddpm' else temb.view(B, 1, inner), groups, variant)
    assert got.dtype == torch.float64 and (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()


# ---- the parameter table -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_parameter_table_with_the_flag(name):
    add, ssn = _plan(name), _plan(name, scale_shift_norm=True)
    assert [e['name'] for e in ssn.table] == [e['name'] for e in add.table]
    film = FILM[DESCS[name]['variant']]
    inner = DESCS[name]['inner_channel']
    spans, n_film = [], 0
    for a, s in zip(add.table, ssn.table):
        if film in s['name']:
            n_film += 1
            cout = a['shape'][0]
            assert s['shape'] == ((2 * cout, inner) if s['name'].endswith('weight') else (2 * cout,)), s
            assert s['numel'] == 2 * a['numel'] and s['pack'] == 0
        else:
            assert (s['shape'], s['numel'], s['pack']) == (a['shape'], a['numel'], a['pack']), s
        assert s['offset'] % 4 == 0, 'not 16-byte aligned: %s' % (s,)
        spans.append((s['offset'], s['offset'] + s['numel'], s['name']))
    assert n_film == 2 * sum(1 for e in add.table if e['name'].endswith('.res_block.block1.block.3.weight'))
    spans.sort()
    assert spans[0][0] >= 0 and spans[-1][1] <= ssn.param_floats
    for (lo, hi, n0), (lo1, _, n1) in zip(spans, spans[1:]):
        assert hi <= lo1, 'parameters overlap: %s and %s' % (n0, n1)
    assert ssn.param_floats > add.param_floats
    # one contiguous arena tensor per block: the view is the flat range in the checkpoint's shape
    arena = torch.arange(ssn.param_floats, dtype=torch.float32)
    for s in ssn.table:
        if film in s['name']:
            v = ssn.view(arena, s)
            assert v.is_contiguous() and tuple(v.shape) == s['shape'] and torch.equal(v.reshape(-1), arena[s['offset']:s['offset'] + s['numel']])


def _net(name, ssn, seed=3):
    import model.networks as networks
    opt = copy.deepcopy(opt_for(name, phase='val', gpu=False))
    if ssn is not None:
        opt['model']['unet']['scale_shift_norm'] = ssn
    netG = networks.define_G(opt)
    torch.manual_seed(seed)
    netG.denoise_fn.reset_parameters()
    return netG


@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_state_dict_round_trip_and_cross_loading(name):
    a, b = _net(name, True, seed=3), _net(name, True, seed=4)
    sd = a.state_dict()
    assert not torch.equal(a.denoise_fn.arena, b.denoise_fn.arena)
    b.load_state_dict(sd, strict=True)
    assert torch.equal(a.denoise_fn.arena, b.denoise_fn.arena)
    film = FILM[DESCS[name]['variant']]
    keys = [k for k in sd if film in k]
    assert keys and all(sd[k].shape[0] % 2 == 0 for k in keys)
    # the widened Linear is initialised by the additive one's rule: U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)) for weight and bias
    bound = 1.0 / DESCS[name]['inner_channel'] ** 0.5
    for k in keys:
        assert sd[k].abs().max().item() <= bound and sd[k].abs().max().item() > 0.5 * bound, k
    # either way round, a checkpoint of the other form fails on the shape, with the key named
    plain = _net(name, None)
    for src, dst in ((plain, a), (a, plain)):
        with pytest.raises(RuntimeError) as ei:
            dst.load_state_dict(src.state_dict(), strict=True)
        msg = str(ei.value)
        assert 'size mismatch' in msg and all(k in msg for k in keys), msg


def test_rng_draw_order_without_the_key_is_unchanged():
    """A network without the key draws what it always drew: false and absent give the same weights, and the flag's own network
    consumes the generator in the same order up to the first widened tensor."""
    a, b, s = _net('sr3_tiny', None), _net('sr3_tiny', False), _net('sr3_tiny', True)
    assert torch.equal(a.denoise_fn.arena, b.denoise_fn.arena)
    ta, ts = a.denoise_fn.plan.table, s.denoise_fn.plan.table
    first = next(i for i, e in enumerate(ts) if FILM['sr3'] in e['name'])
    for ea, es in zip(ta[:first], ts[:first]):
        assert torch.equal(a.denoise_fn.plan.view(a.denoise_fn.arena.detach(), ea), s.denoise_fn.plan.view(s.denoise_fn.arena.detach(), es)), ea['name']


def test_config_key_and_repr():
    assert _net('sr3_tiny', True).denoise_fn.scale_shift_norm is True and _net('ddpm_tiny', None).denoise_fn.scale_shift_norm is False
    assert 'scale_shift_norm=True' in repr(_net('ddpm_tiny', True).denoise_fn) and 'scale_shift_norm=False' in repr(_net('sr3_tiny', None).denoise_fn)
    for bad in (1, 'true', 0, [True]):
        with pytest.raises(ValueError, match='scale_shift_norm'):
            _net('sr3_tiny', bad)
    import model.networks as networks
    opt = copy.deepcopy(opt_for('sr3_tiny', phase='val', gpu=False))
    opt['model']['unet']['use_affine_level'] = True
    with pytest.raises(NotImplementedError, match='scale_shift_norm'):
        networks.define_G(opt)
    from model.sr3_modules.unet import UNet
    with pytest.raises(NotImplementedError, match='scale_shift_norm'):
        UNet(6, 3, 8, 4, (1, 2), (8,), 1, image_size=16, use_affine_level=True)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------

def test_plan_create_ex_flags():
    lib = L.load()
    desc = E.make_desc(**{k: DESCS['sr3_tiny'][k] for k in ('variant', 'in_channel', 'out_channel', 'inner_channel', 'norm_groups', 'channel_mults',
                                                           'attn_res', 'res_blocks', 'image_size')})
    for flags, bits in ((2, '0x2'), (0x81, '0x80'), (0xfffffffe, '0xfffffffe')):
        h = C.c_void_p(1)
        assert lib.sr3_plan_create_ex(C.byref(desc), flags, C.byref(h)) == -1          # SR3_E_BADARG
        msg = (lib.sr3_last_error() or b'').decode()
        assert 'unknown flag' in msg and bits in msg, msg
        assert not h.value
    for flags in (0, 1):
        h = C.c_void_p()
        assert lib.sr3_plan_create_ex(C.byref(desc), flags, C.byref(h)) == 0 and h.value
        lib.sr3_plan_destroy(h)
    assert lib.sr3_version() == 1


class _Ex0(E.Plan):
    """E.Plan whose handle comes from sr3_plan_create_ex(desc, 0, ...)"""
    def __init__(self, *a):
        super().__init__(*a)
        self.lib.sr3_plan_destroy(self.handle)
        h = C.c_void_p()
        L.check(self.lib.sr3_plan_create_ex(C.byref(self.desc), 0, C.byref(h)))
        self.handle = h


@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny', 'sr3_seam'])
def test_without_the_flag_the_plan_is_sr3_plan_creates(name):
    d = DESCS[name]
    args = (d['variant'], d['in_channel'], d['out_channel'], d['inner_channel'], d['norm_groups'], d['channel_mults'], d['attn_res'],
            d['res_blocks'], d['image_size'])
    a, b, c = E.Plan(*args), E.Plan(*args, scale_shift_norm=False), _Ex0(*args)
    for p in (b, c):
        pi = L.ParamInfo()
        table = []
        for i in range(p.lib.sr3_plan_num_params(p.handle)):
            L.check(p.lib.sr3_plan_param_info(p.handle, i, C.byref(pi)))
            table.append(dict(name=pi.name.decode(), shape=tuple(pi.shape[:pi.ndim]), pack=int(pi.pack), offset=int(pi.offset), numel=int(pi.numel)))
        assert table == a.table
        assert int(p.lib.sr3_plan_param_floats(p.handle)) == a.param_floats
        for B in (1, 3):
            assert p.workspace_bytes(B) == a.workspace_bytes(B)
            assert p.op_list(B) == a.op_list(B) and p.fold_list(B) == a.fold_list(B)
            assert all(row == -1 for _, row in p.fold_list(B))
            assert int(p.lib.sr3_train_workspace_bytes(p.handle, B, 0)) == int(a.lib.sr3_train_workspace_bytes(a.handle, B, 0)) > 0


# ---- the launch list ---------------------------------------------------------------------------------------------------------------------

WIDE = dict(inner_channel=32, norm_groups=32, channel_mults=[1, 2, 4], attn_res=[8], res_blocks=1)


@pytest.mark.parametrize('name,desc', [('sr3_tiny', {}), ('ddpm_tiny', {}), ('sr3_tiny', WIDE)], ids=['sr3_tiny', 'ddpm_tiny', 'sr3_wide'])
@pytest.mark.parametrize('fold_fuse', [1, 0])
def test_the_embed_join_precedes_every_modulated_fold(name, desc, fold_fuse):
    """One modulated fold per res block, in block order, on the block's rows (2 x the cumulative Cout); no conv adds a FiLM row, so
    under fork_side the embed op -- on the side stream -- is joined by the first op that reads a modulation row, and that op comes
    before (or is) every modulated fold.  The additive plan of the same network joins at a conv, as it always did."""
    B = 2
    p = _plan(name, desc=desc, scale_shift_norm=True)
    p.set_option('fold_fuse', fold_fuse)
    ops, folds = p.op_list(B), p.fold_list(B)
    mod = [(i, kind, row) for i, (kind, row) in enumerate(folds) if row >= 0]
    couts = [e['shape'][0] for e in p.table if e['name'].endswith('.res_block.block1.block.3.weight')]
    rows, acc = [], 0
    for c in couts:
        rows.append(2 * acc)
        acc += c
    assert [row for _, _, row in mod] == rows
    assert all(kind in ((1,) if not fold_fuse else (1, 2, 3)) for _, kind, _ in mod)
    assert all('wait_id' not in o and 'side_id' not in o for o in ops)          # one stream: list order is execution order
    p.set_option('fork_side', 1)
    ops, folds2 = p.op_list(B), p.fold_list(B)
    mod = [i for i, (_, row) in enumerate(folds2) if row >= 0]
    assert ops[0]['kind'] == 10 and ops[0].get('side_id', -1) >= 0, 'the embed op is not on the side stream'
    join = [i for i, o in enumerate(ops) if o.get('wait_id', -1) == ops[0]['side_id']]
    assert len(join) == 1 and 0 < join[0] <= mod[0], (join, mod)
    assert join[0] == mod[0], 'the join is not the first op that reads a modulation row'
    # the additive network: joined by the first res block's conv1
    q = _plan(name, desc=desc)
    q.set_option('fold_fuse', fold_fuse)
    q.set_option('fork_side', 1)
    qops = q.op_list(B)
    qjoin = [i for i, o in enumerate(qops) if o.get('wait_id', -1) == qops[0].get('side_id', -2)]
    assert len(qjoin) == 1 and qops[qjoin[0]]['kind'] == 50 and all(row == -1 for _, row in q.fold_list(B))
