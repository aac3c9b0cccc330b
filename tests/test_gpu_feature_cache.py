"""Feature-cached forward (plan option feat_cache; sr3_unet_forward_cached) on the GPU, against the engine's own uncached forward and
the CPU restatement in tests/feature_cache_ref.py.  16 x 16, batch 2, the tiny golden weights; one case at a real width."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd')
for p in (ROOT, PKG, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import feature_cache_ref as R                                   # noqa: E402
import gpu_util as G                                            # noqa: E402
from helpers import DESCS, load_golden, opt_for                 # noqa: E402

pytestmark = pytest.mark.gpu

TOL, WIDE = R.TOL, R.WIDE
CASES = [('sr3_tiny', 1), ('sr3_tiny', 2), ('ddpm_tiny', 1), ('ddpm_tiny', 2), ('ddpm_tiny', 3)]
_NETS, _REFS = {}, {}


def inputs(name, B=2):
    return R.inputs(DESCS[name] if name in DESCS else WIDE, B)


def net(name):
    """The case's network on the GPU with the golden weights (built once), and its state dict for the oracle."""
    if name not in _NETS:
        import model as Model
        m = Model.create_model(opt_for(name, phase='val', gpu=True))
        _, sd = load_golden(name)
        m.netG.load_state_dict(sd, strict=True)
        _NETS[name] = (m.netG.denoise_fn, sd, DESCS[name])
    return _NETS[name]


def reference(name, depth):
    """(full eps at A, cached eps at B, full eps at B) on the oracle, computed once per case."""
    if (name, depth) not in _REFS:
        un, sd, desc = net(name) if name != 'wide' else wide()
        _REFS[(name, depth)] = R.cached_forward(sd, desc, depth, *inputs(name))
    return _REFS[(name, depth)]


def err(got, ref):
    return (got.double() - ref.double()).abs().max().item(), TOL * max(1.0, ref.abs().max().item())


@pytest.fixture
def restore_option():
    yield
    for un, _, _ in _NETS.values():
        if un.plan.options.get('feat_cache'):
            un.plan.set_option('feat_cache', 0)


@pytest.mark.parametrize('name,depth', CASES)
def test_refresh_is_the_uncached_forward_bit_for_bit(name, depth, restore_option):
    un, _, _ = net(name)
    d = G.dev()
    xa, ta, _, _ = inputs(name)
    assert not un.plan.options.get('feat_cache')
    base = un(xa.to(d), ta.to(d), full=True).clone()
    un.plan.set_option('feat_cache', depth)
    cache = un.plan.new_feature_cache(2, d)
    got = un(xa.to(d), ta.to(d), full=True, feat_cache=cache, refresh=True)
    assert torch.equal(got, base)
    # ... and through the plan's own cache, which is what a plain forward of such a plan uses
    assert torch.equal(un(xa.to(d), ta.to(d)), base)


@pytest.mark.parametrize('name,depth', CASES)
def test_cached_forward_at_the_refresh_point_matches_the_full_one(name, depth, restore_option):
    un, _, _ = net(name)
    d = G.dev()
    xa, ta, _, _ = inputs(name)
    un.plan.set_option('feat_cache', depth)
    cache = un.plan.new_feature_cache(2, d)
    full = un(xa.to(d), ta.to(d), full=True, feat_cache=cache, refresh=True).clone()
    got = un(xa.to(d), ta.to(d), full=True, feat_cache=cache, refresh=False)
    e, bound = err(got, full)
    print('%s depth %d: cached vs full at the refresh point, max abs %.3e (bound %.3e), equal bits: %s' % (name, depth, e, bound, torch.equal(got, full)))
    assert e <= bound


@pytest.mark.parametrize('name,depth', CASES)
def test_stale_cache_semantics_against_the_oracle(name, depth, restore_option):
    """refresh at (x_A, level_A), cached at an independent (x_B, level_B): the oracle's shallow forward on A's branch tensor -- and not
    the full forward at B, from which the case must stand more than ten tolerances away (on the oracle as on the device)."""
    un, _, _ = net(name)
    d = G.dev()
    xa, ta, xb, tb = inputs(name)
    ref_a, ref_cached, ref_b = reference(name, depth)
    gap = (ref_cached - ref_b).abs().max().item()
    assert gap > 10 * TOL * max(1.0, ref_b.abs().max().item()), 'the case cannot tell a cached step from a full one (gap %.3e)' % gap
    un.plan.set_option('feat_cache', depth)
    cache = un.plan.new_feature_cache(2, d)
    got_a = un(xa.to(d), ta.to(d), full=True, feat_cache=cache, refresh=True).cpu()
    got = un(xb.to(d), tb.to(d), full=True, feat_cache=cache, refresh=False).cpu()
    ea, bound_a = err(got_a, ref_a)
    e, bound = err(got, ref_cached)
    print('%s depth %d: refresh err %.3e, cached err %.3e (bound %.3e), gap to the full forward at B %.3e' % (name, depth, ea, e, bound, gap))
    assert ea <= bound_a and e <= bound
    assert (got - ref_b).abs().max().item() > 10 * TOL * max(1.0, ref_b.abs().max().item())


# ---- one case at a real width: the shallow list on the production kernels ------------------------------------------------------


def wide():
    if 'wide' not in _NETS:
        import model.networks as networks
        opt = opt_for('sr3_tiny', phase='val', gpu=True)
        opt['model']['unet'].update(inner_channel=64, norm_groups=32, channel_multiplier=[1, 2], attn_res=[32], res_blocks=2)
        opt['model']['diffusion']['image_size'] = 32
        torch.manual_seed(11)
        netG = networks.define_G(opt)
        sd = {k: v.clone() for k, v in netG.state_dict().items()}
        _NETS['wide'] = (netG.to(G.dev()).denoise_fn, sd, dict(WIDE))
    return _NETS['wide']


@pytest.mark.parametrize('depth', [1, 3])
def test_real_width_shallow_list_against_the_oracle(depth, restore_option):
    un, sd, desc = wide()
    d = G.dev()
    xa, ta, xb, tb = inputs('wide')
    ref_a, ref_cached, ref_b = reference('wide', depth)
    un.plan.set_option('feat_cache', depth)
    shallow = un.plan.shallow_op_list(2)
    tiles = sorted(set(o['tile_cfg'] for o in shallow if o['kind'] == 50))
    # the shallow list meets the production kernels: every conv on the two-workgroup Winograd tile (ABI 13) or the plain GEMM (22), and
    # the top level's attention, one per res block (d - 1 down blocks, d up blocks) -- depth 1 and 2 take their branch tensor from an
    # attention's out projection
    assert tiles == [13, 22], tiles
    assert sum(1 for o in shallow if o['kind'] == 60) == 2 * depth - 1 and all(o['h_out'] == 32 * 32 for o in shallow if o['kind'] == 60)
    cache = un.plan.new_feature_cache(2, d)
    got_a = un(xa.to(d), ta.to(d), full=True, feat_cache=cache, refresh=True).cpu()
    got = un(xb.to(d), tb.to(d), full=True, feat_cache=cache, refresh=False).cpu()
    ea, bound_a = err(got_a, ref_a)
    e, bound = err(got, ref_cached)
    gap = (ref_cached - ref_b).abs().max().item()
    print('wide depth %d: conv tiles %s, refresh err %.3e, cached err %.3e (bound %.3e), gap %.3e' % (depth, tiles, ea, e, bound, gap))
    assert ea <= bound_a and e <= bound


# ---- the cache is the caller's and no part of the workspace --------------------------------------------------------------------

@pytest.mark.parametrize('name,depth', [('sr3_tiny', 2), ('ddpm_tiny', 1)])
def test_cache_poisoning(name, depth, restore_option):
    from sr3_hip import engine as E
    un, _, _ = net(name)
    d = G.dev()
    xa, ta, xb, tb = (t.to(d) for t in inputs(name))
    un.plan.set_option('feat_cache', depth)
    cache, ws = un.plan.new_feature_cache(2, d), E.Workspace()
    un(xa, ta, full=True, feat_cache=cache, refresh=True, ws=ws)
    base = un(xb, tb, full=True, feat_cache=cache, refresh=False, ws=ws).clone()
    # a NaN-filled cache: the refresh overwrites all of it that a cached forward reads
    cache.view(torch.float32).fill_(float('nan'))
    un(xa, ta, full=True, feat_cache=cache, refresh=True, ws=ws)
    got = un(xb, tb, full=True, feat_cache=cache, refresh=False, ws=ws).clone()
    assert torch.isfinite(got).all() and torch.equal(got, base)
    # a NaN-filled workspace between the refresh and the cached forward: nothing of the cache lives there
    un(xa, ta, full=True, feat_cache=cache, refresh=True, ws=ws)
    ws.buf.fill_(0xFF)                 # (every float a NaN)
    got = un(xb, tb, full=True, feat_cache=cache, refresh=False, ws=ws)
    assert torch.isfinite(got).all() and torch.equal(got, base)


def test_refusals_launch_nothing(restore_option):
    from sr3_hip import lib as L
    un, _, _ = net('sr3_tiny')
    d = G.dev()
    xa, ta, _, _ = (t.to(d) for t in inputs('sr3_tiny'))
    with pytest.raises(L.Sr3Error, match='needs plan option feat_cache'):
        un(xa, ta, full=True, refresh=False)
    un.plan.set_option('feat_cache', 1)
    cache = un.plan.new_feature_cache(2, d)
    with pytest.raises(L.Sr3Error, match='never filled'):
        un(xa, ta, full=True, feat_cache=cache, refresh=False)
    with pytest.raises(L.Sr3Error, match='feature cache too small'):
        un(xa, ta, full=True, feat_cache=cache[:256], refresh=True)
    un(xa, ta, full=True, feat_cache=cache, refresh=True)
    with pytest.raises(L.Sr3Error, match='filled at batch 2'):
        un(xa[:1], ta[:1], full=True, feat_cache=cache, refresh=False)
    other = un.plan.new_feature_cache(2, d)
    with pytest.raises(L.Sr3Error, match='in another buffer'):
        un(xa, ta, full=True, feat_cache=other, refresh=False)
    # a geometry other than the fill's, in a cache large enough for it
    need = un.plan.feature_cache_bytes(2)
    big = torch.empty(4 * need + 512, dtype=torch.uint8, device=d)
    big = big[(-big.data_ptr()) % 256:]
    un(xa, ta, full=True, feat_cache=big[:4 * need], refresh=True)
    x32 = torch.randn(2, 6, 32, 32, device=d)
    with pytest.raises(L.Sr3Error, match='filled at batch 2, geometry 16 x 16: a cached forward at batch 2, geometry 32 x 32'):
        un(x32, ta, full=True, feat_cache=big[:4 * need], refresh=False)
    un.plan.set_geometry(16, 16)
    # through the ABI itself: a null cache and a misaligned one, on a refresh and on a cached forward
    import ctypes as C
    from sr3_hip import engine as E
    ws, out = E.Workspace(), torch.empty(2, 3, 16, 16, device=d)
    wsbuf, wsn = ws.get(un.plan, 2, d)
    lvl = ta.reshape(-1).contiguous()

    def raw(cache_ptr, nbytes, refresh):
        rc = un.plan.lib.sr3_unet_forward_cached(un.plan.handle, L.ptr(xa), None, 0, L.ptr(lvl), None, L.ptr(un.freq), None, None,
                                                 L.ptr(un.weights()), L.ptr(wsbuf), wsn, L.ptr(out), 2, G.stream(), None, cache_ptr, nbytes,
                                                 refresh)
        return rc, un.plan.lib.sr3_last_error().decode()
    for refresh in (1, 0):
        rc, msg = raw(None, need, refresh)
        assert rc == -1 and msg == 'null feature cache', (rc, msg)
        rc, msg = raw(C.c_void_p(big.data_ptr() + 16), need, refresh)
        assert rc == -3 and msg.startswith('misaligned feature cache'), (rc, msg)
    rc, msg = raw(C.c_void_p(big.data_ptr()), need, 1)
    assert rc == 0, msg
