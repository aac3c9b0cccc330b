"""Multi-head SelfAttention (plan options attn_heads / attn_head_dim, sr3_attention_heads_f32, sr3_attention_bwd_heads_f32): the float64
restatement of the reference module against the oracle, the config keys, and the host-side refusals of the plan and the two entries.
CPU only: nothing here launches a kernel (the refusals return before any device call; the pointers handed in are never read)."""
import ctypes as C

import pytest
import torch

import mha_ref
from helpers import DESCS, load_golden, opt_for
from oracle import sr3_oracle as O
from sr3_hip import engine as E
from sr3_hip import lib as L

NET = ('sr3', 6, 3, 32, 32, [1, 2, 4], [8], 1, 16)      # attention at 8 x 8 with 64 channels, the middle block at 4 x 4 with 128
PTR = C.c_void_p(4096)                                   # a non-null, 16-byte aligned address no refusal path dereferences


def _seam_attention_input():
    _, sd = load_golden('sr3_seam')
    p = sorted(k for k in sd if k.endswith('.attn.qkv.weight'))[0][:-len('.qkv.weight')]
    c = sd[p + '.qkv.weight'].shape[1]
    x = torch.randn(2, c, 8, 8, generator=torch.Generator().manual_seed(4))
    return sd, p, x, DESCS['sr3_seam']['norm_groups']


def test_mha_ref_with_one_head_is_the_oracle_bit_for_bit():
    sd, p, x, groups = _seam_attention_input()
    assert torch.equal(mha_ref.self_attention(sd, p, x, groups, 1), O.self_attention(sd, p, x, groups))
    assert torch.equal(mha_ref.patched(n_head=1)(sd, p, x, groups), O.self_attention(sd, p, x, groups))


def test_mha_ref_with_two_heads_differs_and_core_agrees_with_the_module():
    sd, p, x, groups = _seam_attention_input()
    one, two = mha_ref.self_attention(sd, p, x, groups, 1), mha_ref.self_attention(sd, p, x, groups, 2)
    assert (one - two).abs().max().item() > 1e-3
    c = x.shape[1]
    assert torch.equal(mha_ref.patched(head_dim=c // 2)(sd, p, x, groups), two)
    # core() on the NHWC qkv tensor is the module's middle: rebuild the module's output from it
    import torch.nn.functional as F
    xd = x.double()
    sdd = {k: v.double() for k, v in sd.items() if k.startswith(p)}
    norm = F.group_norm(xd, groups, sdd[p + '.norm.weight'], sdd[p + '.norm.bias'], eps=1e-5)
    qkv = F.conv2d(norm, sdd[p + '.qkv.weight']).permute(0, 2, 3, 1).reshape(2, 64, 3 * c)
    for h in (1, 2, 4):
        o = mha_ref.core(qkv, c, h).reshape(2, 8, 8, c).permute(0, 3, 1, 2)
        got = F.conv2d(o, sdd[p + '.out.weight'], sdd[p + '.out.bias']) + xd
        ref = mha_ref.self_attention(sdd, p, xd, groups, h)
        assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_define_g_forwards_the_config_keys(name):
    import model.networks as networks

    def plan(**keys):
        opt = opt_for(name, phase='val', gpu=False)
        opt['model']['unet'].update(keys)
        un = networks.define_G(opt).denoise_fn
        return un, un.plan
    un, p = plan()
    assert 'attn_heads' not in p.options and 'attn_head_dim' not in p.options and 'n_head=1' in un.extra_repr()
    un, p = plan(n_head=2)
    assert p.options['attn_heads'] == 2 and 'attn_head_dim' not in p.options and 'n_head=2' in un.extra_repr()
    un, p = plan(head_dim=4)
    assert p.options['attn_head_dim'] == 4 and 'attn_heads' not in p.options and 'head_dim=4' in un.extra_repr()
    un, p = plan(n_head=None, head_dim=None)
    assert 'attn_heads' not in p.options and 'attn_head_dim' not in p.options
    with pytest.raises(ValueError, match='mutually exclusive'):
        plan(n_head=2, head_dim=4)
    with pytest.raises(L.Sr3Error, match=r'attn_heads 3: the attention of \S+ has 16 channels'):
        plan(n_head=3)


def test_engine_unet_keywords():
    from sr3_hip.nn import EngineUNet
    from model.ddpm_modules.unet import UNet as DdpmUNet
    kw = dict(in_channel=6, out_channel=3, inner_channel=32, norm_groups=32, channel_mults=[1, 2, 4], attn_res=[8], res_blocks=1, image_size=16)
    assert EngineUNet(**kw, head_dim=32).plan.options == {'attn_head_dim': 32}
    assert DdpmUNet(**kw, n_head=4).plan.options == {'attn_heads': 4}
    with pytest.raises(ValueError, match='mutually exclusive'):
        EngineUNet(**kw, n_head=2, head_dim=32)
    with pytest.raises(TypeError):
        EngineUNet(6, 3, 32, 32, [1, 2, 4], [8], 1, 0, True, 16, False, False, 2)        # keyword-only, like long_attention


def test_plan_options_refusals_and_round_trip():
    p = E.Plan(*NET)
    gen = p.generation
    assert p.set_option('attn_heads', 2) == 1 and p.generation != gen
    with pytest.raises(L.Sr3Error, match='mutually exclusive'):
        p.set_option('attn_head_dim', 32)
    assert p.set_option('attn_heads', 1) == 2
    assert p.set_option('attn_head_dim', 32) == 0
    with pytest.raises(L.Sr3Error, match='mutually exclusive'):
        p.set_option('attn_heads', 2)
    assert p.set_option('attn_head_dim', 0) == 32
    # a value some level cannot take: the message names the level and its channels; the plan keeps its value
    for key, value, text in (('attn_heads', 3, r'attn_heads 3: the attention of \S+ has 64 channels'),
                             ('attn_heads', 32, r'attn_heads 32: the attention of \S+ has 64 channels'),       # head width 2
                             ('attn_heads', 128, r'attn_heads 128: the attention of \S+ has 64 channels'),
                             ('attn_head_dim', 48, r'attn_head_dim 48: the attention of \S+ has 64 channels'),
                             ('attn_head_dim', 2, r'attn_head_dim 2: the attention of \S+ has 64 channels'),
                             ('attn_head_dim', 128, r'attn_head_dim 128: the attention of \S+ has 64 channels'),
                             ('attn_heads', 0, r'attn_heads 0'), ('attn_head_dim', -4, r'attn_head_dim -4')):
        with pytest.raises(L.Sr3Error, match=text):
            p.set_option(key, value)
    assert p.set_option('attn_heads', 4) == 1 and p.set_option('attn_heads', 1) == 4
    assert p.set_option('attn_head_dim', 64) == 0           # 64 -> 1 head, 128 -> 2 heads


@pytest.mark.parametrize('key,value', [('attn_heads', 2), ('attn_head_dim', 32)])
def test_the_launch_list_keeps_its_length_and_kinds(key, value):
    fresh, p = E.Plan(*NET), E.Plan(*NET)
    p.set_option(key, value)
    for b in (1, 2):
        assert p.num_ops(b) == fresh.num_ops(b) > 0
        assert p.op_list(b) == fresh.op_list(b)               # kinds, shapes, tiles and FLOPs: the head count changes none of them
        assert p.workspace_bytes(b) == fresh.workspace_bytes(b)
    assert int(p.lib.sr3_train_workspace_bytes(p.handle, 2, 3)) == int(fresh.lib.sr3_train_workspace_bytes(fresh.handle, 2, 3)) > 0


def test_the_library_exports_and_binds_both_entries():
    lib = L.load()
    assert L.SIGNATURES['sr3_attention_heads_f32'] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p])
    assert L.SIGNATURES['sr3_attention_bwd_heads_f32'] == (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])
    assert lib.sr3_attention_heads_f32.argtypes and lib.sr3_attention_bwd_heads_f32.argtypes


REFUSALS = [
    # B, N, C, heads, message
    (2, 64, 128, 0, r'heads 0 < 1'),
    (2, 64, 128, -2, r'heads -2 < 1'),
    (2, 64, 128, 3, r'128 channels do not divide into 3 heads'),
    (2, 64, 96, 16, r'head width 6 \(96 channels / 16 heads\) is not a multiple of 4'),
    (1024, 2304, 512, 8, r'exceeds 2\^31 elements'),
    (1024, 2304, 512, 1, r'exceeds 2\^31 elements'),
]


@pytest.mark.parametrize('B,N,Cc,heads,text', REFUSALS)
def test_the_entries_refuse_with_the_numbers(B, N, Cc, heads, text):
    lib = L.load()
    for mode in (0, 1, 2, 3):
        with pytest.raises(L.Sr3Error, match=text):
            L.check(lib.sr3_attention_heads_f32(PTR, B, N, Cc, heads, PTR, mode, None))
    with pytest.raises(L.Sr3Error, match=text):
        L.check(lib.sr3_attention_bwd_heads_f32(PTR, PTR, PTR, B, N, Cc, heads, PTR, PTR, 1 << 40, None))


def test_the_backward_entry_keeps_the_alignment_and_null_refusals():
    lib = L.load()
    with pytest.raises(L.Sr3Error, match='scratch is not 16-byte aligned'):
        L.check(lib.sr3_attention_bwd_heads_f32(PTR, PTR, PTR, 2, 64, 128, 2, PTR, C.c_void_p(4100), 1 << 30, None))
    with pytest.raises(L.Sr3Error, match='null argument'):
        L.check(lib.sr3_attention_bwd_heads_f32(PTR, PTR, PTR, 2, 64, 128, 2, PTR, None, 0, None))
    with pytest.raises(L.Sr3Error, match='null argument'):
        L.check(lib.sr3_attention_heads_f32(None, 2, 64, 128, 2, PTR, 0, None))
    assert int(lib.sr3_attention_bwd_scratch_bytes(2, 64, 128)) == 2 * 2 * 64 * 2 * 128 * 4      # (the slab total does not depend on heads)
