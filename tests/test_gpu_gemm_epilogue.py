"""Plan option gemm_epi / tiles 27, 28, 29 of the per-op ABI: the three epilogue forms of the plain GEMM kernel (csrc/gemm1x1.hip).
27 = every lane stores its accumulator registers as 4-byte elements; 28 = each wave transposes its 32 x 32 accumulator blocks through LDS
and loads bias / FiLM row / residual and stores 16 bytes wide; 29 = 28 with the stores written through L2.  The additions of an element
keep their order, so 28 and 29 must give the BITS of 27, and 27 must meet the stated tolerance against float64 -- per op on the smallest
shape that reaches each of the nine instantiations (the tile that ran is asserted through sr3_gemm_tile), split-K slabs included, and
over whole paths: a forward, the captured reverse step replayed, one training step."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util as G                                # noqa: E402
from guarded import F as FILL_F, Guarded            # noqa: E402
from sr3_hip import lib as L                        # noqa: E402
from test_gpu_fullsize import make_opt              # noqa: E402

FORMS = (27, 28, 29)

# name, (rows, cols) of the tile, B, C0, C1, Hs, Ws, Cout, ksize, stride, act, bias, film, residual split (RC0, RC1) or None
CASES = [
    # 1. 32-row, 128-column tile
    ('r32_bias', (32, 128), 1, 32, 0, 4, 8, 128, 1, 1, 0, True, False, None),
    ('r32_act_all', (32, 128), 2, 64, 0, 4, 8, 256, 1, 1, 1, True, True, (256, 0)),
    # 2. 64-row, 128-column tile: M > 1024 and Cin > 512, two sources, two-source residual
    ('r64_two_src', (64, 128), 2, 512, 32, 32, 32, 128, 1, 1, 0, True, True, (64, 64)),
    ('r64_two_src_act', (64, 128), 2, 512, 32, 32, 32, 128, 1, 1, 1, True, True, (64, 64)),
    # 3. 64 x 64 tile, waves 2 x 2
    ('wm2_64', (64, 64), 1, 32, 0, 8, 8, 64, 1, 1, 0, False, False, None),
    ('wm2_192', (64, 64), 1, 32, 0, 8, 8, 192, 1, 1, 0, False, False, None),
    ('wm2_64_act_all', (64, 64), 1, 32, 0, 8, 8, 64, 1, 1, 1, True, True, (64, 0)),
    ('wm2_192_act_all', (64, 64), 1, 32, 0, 8, 8, 192, 1, 1, 1, True, True, (64, 128)),
    # 4. stride-2 forms
    ('s2_r32', (32, 128), 2, 32, 0, 8, 16, 128, 3, 2, 0, True, True, (128, 0)),
    ('s2_wm2', (64, 64), 2, 32, 0, 8, 16, 64, 3, 2, 0, True, True, (64, 0)),
    ('s2_r64', (64, 128), 6, 32, 0, 64, 64, 512, 3, 2, 0, True, False, None),
]
# one case per instantiation (MI 1 / 2, ACT, S2, WM 2) runs inside a guarded scratch of exactly the queried size as well
GUARDED = {'r32_bias', 'r32_act_all', 'r64_two_src', 'r64_two_src_act', 'wm2_64', 'wm2_64_act_all', 's2_r32', 's2_wm2', 's2_r64'}
# 5. split-K: cases 1 and 4 on a three-k-step problem (Cin 96; the stride-2 form walks 27 k-steps), ksplit 2 and 3: an uneven split;
# the 64-row forms (MI = 2: two accumulator blocks per wave go through the transpose into a slab) as the stride-2 shape of case 4 and
# the 1x1 shape of case 2 (17 k-steps)
SPLIT_CASES = [
    ('r32_bias_k96', (32, 128), 1, 96, 0, 4, 8, 128, 1, 1, 0, True, False, None),
    ('r32_act_all_k96', (32, 128), 2, 96, 0, 4, 8, 256, 1, 1, 1, True, True, (256, 0)),
    ('s2_r32_k96', (32, 128), 2, 96, 0, 8, 16, 128, 3, 2, 0, True, True, (128, 0)),
    ('s2_wm2_k96', (64, 64), 2, 96, 0, 8, 16, 64, 3, 2, 0, True, True, (64, 0)),
    ('s2_r64_k96', (64, 128), 6, 96, 0, 64, 64, 512, 3, 2, 0, True, False, None),
    ('r64_two_src_k544', (64, 128), 2, 512, 32, 32, 32, 128, 1, 1, 0, True, True, (64, 64)),
    ('r64_two_src_act_k544', (64, 128), 2, 512, 32, 32, 32, 128, 1, 1, 1, True, True, (64, 64)),
]
_split_refs = {}      # case name -> (float64 reference, reference of the bare conv): computed once, shared by both ksplit values


def _make(case, seed=3):
    name, tile, B, C0, C1, Hs, Ws, Cout, k, stride, act, bias, film, res = case
    g = torch.Generator().manual_seed(seed)
    Cin = C0 + C1
    Ho, Wo = Hs // stride, Ws // stride
    src0 = torch.randn(B, C0, Hs, Ws, generator=g)
    src1 = torch.randn(B, C1, Hs, Ws, generator=g) if C1 else None
    w = torch.randn(Cout, Cin, k, k, generator=g) / (k * k * Cin) ** 0.5
    kw = dict(stride=stride)
    if act:
        kw.update(act=act, ss=torch.stack([torch.rand(B, Cin, generator=g) + 0.5, torch.randn(B, Cin, generator=g) * 0.3], dim=2).contiguous())
    if bias:
        kw['bias'] = torch.randn(Cout, generator=g)
    if film:
        kw['film'] = torch.randn(B, Cout, generator=g)
    if res:
        kw['res0'] = torch.randn(B, res[0], Ho, Wo, generator=g)
        if res[1]:
            kw['res1'] = torch.randn(B, res[1], Ho, Wo, generator=g)
    # the tile this shape runs on, from the library: the case reaches the instantiation its name says
    rows, cols = C.c_int(0), C.c_int(0)
    assert L.load().sr3_gemm_tile(B, Ho, Wo, Cin, Cout, k, C.byref(rows), C.byref(cols)) == 1, name
    assert (rows.value, cols.value) == tile, '%s runs on a %d x %d tile' % (name, rows.value, cols.value)
    return src0, src1, w, kw


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_wide_epilogues_give_the_bits_of_the_four_byte_one(case):
    src0, src1, w, kw = _make(case)
    ref = G.conv_ref(src0, src1, w, **kw)
    outs = {t: G.conv_call(src0, src1, w, tile_cfg=t, ksplit=1, **kw)[0] for t in FORMS}
    print('%s: max abs err of tile 27 %.3e' % (case[0], (outs[27].double() - ref).abs().max().item()))
    G.assert_close(outs[27], ref, what=case[0] + ' tile 27')
    for t in (28, 29):
        assert torch.equal(outs[t], outs[27]), '%s: tile %d differs from 27 in %d elements' % (case[0], t, int((outs[t] != outs[27]).sum()))
    # tile 22 is one of the three forms
    assert torch.equal(G.conv_call(src0, src1, w, tile_cfg=22, ksplit=1, **kw)[0], outs[27])
    if case[0] in GUARDED:
        for t in FORMS:
            got, _ = G.conv_call(src0, src1, w, tile_cfg=t, ksplit=1, guard=FILL_F, **kw)
            assert torch.equal(got, outs[27]), '%s: tile %d in a guarded scratch' % (case[0], t)


def _call_with_slabs(src0, src1, w, tile_cfg, ksplit, bias=None, ss=None, act=0, film=None, res0=None, res1=None, stride=1):
    """gpu_util.conv_call with the scratch kept: returns (out NCHW cpu, slabs [ksplit][B, Ho, Wo, Cout] cpu); the scratch is exactly the
    queried size inside a guarded buffer, whose bands must come back intact, and the output sits in a guarded tensor of its own."""
    lib = L.load()
    d = G.dev()
    B, C0, Hs, Ws = src0.shape
    C1 = 0 if src1 is None else src1.shape[1]
    Cout, Cin, k, _ = w.shape
    Ho, Wo = Hs // stride, Ws // stride
    g = lambda t: None if t is None else t.to(d)
    s0, s1 = g(G.nhwc(src0)), (None if src1 is None else g(G.nhwc(src1)))
    wd, bd, ssd, fd = g(G.ohwi(w)), g(bias), g(ss), g(film)
    r0 = None if res0 is None else g(G.nhwc(res0))
    r1 = None if res1 is None else g(G.nhwc(res1))
    gout = Guarded(B * Ho * Wo * Cout * 4, 0xFF, d, 4096 * 4)
    out = gout.view(torch.float32, (B, Ho, Wo, Cout))
    nb = int(lib.sr3_conv_scratch_bytes(B, Ho, Wo, Cin, Cout, k, tile_cfg, ksplit))
    gs = Guarded(nb, 0xFF, d)
    L.check(lib.sr3_conv_f32(L.ptr(s0), C0, L.ptr(s1), C1, B, Hs, Ws, 0, stride, k, Cout, L.ptr(wd), L.ptr(bd), L.ptr(ssd), act, L.ptr(fd),
                             0 if film is None else film.shape[1], L.ptr(r0), 0 if res0 is None else res0.shape[1], L.ptr(r1),
                             0 if res1 is None else res1.shape[1], L.ptr(out), None, tile_cfg, ksplit, gs.ptr, nb, G.stream()))
    torch.cuda.synchronize()
    assert gs.intact() and gout.intact(), 'tile %d ksplit %d wrote outside its scratch or its output' % (tile_cfg, ksplit)
    n = B * Ho * Wo * Cout
    slabs = gs.view()[:ksplit * n * 4].view(torch.float32).view(ksplit, B, Ho, Wo, Cout).cpu()
    return G.nchw(out.clone()).cpu(), slabs


@pytest.mark.parametrize('ksplit', [2, 3])
@pytest.mark.parametrize('case', SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_split_k_slabs_and_reduced_output_have_the_same_bits(case, ksplit):
    src0, src1, w, kw = _make(case)
    bare = {k: v for k, v in kw.items() if k in ('stride', 'act', 'ss')}
    if case[0] not in _split_refs:
        _split_refs[case[0]] = (G.conv_ref(src0, src1, w, **kw), G.conv_ref(src0, src1, w, **bare))
    ref, ref_bare = _split_refs[case[0]]
    got = {t: _call_with_slabs(src0, src1, w, t, ksplit, **kw) for t in FORMS}
    out27, slabs27 = got[27]
    assert bool(torch.isfinite(slabs27).all())            # every slab element written (the scratch was NaN)
    G.assert_close(out27, ref, what='%s ksplit %d tile 27' % (case[0], ksplit))
    # the slabs are bare partial sums: together they are the conv without its epilogue terms
    G.assert_close(G.nchw(slabs27.double().sum(0)).float(), ref_bare, what=case[0] + ' slab sum')
    for t in (28, 29):
        out, slabs = got[t]
        assert torch.equal(slabs, slabs27), '%s ksplit %d: the slabs of tile %d differ' % (case[0], ksplit, t)
        assert torch.equal(out, out27), '%s ksplit %d: the reduced output of tile %d differs' % (case[0], ksplit, t)


def test_wide_forms_refuse_a_residual_split_off_a_quad():
    """RC0 % 4 == 0 is what lets a lane load its four residual channels from ONE source: 28 / 29 refuse anything else before a launch,
    the 4-byte form takes it."""
    case = ('r32_res_62_66', (32, 128), 1, 32, 0, 4, 8, 128, 1, 1, 0, True, False, (62, 66))
    src0, src1, w, kw = _make(case)
    out, _ = G.conv_call(src0, src1, w, tile_cfg=27, ksplit=1, **kw)
    G.assert_close(out, G.conv_ref(src0, src1, w, **kw), what='RC0 62 on tile 27')
    for t in (28, 29):
        with pytest.raises(L.Sr3Error, match='RC0'):
            G.conv_call(src0, src1, w, tile_cfg=t, ksplit=1, **kw)


# ---- whole paths: res_conv, qkv, out and both Downsamples of this network run on tile 22 ----
CFG = dict(which='sr3', in_channel=6, inner=32, groups=8, mults=[2, 4, 4], attn=[16], rb=1, size=32, cond=True)
B = 4
_net = {}


def _netG():
    if 'netG' not in _net:
        import model.networks as networks
        opt = make_opt(CFG, T=100)
        opt['phase'] = 'val'
        torch.manual_seed(29)
        netG = networks.define_G(opt).to(G.dev())
        netG.set_new_noise_schedule(opt['model']['beta_schedule']['val'], G.dev())
        netG.show_progress = False
        _net['netG'] = netG
    return _net['netG']


def _forward(form):
    un = _netG().denoise_fn
    un.plan.set_option('gemm_epi', form)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, 6, 32, 32, generator=g).to(G.dev())
    lvl = (torch.rand(B, 1, generator=g) * 0.9 + 0.05).to(G.dev())
    return un(x, lvl).clone()


def test_forward_has_the_same_bits_under_every_form():
    e0 = _forward(0)
    assert bool(torch.isfinite(e0).all())
    ops = [o for o in _netG().denoise_fn.plan.op_list(B) if o['kind'] == 50 and o['tile_cfg'] == 22]
    assert any(o['ksize'] == 1 for o in ops) and sum(1 for o in ops if o['ksize'] == 3 and o['stride'] == 2) == 2
    assert any(o['ksize'] == 1 and o['cout'] == 3 * o['cin'] for o in ops)       # qkv
    assert any(o['ksize'] == 1 and o['cout'] % 128 for o in ops) and any(o['ksize'] == 1 and o['cout'] % 128 == 0 for o in ops)
    for form in (1, 2):
        e = _forward(form)
        assert torch.equal(e, e0), 'gemm_epi = %d: %d of %d elements differ' % (form, int((e != e0).sum()), e.numel())


def test_three_replays_of_the_captured_step_are_bit_identical():
    netG = _netG()
    un = netG.denoise_fn
    d = G.dev()
    shape = (B, 3, 32, 32)
    g = torch.Generator().manual_seed(9)
    x0 = torch.randn(shape, generator=g)
    cond = torch.rand(shape, generator=g) * 2 - 1
    got = {}
    for form in (0, 2):
        un.plan.set_option('gemm_epi', form)
        st = netG._loop_state(shape, shape, d)
        un.ensure_derived()
        netG._capture(st)
        st['img'].copy_(x0); st['cond'].copy_(cond); st['step'].fill_(60)
        torch.manual_seed(31)
        imgs = []
        for _ in range(3):
            st['graph'].replay()
            imgs.append(st['img'].clone())
        torch.cuda.synchronize()
        assert int(st['step'][1].item()) == 57
        got[form] = imgs
    for i in range(3):
        assert torch.equal(got[0][i], got[2][i]), 'replay %d differs' % i
    assert bool(torch.isfinite(got[2][2]).all()) and not torch.equal(got[2][0], got[2][2])


def test_one_training_step_has_the_same_loss_and_weights():
    """optimize_parameters from the same weights and seed: the training forward and the 1x1 / stride-2 data gradients run the same kernel,
    so the loss and the parameter arena after Adam are bit-equal between gemm_epi 0 and 2."""
    import model as Model
    g = torch.Generator().manual_seed(13)
    hr = torch.rand(B, 3, 32, 32, generator=g) * 2 - 1
    sr = torch.rand(B, 3, 32, 32, generator=g) * 2 - 1
    got = {}
    for form in (0, 2):
        opt = make_opt(CFG, T=100)
        torch.manual_seed(29)
        m = Model.create_model(opt)
        un = m.netG.denoise_fn
        un.plan.set_option('gemm_epi', form)
        m.feed_data({'HR': hr.clone(), 'SR': sr.clone()})
        torch.manual_seed(41)
        np.random.seed(41)                                # (the timestep and the noise level of the step come from numpy's generator)
        m.optimize_parameters()
        torch.cuda.synchronize()
        got[form] = (float(m.get_current_log()['l_pix']), un.arena.data.clone())
    assert got[0][0] == got[2][0] and got[0][0] == got[0][0], (got[0][0], got[2][0])
    assert bool(torch.isfinite(got[2][1]).all())
    assert torch.equal(got[0][1], got[2][1]), 'the weights after Adam differ in %d elements' % int((got[0][1] != got[2][1]).sum())
