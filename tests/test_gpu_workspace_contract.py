"""The workspace contract of the whole-network entries, through the C ABI alone (the test owns every byte):

  1. a buffer of exactly the queried size is enough,
  2. nothing outside it is written,
  3. what it held before the call does not matter.

sr3_unet_forward, sr3_reverse_step_hist and sr3_train_step_ex run in guarded buffers (tests/guarded.py) of exactly
sr3_workspace_bytes / sr3_train_workspace_bytes / sr3_plan_derived_bytes, pre-filled with zeros (Z), NaN patterns (N) and a large
finite pattern (F); the results must be finite and BIT-equal across the fills, every band must be intact, and one comparison with the
oracle per case keeps bit-equality from passing on equally wrong results.  A stale-history sequence then runs different launch
lists one after another in one buffer that is never refilled.  No buffer is ever passed smaller than its query here (the refusals of
undersized buffers are checked without a device, tests/test_scratch_contract_cpu.py).

The network is small (inner 64, three levels, 32 x 32) but its launch lists hold the production kernels -- asserted per case from
plan.op_list: the two-workgroup Winograd tile 13 at split-K 1..4, the plain GEMM tile 22 at split-K 1 / 2 / 4, fused output
statistics, the MFMA input conv with fused statistics, attention; the halo tile 5 on the 8 x 8 maps at batch 3, the four-image
Winograd tile 12 at batch 4; at 24 x 40 the ragged tile 23 (split-K 1..4), tile 16 (incl. split-K 6) and tile 3.

Bounds: forward 2e-5 * max(1, |ref|_inf) against the fp32 oracle; training gradients normwise 1e-4 where
|ref| > 1e-6 and the loss rel 1e-5 (tests/test_gpu_train.py), here against float64 autograd over the oracle under the L2 objective."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util as G                                             # noqa: E402
import guarded as GD                                             # noqa: E402
from guarded import Guarded, Z, N, F                             # noqa: E402
from sr3_hip import engine as E, lib as L                        # noqa: E402

NET = dict(inner_channel=64, norm_groups=32, channel_mults=[1, 2, 2], attn_res=[8], res_blocks=1, image_size=32)
IN_CH = {'sr3': 6, 'ddpm': 3}
NATIVE, RECT = (32, 32), (24, 40)
DROP_SEED = 20240917

_NETS = {}


class Net(object):
    """One variant's weights (the reference's default init through the drop-in model package, seeded; GroupNorm scale / shift moved
    off 1 / 0 so that they matter), as the oracle's state dict and as a guarded device arena."""

    def __init__(self, variant):
        if variant == 'sr3':
            from model.sr3_modules.unet import UNet
        else:
            from model.ddpm_modules.unet import UNet
        torch.manual_seed(4711)
        un = UNet(in_channel=IN_CH[variant], out_channel=3, inner_channel=NET['inner_channel'], norm_groups=NET['norm_groups'],
                  channel_mults=NET['channel_mults'], attn_res=NET['attn_res'], res_blocks=NET['res_blocks'], dropout=0,
                  image_size=NET['image_size'])
        arena = un.arena.data
        gen = torch.Generator().manual_seed(4712)
        for e in un.plan.table:
            if '.block.0.' in e['name'] or '.norm.' in e['name']:
                arena[e['offset']:e['offset'] + e['numel']] += 0.1 * torch.randn(e['numel'], generator=gen)
        self.variant = variant
        self.desc = dict(NET, variant=variant, in_channel=IN_CH[variant], out_channel=3)
        self.sd = {k: v.clone() for k, v in un.state_dict(prefix='denoise_fn.').items()}
        self.table = un.plan.table
        self.param_floats = un.plan.param_floats
        self.cc = 3 if variant == 'sr3' else 0
        d = G.dev()
        self.arena_g, self.arena = GD.tensor_in(arena, d)
        self.freq_g, self.freq = GD.tensor_in(un.plan.default_freq(), d)
        self.is_param = torch.zeros(self.param_floats, dtype=torch.bool)
        for e in self.table:
            self.is_param[e['offset']:e['offset'] + e['numel']] = True
        self.is_param_dev = self.is_param.to(d)

    def plan(self, **options):
        p = E.Plan(self.variant, IN_CH[self.variant], 3, NET['inner_channel'], NET['norm_groups'], NET['channel_mults'], NET['attn_res'],
                   NET['res_blocks'], NET['image_size'])
        for k, v in options.items():
            p.set_option(k, v)
        assert p.param_floats == self.param_floats
        return p


def net(variant):
    if variant not in _NETS:
        _NETS[variant] = Net(variant)
    return _NETS[variant]


def bits(t):
    return t.contiguous().view(torch.int32)


def bind_derived(plan, nt, fill=Z):
    """A guarded buffer of exactly sr3_plan_derived_bytes, filled, bound and prepared from the arena."""
    lib = plan.lib
    need = int(lib.sr3_plan_derived_bytes(plan.handle))
    assert need > 0
    dg = Guarded(need, fill, G.dev())
    L.check(lib.sr3_plan_bind_derived(plan.handle, dg.ptr, need))
    L.check(lib.sr3_plan_prepare_derived(plan.handle, nt.arena_g.ptr, G.stream()))
    torch.cuda.synchronize()
    assert dg.intact(), 'sr3_plan_prepare_derived wrote outside its %d bytes' % need
    return dg


def reprepare(plan, nt, dg, fill):
    dg.fill(fill)
    L.check(plan.lib.sr3_plan_invalidate_derived(plan.handle))
    L.check(plan.lib.sr3_plan_prepare_derived(plan.handle, nt.arena_g.ptr, G.stream()))
    torch.cuda.synchronize()
    assert dg.intact(), 'sr3_plan_prepare_derived wrote outside its buffer (fill 0x%02X)' % fill


def conv_cfgs(plan, B):
    return set((o['tile_cfg'], o['ksplit']) for o in plan.op_list(B) if o['kind'] == 50)


def assert_launch_list(plan, B, geo, winograd=1):
    """The kernels the case is meant to cover are in its launch list (a heuristic change that moves them away fails here)."""
    ops = plan.op_list(B)
    cfgs = conv_cfgs(plan, B)
    assert any(o['kind'] == 60 for o in ops), 'no attention op'
    assert any(o['kind'] == 50 and o['fused_output_stats'] for o in ops), 'no conv with fused output statistics'
    if not winograd:
        assert not [c for c in cfgs if c[0] in (11, 12, 13, 23)], cfgs
        assert {(5, 1), (5, 2), (5, 4), (6, 1), (22, 1), (22, 2), (22, 4)} <= cfgs, cfgs
        return
    if geo == NATIVE:
        assert any(o['kind'] == 20 and o['fused_output_stats'] for o in ops), 'the input conv does not fuse its statistics'
        assert {(13, 1), (13, 2), (13, 3), (13, 4), (22, 1), (22, 2), (22, 4)} <= cfgs, cfgs
        if B % 4 == 0:
            assert {(12, 2), (12, 4)} <= cfgs, cfgs
        else:
            assert {(5, 2), (5, 4)} <= cfgs, cfgs
    else:
        assert {(23, 1), (23, 2), (23, 3), (23, 4), (16, 1), (16, 6), (22, 1)} <= cfgs and any(c[0] == 3 for c in cfgs), cfgs


# ---- forward -----------------------------------------------------------------------------------------------------------------------

FWD_CASES = {
    'sr3_b3': ('sr3', 3, NATIVE, 1),
    'sr3_b4': ('sr3', 4, NATIVE, 1),
    'sr3_b3_24x40': ('sr3', 3, RECT, 1),
    'sr3_b1_direct': ('sr3', 1, NATIVE, 0),
    'ddpm_b4': ('ddpm', 4, NATIVE, 1),
}
_FWD_IN = {}
_FWD_FRESH = {}


def fwd_inputs(case):
    """(guards, x, cond, level, tstep, oracle output), made once per case and never changed."""
    if case not in _FWD_IN:
        from oracle import sr3_oracle as O
        variant, B, (H, W), _ = FWD_CASES[case]
        nt, d = net(variant), G.dev()
        g = torch.Generator().manual_seed(100 + len(case) + B)
        x = torch.randn(B, 3, H, W, generator=g)
        cond = torch.rand(B, 3, H, W, generator=g) * 2 - 1
        level = 0.05 + 0.9 * torch.rand(B, generator=g)
        tstep = torch.randint(0, 2000, (B,), generator=g)
        with torch.no_grad():
            if variant == 'sr3':
                ref = O.unet_forward(nt.sd, nt.desc, torch.cat([cond, x], 1), level.view(B, 1))
            else:
                ref = O.unet_forward(nt.sd, nt.desc, x, tstep)
        xg, xd = GD.tensor_in(x, d)
        cg, cd = GD.tensor_in(cond, d)
        lg, ld = GD.tensor_in(level, d)
        tg, td = GD.tensor_in(tstep, d)
        _FWD_IN[case] = dict(guards=[xg, cg, lg, tg], x=xg, cond=cg if variant == 'sr3' else None, level=lg if variant == 'sr3' else None,
                             tstep=tg if variant == 'ddpm' else None, ref=ref)
    return _FWD_IN[case]


def run_forward(plan, nt, case, ws, ws_bytes):
    """One sr3_unet_forward of the case in the workspace `ws` (of which `ws_bytes`, the query, are handed over); returns the output
    on the host after checking rc, finiteness and every band but the workspace's own."""
    variant, B, (H, W), _ = FWD_CASES[case]
    inp = fwd_inputs(case)
    og, out = GD.tensor_out((B, 3, H, W), G.dev())
    p = lambda g: None if g is None else g.ptr
    rc = plan.lib.sr3_unet_forward(plan.handle, inp['x'].ptr, p(inp['cond']), nt.cc, p(inp['level']), p(inp['tstep']), nt.freq_g.ptr, None,
                                   None, nt.arena_g.ptr, ws.ptr, ws_bytes, og.ptr, B, G.stream())
    assert rc == 0, plan.lib.sr3_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()), '%s: %d non-finite output elements' % (case, int((~torch.isfinite(out)).sum()))
    assert og.intact(), '%s: the forward wrote outside its output' % case
    for g_ in inp['guards'] + [nt.arena_g, nt.freq_g]:
        assert g_.intact(), '%s: an input band was written' % case
    return out.cpu()


def fwd_plan(case):
    variant, B, geo, winograd = FWD_CASES[case]
    nt = net(variant)
    plan = nt.plan(**({} if winograd else {'winograd': 0}))
    plan.set_geometry(*geo)
    assert_launch_list(plan, B, geo, winograd)
    return nt, plan, plan.workspace_bytes(B)


def fwd_fresh(case):
    """The case's output in a zero-filled workspace of exactly the queried size (computed once)."""
    if case not in _FWD_FRESH:
        nt, plan, need = fwd_plan(case)
        dg = bind_derived(plan, nt)
        ws = Guarded(need, Z, G.dev())
        _FWD_FRESH[case] = run_forward(plan, nt, case, ws, need)
        assert ws.intact() and dg.intact()
    return _FWD_FRESH[case]


def describe_diff(a, b):
    """Where two outputs differ: count and first NCHW positions (they name the layer / lane that read stale memory)."""
    ne = (bits(a) != bits(b)).nonzero()
    return '%d of %d elements differ, first at %s, max |diff| %.3g' % (len(ne), a.numel(), ne[:4].tolist(), float((a - b).abs().max()))


@pytest.mark.parametrize('case', list(FWD_CASES))
def test_forward_ignores_workspace_and_derived_contents(case):
    nt, plan, need = fwd_plan(case)
    variant, B, geo, _ = FWD_CASES[case]
    base = fwd_fresh(case)
    ref = fwd_inputs(case)['ref']
    err = G.assert_close(base, ref, tol=2e-5, what='%s forward vs oracle' % case)
    print('%s: workspace %d bytes, forward max abs err vs oracle %.2e (|ref|max %.2f)' % (case, need, err, ref.abs().max().item()))
    dg = bind_derived(plan, nt)
    ws = Guarded(need, Z, G.dev())
    for name, byte in GD.FILLS:
        ws.fill(byte)
        out = run_forward(plan, nt, case, ws, need)
        assert ws.intact(), '%s: the forward wrote outside its %d workspace bytes (fill %s)' % (case, need, name)
        assert dg.intact(), '%s: the forward wrote outside the derived buffer (fill %s)' % (case, name)
        assert torch.equal(bits(out), bits(base)), '%s: workspace fill %s changes the output: %s' % (case, name, describe_diff(out, base))
    for name, byte in GD.FILLS[1:]:
        reprepare(plan, nt, dg, byte)
        ws.fill(Z)
        out = run_forward(plan, nt, case, ws, need)
        assert ws.intact() and dg.intact()
        assert torch.equal(bits(out), bits(base)), '%s: derived-buffer fill %s changes the output: %s' % (case, name, describe_diff(out, base))


def test_forward_ignores_another_launch_lists_leftovers():
    """One workspace sized for the largest call, filled with NaN patterns once and never again: four forwards with different launch
    lists run in it one after the other, each handed exactly its queried byte count; each output is the fresh-buffer one."""
    seq = ['sr3_b4', 'sr3_b3', 'sr3_b3_24x40', 'sr3_b4']
    nt = net('sr3')
    plan = nt.plan()
    needs = {}
    for case in set(seq):
        plan.set_geometry(*FWD_CASES[case][2])
        needs[case] = plan.workspace_bytes(FWD_CASES[case][1])
    dg = bind_derived(plan, nt)
    ws = Guarded(max(needs.values()), N, G.dev())
    for i, case in enumerate(seq):
        plan.set_geometry(*FWD_CASES[case][2])
        out = run_forward(plan, nt, case, ws, needs[case])
        assert ws.intact() and dg.intact()
        base = fwd_fresh(case)
        assert torch.equal(bits(out), bits(base)), 'call %d (%s) in a reused workspace: %s' % (i, case, describe_diff(out, base))


def test_reverse_step_ignores_workspace_contents():
    """sr3_reverse_step_hist without history (the fused step the sampling graphs replay): x after the step and the step counter."""
    case = 'sr3_b3'
    nt, plan, need = fwd_plan(case)
    variant, B, (H, W), _ = FWD_CASES[case]
    inp = fwd_inputs(case)
    d = G.dev()
    T, t = 8, 5
    g = torch.Generator().manual_seed(77)
    tabs = [GD.tensor_in(v, d)[0] for v in (1.0 + torch.rand(T, generator=g), 0.5 * torch.rand(T, generator=g), 0.3 * torch.rand(T, generator=g),
                                           0.7 * torch.rand(T, generator=g), 0.1 * torch.rand(T, generator=g))]
    lvl_g, _ = GD.tensor_in(0.05 + 0.9 * torch.rand(T + 1, generator=g), d)
    zg, _ = GD.tensor_in(torch.randn(B, 3, H, W, generator=g), d)
    x0 = inp['x'].view(torch.float32, (B, 3, H, W)).clone()
    dg = bind_derived(plan, nt)
    ws = Guarded(need, Z, d)
    outs = []
    for name, byte in GD.FILLS:
        ws.fill(byte)
        xg, xv = GD.tensor_out((B, 3, H, W), d)
        xv.copy_(x0)
        sg, sv = GD.tensor_out((2,), d, dtype=torch.int32)
        sv.copy_(torch.tensor([byte, t], dtype=torch.int32))          # (step2[0] is the step's own scratch: prior contents arbitrary)
        rc = plan.lib.sr3_reverse_step_hist(plan.handle, xg.ptr, inp['cond'].ptr, nt.cc, nt.freq_g.ptr, lvl_g.ptr, sg.ptr, nt.arena_g.ptr,
                                            ws.ptr, need, zg.ptr, tabs[0].ptr, tabs[1].ptr, tabs[2].ptr, tabs[3].ptr, tabs[4].ptr, 1, None, B,
                                            G.stream(), None, None, None)
        assert rc == 0, plan.lib.sr3_last_error()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(xv).all()) and int(sv[1]) == t - 1
        for g_ in [ws, dg, xg, sg, zg, lvl_g, nt.arena_g, nt.freq_g] + tabs + inp['guards']:
            assert g_.intact(), 'reverse step wrote outside a buffer (fill %s)' % name
        outs.append(xv.cpu())
        assert not torch.equal(outs[-1], x0.cpu())          # the step really updated x
    for (name, _), o in zip(GD.FILLS[1:], outs[1:]):
        assert torch.equal(bits(o), bits(outs[0])), 'reverse step: workspace fill %s changes x: %s' % (name, describe_diff(o, outs[0]))


# ---- training step -----------------------------------------------------------------------------------------------------------------

TRAIN_CASES = {
    'sr3_b4': ('sr3', 4, NATIVE, 0.0),
    'sr3_b3_dropout': ('sr3', 3, NATIVE, 0.2),
    'sr3_b2_24x40': ('sr3', 2, RECT, 0.0),
    'ddpm_b4': ('ddpm', 4, NATIVE, 0.0),
}
_TRAIN_IN = {}
_TRAIN_FRESH = {}
_TRAIN_PLANS = {}


def train_inputs(case):
    if case not in _TRAIN_IN:
        variant, B, (H, W), _ = TRAIN_CASES[case]
        d = G.dev()
        g = torch.Generator().manual_seed(300 + len(case) + B)
        t = dict(hr=torch.rand(B, 3, H, W, generator=g) * 2 - 1, sr=torch.rand(B, 3, H, W, generator=g) * 2 - 1,
                 z=torch.randn(B, 3, H, W, generator=g), gamma=0.2 + 0.75 * torch.rand(B, generator=g),
                 tstep=torch.randint(0, 2000, (B,), generator=g))
        t['ca'] = t['gamma'].clone()
        t['cb'] = (1 - t['gamma'] ** 2).sqrt()
        _TRAIN_IN[case] = dict(cpu=t, dev={k: GD.tensor_in(v, d)[0] for k, v in t.items()})
    return _TRAIN_IN[case]


def train_plan(variant, geo, train_geom=None):
    """The plan a case trains on, with its derived filters in a guarded buffer: the default-option plan at the native size (what most
    callers run), a plan under train_geom off it.  train_geom 1 forces the option at the native size too (the equivalence test)."""
    if train_geom is None:
        train_geom = int(geo != NATIVE)
    key = (variant, train_geom)
    if key not in _TRAIN_PLANS:
        nt = net(variant)
        plan = nt.plan(**({'train_geom': 1} if train_geom else {}))
        _TRAIN_PLANS[key] = (nt, plan, bind_derived(plan, nt))
    nt, plan, dg = _TRAIN_PLANS[key]
    if train_geom:
        plan.set_geometry(*geo)
    return nt, plan, dg


def train_need(case, train_geom=None):
    variant, B, geo, _ = TRAIN_CASES[case]
    nt, plan, dg = train_plan(variant, geo, train_geom)
    assert_launch_list(plan, B, geo)
    need = int(plan.lib.sr3_train_workspace_bytes(plan.handle, B, nt.cc))
    assert need > 0, plan.lib.sr3_last_error()
    return need


def run_train(case, ws, ws_bytes, grad_fill, loss_kind=-1, train_geom=None):
    """One sr3_train_step_ex in `ws`; returns (loss bits, gradient arena on the device) after checking rc and every band but ws's."""
    variant, B, (H, W), p_drop = TRAIN_CASES[case]
    nt, plan, dg = train_plan(variant, (H, W), train_geom)
    dv = train_inputs(case)['dev']
    d = G.dev()
    gg = Guarded(nt.param_floats * 4, grad_fill, d, GD.TENSOR_BAND)
    lg, lv = GD.tensor_out((1,), d)
    sr3 = variant == 'sr3'
    rc = plan.lib.sr3_train_step_ex(plan.handle, dv['hr'].ptr, dv['sr'].ptr if sr3 else None, nt.cc, dv['z'].ptr, dv['ca'].ptr, dv['cb'].ptr,
                                    dv['gamma'].ptr if sr3 else None, None if sr3 else dv['tstep'].ptr, nt.freq_g.ptr, nt.arena_g.ptr, gg.ptr,
                                    ws.ptr, ws_bytes, lg.ptr, C.c_float(1.0 / (B * 3 * H * W)), C.c_float(p_drop), C.c_uint(DROP_SEED), 0, None,
                                    None, B, None, None, None, loss_kind, C.c_float(0.0), G.stream())
    assert rc == 0, plan.lib.sr3_last_error()
    torch.cuda.synchronize()
    for g_ in [gg, lg, dg, nt.arena_g, nt.freq_g] + list(dv.values()):
        assert g_.intact(), '%s: the training step wrote outside a buffer' % case
    grads = gg.view(torch.float32)
    assert bool(torch.isfinite(lv).all()), '%s: loss %s' % (case, lv)
    nonfinite = (~torch.isfinite(grads)) & nt.is_param_dev
    assert not bool(nonfinite.any()), '%s: %d non-finite gradients, first at arena offset %d' % (case, int(nonfinite.sum()),
                                                                                              int(nonfinite.nonzero()[0]))
    return int(bits(lv)[0]), grads.clone()


def train_fresh(case):
    """Loss bits and gradient arena of the case in a zero-filled workspace of exactly the queried size, gradients pre-filled with NaN."""
    if case not in _TRAIN_FRESH:
        need = train_need(case)
        ws = Guarded(need, Z, G.dev())
        _TRAIN_FRESH[case] = run_train(case, ws, need, N)
        assert ws.intact(), '%s: the training step wrote outside its %d workspace bytes' % (case, need)
    return _TRAIN_FRESH[case]


def assert_same_step(case, got, base, what):
    """Loss and every parameter's gradient bit-equal; the arena's padding floats (no parameter's) are WRITTEN by the step -- the output
    conv's bias slot is 4 floats wide and receives the column sums of dOut's four lanes, the pad lane's being +0 -- so they are 0
    whatever the arena held (include/sr3_mi355x.h at sr3_train_step)."""
    nt = net(TRAIN_CASES[case][0])
    assert got[0] == base[0], '%s: %s changes the loss bits' % (case, what)
    gb, bb = bits(got[1]), bits(base[1])
    ne = (gb != bb) & nt.is_param_dev
    if bool(ne.any()):
        offs = ne.nonzero().flatten()
        first = int(offs[0])
        owner = [e['name'] for e in nt.table if e['offset'] <= first < e['offset'] + e['numel']]
        raise AssertionError('%s: %s changes %d gradient floats, first at arena offset %d (%s), max |diff| %.3g'
                             % (case, what, len(offs), first, owner, float((got[1] - base[1])[ne].abs().max())))
    pad = ~nt.is_param_dev
    assert int(pad.sum()) >= 1          # (the output conv's 3-float bias in its 4-float slot)
    assert bool((gb[pad] == 0).all()), '%s: %s: padding floats of the gradient arena are not +0: %s' % (case, what, got[1][pad][:8].tolist())


@pytest.mark.parametrize('case', list(TRAIN_CASES))
def test_training_step_ignores_workspace_and_arena_contents(case):
    need = train_need(case)
    base = train_fresh(case)
    assert_same_step(case, base, base, 'nothing')
    ws = Guarded(need, Z, G.dev())
    for ws_name, ws_fill, grad_fill in (('N', N, N), ('F', F, N), ('Z', Z, F)):
        ws.fill(ws_fill)
        got = run_train(case, ws, need, grad_fill)
        assert ws.intact(), '%s: the training step wrote outside its %d workspace bytes (fill %s)' % (case, need, ws_name)
        assert_same_step(case, got, base, 'workspace fill %s / gradient-arena fill 0x%02X' % (ws_name, grad_fill))
    print('%s: training workspace %d bytes, loss %r' % (case, need, torch.tensor([base[0]], dtype=torch.int32).view(torch.float32).item()))


def test_training_step_ignores_another_steps_leftovers():
    """One workspace sized for the largest step, NaN-filled once: four steps with different launch lists in a row."""
    seq = ['sr3_b4', 'sr3_b2_24x40', 'sr3_b3_dropout', 'sr3_b4']
    needs = {case: train_need(case) for case in set(seq)}
    ws = Guarded(max(needs.values()), N, G.dev())
    for i, case in enumerate(seq):
        got = run_train(case, ws, needs[case], N)
        assert ws.intact()
        assert_same_step(case, got, train_fresh(case), 'call %d of a reused workspace' % i)


def test_native_step_under_train_geom_is_the_default_plans_step():
    """include/sr3_mi355x.h on plan option train_geom: at image_size x image_size the workspace bytes and every bit of the result are
    those of train_geom = 0 -- here in a NaN-filled workspace, against the default plan's zero-filled run."""
    for case in ('sr3_b4', 'sr3_b3_dropout'):
        need = train_need(case, train_geom=1)
        assert need == train_need(case)
        ws = Guarded(need, N, G.dev())
        got = run_train(case, ws, need, N, train_geom=1)
        assert ws.intact()
        assert_same_step(case, got, train_fresh(case), 'plan option train_geom = 1')


def test_training_step_in_a_dirty_workspace_matches_float64_autograd():
    """The correctness anchor of the bit comparisons: the batch-4 step under the L2 objective (the L1 loss's sign kinks make a
    single-draw comparison meaningless), run in a NaN-filled workspace into a NaN-filled arena, against float64 autograd over the
    oracle: loss rel 1e-5, every parameter gradient normwise 1e-4 where |ref| > 1e-6 (the bounds of tests/test_gpu_train.py)."""
    from oracle import sr3_oracle as O
    import grad_ref as R
    case = 'sr3_b4'
    nt = net('sr3')
    need = train_need(case)
    ws = Guarded(need, N, G.dev())
    loss_bits, grads = run_train(case, ws, need, N, loss_kind=1)
    assert ws.intact()
    loss = torch.tensor([loss_bits], dtype=torch.int32).view(torch.float32).item()
    t = train_inputs(case)['cpu']
    d = G.dev()
    sdr = {k: v.clone().requires_grad_(k.startswith('denoise_fn.')) for k, v in R.to_double(nt.sd, d).items()}
    f = lambda v: v.to(device=d, dtype=torch.float64)
    ref_loss = O.p_losses_sr3(sdr, nt.desc, f(t['hr']), f(t['sr']), f(t['gamma']), f(t['z']), conditional=True, loss_type='l2')
    (ref_loss / t['hr'].numel()).backward()
    ref_loss = float(ref_loss.detach())
    plan = train_plan('sr3', NATIVE)[1]
    rows = []
    for e in nt.table:
        ref = sdr['denoise_fn.' + e['name']].grad
        got = plan.view(grads, e).double()
        den = max(ref.norm().item(), 1e-7)
        rows.append(((got - ref).norm().item() / den, e['name'], den))
    rows.sort(reverse=True)
    counted = [r for r in rows if r[2] > 1e-6]
    print('L2 training step in a NaN-filled workspace, batch 4: loss rel err %.1e, worst gradient rel err vs float64 %.1e (%s), median '
          '%.1e over %d tensors' % (abs(loss - ref_loss) / abs(ref_loss), counted[0][0], counted[0][1], counted[len(counted) // 2][0], len(counted)))
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    bad = [r for r in counted if r[0] > 1e-4]
    assert len(counted) > 100 and not bad, bad[:8]
