"""sr3_unet_forward_profile, the per-launch timing entry (and the only caller that hands conv_forward an event to record between a conv and its
split-K reduce): one entry per plan op plus a kind-59 entry behind every split-K conv, the kernel numbers of csrc/tile_code.h, and the same eps
as sr3_unet_forward."""
import ctypes as C
import json
import math
import os

import pytest
import torch

from helpers import DESCS, GOLDEN, opt_for

pytestmark = pytest.mark.gpu

# the smallest network of helpers.py whose default batch-1 plan has a split-K conv (checked below)
NAME = 'sr3_seam'
OP_CONV, KIND_REDUCE = 50, 59


def split_convs(ops):
    return [o['kind'] == OP_CONV and o['ksplit'] > 1 for o in ops]


def run_profile():
    """(launch list, split-K flag per op, op_kind, op_ms, eps of the profile call, eps of sr3_unet_forward) of one batch-1 forward of NAME"""
    import model as Model
    from sr3_hip import engine as E, lib as L
    torch.manual_seed(7)
    un = Model.create_model(opt_for(NAME, phase='val', gpu=True)).netG.denoise_fn
    plan, lib, dev = un.plan, L.load(), un.weights().device
    ops = plan.op_list(1)
    split = split_convs(ops)
    assert any(split), 'the plan of %s has no split-K conv: nothing here would run the mid event' % NAME
    for d in DESCS.values():
        other = E.Plan(d['variant'], d['in_channel'], d['out_channel'], d['inner_channel'], d['norm_groups'], d['channel_mults'], d['attn_res'],
                       d['res_blocks'], d['image_size'])
        assert other.param_floats >= plan.param_floats or not any(split_convs(other.op_list(1))), d

    S = DESCS[NAME]['image_size']
    x, cond = torch.randn(1, 3, S, S, device=dev), torch.rand(1, 3, S, S, device=dev) * 2 - 1
    level = torch.full((1,), 0.5, device=dev)
    ref = un(x, level, cond=cond).clone()      # sr3_unet_forward (and the derived filters, prepared)

    wsbuf, need = un._ws.get(plan, 1, dev)
    out = torch.empty_like(ref)
    max_ops = 2 * len(ops)
    ms, kind, fl, n = (C.c_float * max_ops)(), (C.c_int * max_ops)(), (C.c_double * max_ops)(), C.c_int()
    L.check(lib.sr3_unet_forward_profile(plan.handle, L.ptr(x), L.ptr(cond), 3, L.ptr(level), None, L.ptr(un.freq), L.ptr(un.weights()),
                                         L.ptr(wsbuf), need, L.ptr(out), 1, C.c_void_p(torch.cuda.current_stream().cuda_stream), max_ops,
                                         ms, kind, fl, C.byref(n)))
    torch.cuda.synchronize()
    return ops, split, [int(k) for k in kind[:n.value]], list(ms[:n.value]), out, ref


def test_profile_follows_the_launch_list():
    ops, split, kinds, ms, out, ref = run_profile()
    assert len(kinds) == len(ops) + sum(split)
    # every kind-59 entry sits directly behind a split-K conv, and every split-K conv has one
    j, behind = -1, []
    for i, k in enumerate(kinds):
        if k == KIND_REDUCE:
            assert i > 0 and kinds[i - 1] != KIND_REDUCE and split[j], (i, kinds)
            behind.append(j)
        else:
            j += 1
    assert j == len(ops) - 1 and behind == [i for i, s in enumerate(split) if s]
    assert all(math.isfinite(t) and t >= 0.0 for t in ms), ms
    assert torch.equal(out, ref)
    with open(os.path.join(GOLDEN, 'profile_kinds.json')) as f:
        golden = json.load(f)
    assert golden['network'] == NAME and kinds == golden['op_kind']
