#!/usr/bin/env python3
"""What multi-head attention (sr3_attention_heads_f32, plan options attn_heads / attn_head_dim) costs next to the single head, GPU only.
Device-event times after a warm-up, the forms of one table ALTERNATED in one process (round-robin, best of `--rounds` rounds):

  (1) forward per op at (16, 256, 512) and (16, 64, 512), split arithmetic (mode 1, the plans' default): one 512-wide head (today's
      kernel), 8 heads of 64 on k_attention_heads, and the same 8 heads forced onto the strided generic kernel (mode bit 2);
  (2) backward per op at (64, 256, 512): one head against 8;
  (3) the C2 reverse step (SR3 16 -> 128, batch 16, graph replay) and the C3 training step (batch 64, dropout as configured,
      optimize_parameters) with model.unet.head_dim = 64 against the same tree with the key absent.

    python tools/attn_heads_probe.py [--launches 50] [--rounds 5] [--out profiles/attn_heads_probe.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd')


def alternate(torch, forms, launches, rounds):
    """forms: {name: callable}; -> {name: best us per call} with the forms taken in turn inside every round."""
    for f in forms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    best = {k: 1e30 for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                f()
            e1.record()
            torch.cuda.synchronize()
            best[k] = min(best[k], e0.elapsed_time(e1) * 1e3 / launches)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=30, help='graph replays per timing of the reverse step')
    ap.add_argument('--train-steps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'attn_heads_probe.json'))
    a = ap.parse_args()
    for p in (os.path.join(ROOT, 'tools'), os.path.join(ROOT, 'tests'), ROOT, PKG):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import bench
    import gpu_util as G
    import model as Model
    import model.networks as networks
    from sr3_hip import lib as L
    lib, d = L.load(), G.dev()
    rec = {'what': 'tools/attn_heads_probe.py: device-event times, forms alternated in one process, best of %d rounds' % a.rounds,
           'device': torch.cuda.get_device_name(0), 'launches': a.launches, 'forward_us': [], 'backward_us': [], 'networks': {}}

    for B, N, C in ((16, 256, 512), (16, 64, 512)):
        qkv = torch.randn(B, N, 3 * C, device=d)
        out = torch.empty(B, N, C, device=d)
        call = lambda heads, mode: (lambda: L.check(lib.sr3_attention_heads_f32(L.ptr(qkv), B, N, C, heads, L.ptr(out), mode, G.stream())))
        t = alternate(torch, {'heads1_k_attention_v2': call(1, 1), 'heads8_k_attention_heads': call(8, 1), 'heads8_strided_generic': call(8, 5),
                              'heads8_k_attention_heads_fp32': call(8, 0)}, a.launches, a.rounds)
        row = dict(B=B, N=N, C=C, mode='1 (split) unless named', **{k: round(v, 2) for k, v in t.items()})
        row['new_kernel_over_strided'] = round(t['heads8_k_attention_heads'] / t['heads8_strided_generic'], 3)
        row['new_kernel_over_single_head'] = round(t['heads8_k_attention_heads'] / t['heads1_k_attention_v2'], 3)
        rec['forward_us'].append(row)
        print('forward', row, flush=True)

    B, N, C = 64, 256, 512
    qkv, dout = torch.randn(B, N, 3 * C, device=d), torch.randn(B, N, C, device=d)
    nb = int(lib.sr3_attention_bwd_scratch_bytes(B, N, C))
    scratch = torch.empty(nb, dtype=torch.uint8, device=d)
    dq = torch.empty(B, N, 3 * C, device=d)
    outs = {}
    for heads in (1, 8):
        outs[heads] = torch.empty(B, N, C, device=d)
        L.check(lib.sr3_attention_heads_f32(L.ptr(qkv), B, N, C, heads, L.ptr(outs[heads]), 1, G.stream()))
    bwd = lambda heads: (lambda: L.check(lib.sr3_attention_bwd_heads_f32(L.ptr(qkv), L.ptr(dout), L.ptr(outs[heads]), B, N, C, heads, L.ptr(dq),
                                                                          L.ptr(scratch), nb, G.stream())))
    t = alternate(torch, {'heads1': bwd(1), 'heads8': bwd(8)}, max(a.launches // 5, 5), a.rounds)
    row = dict(B=B, N=N, C=C, **{k: round(v, 2) for k, v in t.items()}, heads8_over_heads1=round(t['heads8'] / t['heads1'], 3))
    rec['backward_us'].append(row)
    print('backward', row, flush=True)
    del qkv, dout, scratch, dq, outs

    # ---- (3) C2 reverse step, batch 16 ----
    from wino_ragged_probe import step_ms
    nets = {}
    for key in ('absent', 'head_dim64'):
        torch.manual_seed(0)
        opt = bench.config_opt('sr3_16_128')
        if key != 'absent':
            opt['model']['unet']['head_dim'] = 64
        n = networks.define_G(opt).to(d)
        n.set_new_noise_schedule(opt['model']['beta_schedule']['val'], d)
        n.show_progress = False
        nets[key] = n
    best = {k: 1e30 for k in nets}
    for _ in range(a.rounds):
        for k, n in nets.items():
            best[k] = min(best[k], step_ms(n, 128, 128, 16, a.steps))
    rec['networks']['c2_reverse_step_ms_batch16'] = dict({k: round(v, 4) for k, v in best.items()},
                                                         head_dim64_over_absent=round(best['head_dim64'] / best['absent'], 4),
                                                         attention_heads={k: sorted(set((o['h_out'], o['cin']) for o in n.denoise_fn.plan.op_list(16) if o['kind'] == 60))
                                                                          for k, n in nets.items()})
    print('c2', rec['networks']['c2_reverse_step_ms_batch16'], flush=True)
    del nets

    # ---- (3) C3 training step, batch 64 ----
    models = {}
    S, Bt = 128, 64
    g = torch.Generator().manual_seed(77)
    data = {'HR': torch.rand(Bt, 3, S, S, generator=g) * 2 - 1, 'SR': torch.rand(Bt, 3, S, S, generator=g) * 2 - 1}
    for key in ('absent', 'head_dim64'):
        torch.manual_seed(1000)
        np.random.seed(1234)
        opt = bench.config_opt('sr3_16_128', phase='train')
        if key != 'absent':
            opt['model']['unet']['head_dim'] = 64
        m = Model.create_model(opt)
        m.feed_data(data)
        models[key] = m
    t = alternate(torch, {k: m.optimize_parameters for k, m in models.items()}, a.train_steps, a.rounds)
    rec['networks']['c3_train_step_ms_batch64'] = dict({k: round(v / 1e3, 3) for k, v in t.items()},
                                                       head_dim64_over_absent=round(t['head_dim64'] / t['absent'], 4))
    print('c3', rec['networks']['c3_train_step_ms_batch64'], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
