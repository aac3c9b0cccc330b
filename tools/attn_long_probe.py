#!/usr/bin/env python3
"""The key-blocked attention kernel (csrc/attention_long.hip; mode bit 1 of sr3_attention_ex_f32, plan option attn_long) next to the
score-strip kernels, and what attention costs in a reverse step at image sizes beyond the strip.  Two tables, GPU only:

  (1) us per launch (HIP events, best of 3 x 30 launches after a warm-up, one process) and achieved TFLOP/s of 4 B N^2 C: strip
      (mode 1) against key-blocked (mode 3) where both run, key-blocked alone beyond the strip; the yardstick is the strip kernel
      at N = 1024 of the same run (time per FLOP);
  (2) ms per graph-replayed reverse step with the headline SR3 16 -> 128 weights at 128 x 128 and beyond the strip, next to the
      pixel-proportional cost of the 128 x 128 step of the same run, with the attention ops' share of the forward
      (sr3_unet_forward_profile).

    python tools/attn_long_probe.py [--launches 30] [--steps 30] > profiles/attn_long_probe.txt"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd')
# B, N, C, modes
OPS = [(16, 256, 512, (1, 3)), (4, 1024, 512, (1, 3)), (4, 2304, 512, (3,)), (4, 4096, 512, (3,)), (1, 9216, 128, (3,)),
       (1, 2304, 512, (3,)), (2, 2304, 512, (3,)), (1, 4096, 512, (3,))]
STEPS = [(128, 128, 16), (256, 256, 4), (384, 384, 2), (512, 512, 1)]      # H, W, batch


def op_us(lib, L, G, torch, B, N, C, mode, launches):
    d = G.dev()
    qkv = torch.randn(B, N, 3 * C, device=d)
    out = torch.empty(B, N, C, device=d)
    call = lambda: L.check(lib.sr3_attention_ex_f32(L.ptr(qkv), B, N, C, L.ptr(out), mode, G.stream()))
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            call()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / launches)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, PKG)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import torch
    import bench
    import gpu_util as G
    import model.networks as networks
    from sr3_hip import lib as L
    from wino_ragged_probe import profile, step_ms
    lib = L.load()
    print('# (1) us per launch, best of 3 x %d launches; TF = 4 B N^2 C / time' % a.launches)
    print('# %-16s %22s %22s  %s' % ('B, N, C', 'strip (mode 1) us (TF)', 'key-blocked (mode 3)', 'key-blocked time per FLOP / strip at (4, 1024, 512)'))
    yard = None
    for B, N, C, modes in OPS:
        fl = 4.0 * B * N * N * C
        t = {m: op_us(lib, L, G, torch, B, N, C, m, a.launches) for m in modes}
        if (B, N, C) == (4, 1024, 512):
            yard = t[1] / fl
        cell = lambda m: '%10.1f (%6.1f)' % (t[m], fl / t[m] * 1e-6) if m in t else '%19s' % '-'
        print('  %-16s %22s %22s  %s' % ('%d, %d, %d' % (B, N, C), cell(1), cell(3), '%.2f' % (t[3] / fl / yard) if yard else '-'), flush=True)
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    opt = bench.config_opt('sr3_16_128')
    netG = networks.define_G(opt).to(dev)
    netG.set_new_noise_schedule(opt['model']['beta_schedule']['val'], dev)
    netG.show_progress = False
    netG.denoise_fn.plan.set_option('attn_long', 1)
    print('# (2) ms per graph-replayed reverse step (best of 3 x %d steps), plan option attn_long = 1; attention share: kind-60 ops of one' % a.steps)
    print('#     profiled forward (mean of %d)' % a.reps)
    print('# %-9s %3s  %9s  %28s  %s' % ('geometry', 'B', 'step ms', 'step / pixel-proportional', 'attention ops: ms of the forward (share), kernels'))
    base = None
    for H, W, B in STEPS:
        ms = step_ms(netG, H, W, B, a.steps)
        rows, tot = profile(netG, H, W, B, a.reps)
        att = [(o, t) for o, t in rows if o['kind'] == 60]
        # (profile() adds the launches behind an op up to the next contraction to it: for attention that is nothing -- the 1x1 out conv follows)
        att_ms = sum(t for _, t in att)
        if base is None:
            base = dict(ms=ms, px=H * W * B)
        prop = base['ms'] * (H * W * B) / base['px']
        kern = ', '.join('%d x N=%d %s' % (sum(1 for o, _ in att if (o['h_out'], o['tile_cfg']) == k), k[0], 'key-blocked' if k[1] == 24 else 'strip')
                         for k in sorted(set((o['h_out'], o['tile_cfg']) for o, _ in att)))
        print('  %3dx%-5d %3d  %9.3f  %10.2f (%8.3f ms)      %8.3f of %8.3f ms (%4.1f %%), %s' % (H, W, B, ms, ms / prop, prop, att_ms, tot, 100 * att_ms / tot, kern),
              flush=True)


if __name__ == '__main__':
    main()
