#!/usr/bin/env python3
"""The ragged two-workgroup Winograd tile (csrc/conv3x3_wino2.hip, ABI tile 23) against the kernels its layers fall back to, at
image sizes other than the config's image_size, on the headline SR3 16 -> 128 network.  Two tables, GPU only:

  (1) per ragged layer shape, INSIDE the forward (HIP events around every launch, sr3_unet_forward_profile; operands as cold as a
      forward leaves them): time of the conv and of everything it drags along up to the next contraction -- its split-K reduce,
      the stand-alone statistics pass, the GroupNorm fold -- with plan option wino_ragged = 1 and = 0;
  (2) ms per graph-replayed reverse step at 128 x 128 (the headline) and at every other geometry, both settings, and how far
      each is from the pixel-proportional cost of the 128 x 128 step of the same run.

    python tools/wino_ragged_probe.py [--reps 5] [--steps 30] > profiles/wino_ragged_probe.txt"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd')
GEOMETRIES = [(128, 128, 16), (128, 192, 16), (176, 128, 16), (256, 256, 4), (64, 64, 16)]      # H, W, batch


def profile(netG, H, W, B, reps):
    """[(op dict, ms of the op and of the launches behind it up to the next contraction)] for every conv / attention op."""
    import torch
    from sr3_hip import lib as L
    un = netG.denoise_fn
    plan, lib, dev = un.plan, L.load(), un.arena.device
    plan.set_geometry(H, W)
    un.ensure_derived()
    x = torch.randn(B, 3, H, W, device=dev)
    cond = torch.rand(B, 3, H, W, device=dev) * 2 - 1
    level = torch.full((B,), 0.5, device=dev)
    wsbuf, need = un._ws.get(plan, B, dev)
    out = torch.empty(B, 3, H, W, device=dev)
    max_ops = 4096
    ms, kind, fl, n = (C.c_float * max_ops)(), (C.c_int * max_ops)(), (C.c_double * max_ops)(), C.c_int()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    acc = None
    for r in range(reps + 1):
        L.check(lib.sr3_unet_forward_profile(plan.handle, L.ptr(x), L.ptr(cond), 3, L.ptr(level), None, L.ptr(un.freq),
                                             L.ptr(un.arena.data), L.ptr(wsbuf), need, L.ptr(out), B, stream, max_ops, ms, kind, fl,
                                             C.byref(n)))
        if r == 0:
            continue
        acc = acc or [0.0] * n.value
        for i in range(n.value):
            acc[i] += ms[i] / reps
    ops = plan.op_list(B)
    rows, j = [], -1
    for i in range(n.value):
        if int(kind[i]) != 59:
            j += 1
        o = ops[j]
        if int(kind[i]) != 59 and o['kind'] in (20, 50, 60, 70):
            rows.append([o, 0.0])
        if rows:
            rows[-1][1] += acc[i]
    return rows, sum(acc)


def step_ms(netG, H, W, B, steps):
    import torch
    dev = netG.denoise_fn.arena.device
    shape = (B, 3, H, W)
    netG.denoise_fn.plan.set_geometry(H, W)
    st = netG._loop_state(shape, shape, dev)
    netG.denoise_fn.ensure_derived()
    if st['graph'] is None:
        netG._capture(st)
    st['img'].normal_()
    st['cond'].uniform_(-1, 1)
    best = 1e9
    for _ in range(3):
        st['step'].fill_(netG.num_timesteps - 1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st['graph'].replay()
        e0.record()
        for _ in range(steps):
            st['graph'].replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / steps)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=30)
    a = ap.parse_args()
    sys.path.insert(0, PKG)
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import model.networks as networks
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    opt = bench.config_opt('sr3_16_128')
    netG = networks.define_G(opt).to(dev)
    netG.set_new_noise_schedule(opt['model']['beta_schedule']['val'], dev)
    netG.show_progress = False
    plan = netG.denoise_fn.plan
    print('# (1) per ragged layer shape inside the forward: conv + reduce + statistics + fold, us per launch group (mean of %d forwards)' % a.reps)
    print('# %-9s %3s  %-34s %5s  %12s %12s  %6s  %s' % ('geometry', 'B', 'layer', 'count', 'ragged us', 'fallback us', 'ratio', 'fallback tile'))
    for H, W, B in GEOMETRIES[1:]:
        plan.set_option('wino_ragged', 1)
        on, tot_on = profile(netG, H, W, B, a.reps)
        plan.set_option('wino_ragged', 0)
        off, tot_off = profile(netG, H, W, B, a.reps)
        plan.set_option('wino_ragged', 1)
        table = {}
        assert len(on) == len(off)
        for (o1, t1), (o0, t0) in zip(on, off):
            if o1['kind'] == 50 and o1['tile_cfg'] == 23:
                key = (o1['h_out'], o1['w_out'], o1['cin'], o1['cout'], o1['upsample'])
                e = table.setdefault(key, [0, 0.0, 0.0, set(), set()])
                e[0] += 1; e[1] += t1; e[2] += t0
                e[3].add('t%d ks%d' % (o0['tile_cfg'], o0['ksplit'])); e[4].add('ks%d' % o1['ksplit'])
        for key, e in sorted(table.items(), reverse=True):
            label = '3x3%s %4d->%4d @%3dx%-3d %s' % (' up' if key[4] else '   ', key[2], key[3], key[0], key[1], ','.join(sorted(e[4])))
            print('  %3dx%-5d %3d  %-34s %5d  %12.1f %12.1f  %6.2f  %s' % (H, W, B, label, e[0], e[1] / e[0] * 1e3, e[2] / e[0] * 1e3,
                                                                      e[1] / e[2], ','.join(sorted(e[3]))))
        print('# %dx%d batch %d: all launches of one forward summed: ragged %.3f ms, fallback %.3f ms' % (H, W, B, tot_on, tot_off))
    print('# (2) ms per graph-replayed reverse step (best of 3 x %d steps)' % a.steps)
    print('# %-9s %3s  %10s %12s  %22s' % ('geometry', 'B', 'ragged ms', 'fallback ms', 'ragged / pixel-proportional'))
    base = {}
    for H, W, B in GEOMETRIES:
        plan.set_option('wino_ragged', 1)
        t1 = step_ms(netG, H, W, B, a.steps)
        plan.set_option('wino_ragged', 0)
        t0 = step_ms(netG, H, W, B, a.steps)
        if (H, W) == (128, 128):
            base = dict(ms=t1, px=H * W * B)
        prop = base['ms'] * (H * W * B) / base['px']
        print('  %3dx%-5d %3d  %10.3f %12.3f  %10.2f (%.3f ms)' % (H, W, B, t1, t0, t1 / prop, prop))
    plan.set_option('wino_ragged', 1)


if __name__ == '__main__':
    main()
