#!/usr/bin/env python3
"""What the passes between the training step and Adam cost (config train.optimizer.accumulate / clip_grad_norm): on an arena of the
BASELINE config's size, through the C ABI, timed with HIP events -- the global norm (sr3_grad_norm), the accumulate without and with
the fused norm (sr3_grad_accumulate), the scaled Adam+EMA (sr3_adam_ema_step_scaled, mode 2), the unscaled sr3_adam_ema_step and the plain
sr3_adam_step on the same buffers -- legs interleaved --rounds times after --warmup calls each; median and p10-p90 per leg, GB/s = the bytes the
algorithm needs over the median.
    python tools/optim_probe.py [--config sr3_16_128] [--rounds 40] [--warmup 5]      (GPU box)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='sr3_16_128')
    ap.add_argument('--rounds', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, PKG)
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import model.networks as networks
    from sr3_hip import lib as L
    assert torch.cuda.is_available(), 'optim_probe needs a GPU'
    dev = torch.device('cuda', 0)
    n = networks.define_G(bench.config_opt(a.config)).denoise_fn.plan.param_floats
    lib = L.load()
    gen = torch.Generator(device=dev).manual_seed(0)
    p, ema = (torch.randn(n, device=dev, generator=gen) for _ in range(2))
    g, acc, m = (torch.randn(n, device=dev, generator=gen) * 0.1 for _ in range(3))
    v = torch.rand(n, device=dev, generator=gen) * 0.01
    nb = int(lib.sr3_grad_norm_scratch_bytes(n))
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    out4 = torch.zeros(4, device=dev)
    one4 = torch.tensor([1.0, 1.0, 1.0, 0.0], device=dev)       # coef 1, flag set: the scaled kernel does the unscaled one's work
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = C.c_float
    adam = [L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(ema), n, f(1e-4), f(0.9), f(0.999), f(1e-8), 7, f(0.9999), 2]
    legs = {       # name -> (bytes per element, call)
        'grad_norm': (4, lambda: lib.sr3_grad_norm(L.ptr(g), n, f(1.0), L.ptr(scratch), nb, L.ptr(out4), st)),
        'accumulate': (12, lambda: lib.sr3_grad_accumulate(L.ptr(acc), L.ptr(g), n, 0, f(1.0), None, 0, None, st)),
        'accumulate_fused_norm': (12, lambda: lib.sr3_grad_accumulate(L.ptr(acc), L.ptr(g), n, 0, f(1.0), L.ptr(scratch), nb, L.ptr(out4), st)),
        'adam_ema_scaled_mode2': (36, lambda: lib.sr3_adam_ema_step_scaled(*adam, L.ptr(one4), st)),
        'adam_ema_mode2': (36, lambda: lib.sr3_adam_ema_step(*adam, st)),
        'adam': (28, lambda: lib.sr3_adam_step(*adam[:4], *adam[5:11], st)),
    }
    ms = {k: [] for k in legs}
    for rnd in range(a.warmup + a.rounds):
        if rnd % 8 == 0:
            acc.copy_(g)                                          # (the running sum stays finite over the rounds)
        for name, (_, call) in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            L.check(call())
            e1.record()
            torch.cuda.synchronize()
            if rnd >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
    assert bool(torch.isfinite(out4).all()) and bool(torch.isfinite(p).all())
    rec = {'what': 'optimizer passes', 'config': a.config, 'floats': n, 'rounds': a.rounds}
    for name, (bpe, _) in legs.items():
        t = sorted(ms[name])
        med = statistics.median(t)
        rec[name] = {'us_median': round(med * 1e3, 1), 'us_p10': round(t[len(t) // 10] * 1e3, 1), 'us_p90': round(t[(len(t) * 9) // 10] * 1e3, 1),
                     'bytes_per_element': bpe, 'GBps': round(bpe * n / (med * 1e-3) / 1e9)}
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
