#!/usr/bin/env python3
"""What the on-device degradation of an HR-only training batch costs: data.degrade.degrade_batch at batch 64,
128 x 128 -> 16 x 16 -> 128 x 128, 21 x 21 anisotropic blur and noise on for every sample -- timed with HIP events around the whole
call (weights made on the host, uploaded, four kernels' worth of work), --warmup calls, then --rounds timed ones; median and
p10-p90.  The blur kernel alone is timed the same way.  Next to it the same chain restated with NumPy + Pillow (the 441-tap
shifted accumulate of tests/test_degrade_cpu.py, Image.resize, fp32 noise) over --threads CPU threads, wall clock.  The JPEG link
(data.degrade.jpeg_batch, 4:2:0, per-image qualities in 30..95) is timed on its own on an LR batch of 64 x 16 x 16 x 3 and on one of
16 x 128 x 128 x 3, next to the Pillow save / open loop over the same threads, with the byte equality of the two.
    python tools/degrade_probe.py [--batch 64] [--rounds 30] [--warmup 5] [--threads 16] [--step-ms 123.8]      (GPU box)
--second [--mid 64] times the second-order chain of DESIGN.md 3.4c instead, next to the first-order one (second_order below)."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd')


def spread(ms):
    s = sorted(ms)
    return {'median_ms': round(statistics.median(s), 4), 'p10_ms': round(s[len(s) // 10], 4), 'p90_ms': round(s[(len(s) * 9) // 10], 4),
            'n': len(s)}


def second_order(a):
    """--second: the two-round chain at batch 64, 128 -> M = 64 -> 16 -> 128 with every stage on for every sample --
    a 21-tap blur (half the batch sinc) and noise in all four modes in both rounds, both JPEGs, the final sinc in both orders -- next
    to the first-order chain (blur, noise, JPEG) on the same crops, each timed as the whole degrade_batch call."""
    import numpy as np
    import torch
    import data.degrade as D
    assert torch.cuda.is_available(), 'degrade_probe needs a GPU'
    assert a.rounds >= 20, 'at least 20 timed repetitions'
    R, Lr, M, k, n = 128, 16, a.mid, 21, a.batch
    blur = {'kernel': k, 'sigma': [0.2, 3.0], 'anisotropic': True}
    one = {'blur': blur, 'noise': {'sigma': [1, 25]}, 'jpeg': {'quality': [30, 95]}}
    two = dict(one, sinc={'prob': 0.5}, shot={'prob': 0.5}, gray_noise=0.5,
               second=dict(one, mid=[M, M], resample=['box', 'bilinear', 'bicubic'], sinc={'prob': 0.5}, shot={'prob': 0.5}, gray_noise=0.5,
                           final_sinc={'kernel': 7}))
    cfg1, cfg2 = D.degrade_config(one, Lr), D.degrade_config(two, Lr)
    torch.manual_seed(0)
    dev = torch.device('cuda', 0)
    hr = torch.from_numpy(np.random.RandomState(0).randint(0, 256, size=(n, R, R, 3)).astype(np.uint8)).to(dev)
    deg = torch.stack([D.draw_deg(cfg2) for _ in range(n)])
    deg2 = torch.stack([D.draw_deg2(cfg2) for _ in range(n)])
    assert bool((deg[:, 0] == 1).all() and (deg[:, 4] > 0).all() and (deg[:, 5] > 0).all())
    assert bool((deg2[:, 7] == 1).all() and (deg2[:, 13] > 0).all() and (deg2[:, 16] > 0).all() and (deg2[:, 17] == 1).all())
    g = torch.Generator(device=dev).manual_seed(1)
    z, z2 = torch.randn(n, M, M, 3, device=dev, generator=g), torch.randn(n, Lr, Lr, 3, device=dev, generator=g)
    r = torch.randint(0, 2 ** 31 - 1, (n, M, M, 3), dtype=torch.int32, device=dev, generator=g)
    r2 = torch.randint(0, 2 ** 31 - 1, (n, Lr, Lr, 3), dtype=torch.int32, device=dev, generator=g)

    def timed(call):
        ms = []
        for rnd in range(a.warmup + a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if rnd >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return spread(ms)

    t2 = timed(lambda: D.degrade_batch(hr, deg, cfg2, z=z, deg2=deg2, r=r, z2=z2, r2=r2))
    t2_drawn = timed(lambda: D.degrade_batch(hr, deg, cfg2, deg2=deg2))                 # the loader's call: the noise drawn inside
    t1 = timed(lambda: D.degrade_batch(hr, deg, cfg1, z=z2))
    a1, b1 = D.degrade_batch(hr, deg, cfg2, z=z, deg2=deg2, r=r, z2=z2, r2=r2)
    a2, b2 = D.degrade_batch(hr, deg, cfg2, z=z, deg2=deg2, r=r, z2=z2, r2=r2)
    out = {'probe': 'degrade_batch_second', 'device': torch.cuda.get_device_name(0), 'batch': n, 'r_resolution': R, 'mid': M, 'l_resolution': Lr,
           'kernel': k, 'modes_round1': sorted(set(deg2[:, 2].tolist())), 'modes_round2': sorted(set(deg2[:, 14].tolist())),
           'final_orders': sorted(set(deg2[:, 19].tolist())), 'gpu_second_order': t2, 'gpu_second_order_drawing_noise': t2_drawn,
           'gpu_first_order': t1, 'repeatable': bool(torch.equal(a1, a2) and torch.equal(b1, b2)), 'step_ms': a.step_ms,
           'second_share_of_step': round(t2_drawn['median_ms'] / a.step_ms, 5), 'first_share_of_step': round(t1['median_ms'] / a.step_ms, 5)}
    print(json.dumps(out))
    assert out['repeatable'], 'two calls with the same draws differ'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--second', action='store_true', help='time the second-order chain (and the first-order one beside it) instead')
    ap.add_argument('--mid', type=int, default=64, help='--second: the intermediate size M')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--cpu-rounds', type=int, default=5)
    ap.add_argument('--step-ms', type=float, default=123.8, help='the training step the cost is compared with (BASELINE config, batch 64)')
    a = ap.parse_args()
    sys.path.insert(0, PKG)
    sys.path.insert(0, ROOT)
    if a.second:
        return second_order(a)
    import numpy as np
    import torch
    from PIL import Image
    import data.degrade as D
    assert torch.cuda.is_available(), 'degrade_probe needs a GPU'
    assert a.rounds >= 20, 'at least 20 timed repetitions'
    R, Lr, k, n = 128, 16, 21, a.batch
    cfg = D.degrade_config({'blur': {'kernel': k, 'sigma': [0.2, 3.0], 'anisotropic': True}, 'noise': {'sigma': [1, 25]}}, Lr)
    torch.manual_seed(0)
    rng = np.random.RandomState(0)
    hr = rng.randint(0, 256, size=(n, R, R, 3)).astype(np.uint8)
    deg = torch.stack([D.draw_deg(cfg) for _ in range(n)])
    assert bool((deg[:, 0] == 1).all()) and bool((deg[:, 4] > 0).all())
    z = torch.randn(n, Lr, Lr, 3, generator=torch.Generator().manual_seed(1))
    dev = torch.device('cuda', 0)
    hr_d, z_d = torch.from_numpy(hr).to(dev), z.to(dev)
    w_d = torch.from_numpy(np.stack([D.blur_weights(r[1], r[2], r[3], k) for r in deg.double().numpy()])).to(dev)

    def timed(call):
        ms = []
        for rnd in range(a.warmup + a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if rnd >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return spread(ms)

    gpu = timed(lambda: D.degrade_batch(hr_d, deg, cfg, z=z_d))
    blur = timed(lambda: D.blur_batch(hr_d, w_d))
    lr_d, sr_d = D.degrade_batch(hr_d, deg, cfg, z=z_d)

    # the same chain on the CPU: NumPy blur (int64 shifted accumulate) -> Pillow -> NumPy fp32 noise -> Pillow, one image per task
    d64, zn = deg.double().numpy(), z.numpy()

    def one(i):
        w = D.blur_weights(d64[i][1], d64[i][2], d64[i][3], k)
        r = k // 2
        p = np.pad(hr[i].astype(np.int64), ((r, r), (r, r), (0, 0)), mode='reflect')
        acc = np.zeros(hr[i].shape, dtype=np.int64)
        for dy in range(k):
            for dx in range(k):
                acc += int(w[dy, dx]) * p[dy:dy + R, dx:dx + R]
        x = np.clip((acc + 32768) >> 16, 0, 255).astype(np.uint8)
        lr = np.asarray(Image.fromarray(x).resize((Lr, Lr), Image.BICUBIC))
        v = lr.astype(np.float32) + np.float32(d64[i][4]) * zn[i]
        lr = np.clip(np.rint(v), 0, 255).astype(np.uint8)
        return lr, np.asarray(Image.fromarray(lr).resize((R, R), Image.BICUBIC))

    cpu_ms = []
    with ThreadPoolExecutor(a.threads) as pool:
        for rnd in range(1 + a.cpu_rounds):
            t0 = time.perf_counter()
            ref = list(pool.map(one, range(n)))
            if rnd:
                cpu_ms.append((time.perf_counter() - t0) * 1e3)
    same = all(np.array_equal(lr_d[i].cpu().numpy(), ref[i][0]) and np.array_equal(sr_d[i].cpu().numpy(), ref[i][1]) for i in range(n))
    cpu = spread(cpu_ms)

    # the JPEG link alone: sr3_jpeg_u8 (4:2:0, qualities 30..95 drawn per image) against the Pillow loop it stands for -- save to a
    # buffer, open, one image per task over the same threads -- on an LR batch of the training geometry and on a larger one
    import io

    def pil_jpeg(img, q):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, 'JPEG', quality=int(q), subsampling=2)
        return np.asarray(Image.open(io.BytesIO(buf.getvalue())))

    jpeg = []
    with ThreadPoolExecutor(a.threads) as pool:
        for nj, side in ((64, 16), (16, 128)):
            imgs = rng.randint(0, 256, size=(nj, side, side, 3)).astype(np.uint8)
            imgs[:, :side // 2] = imgs[:, :side // 2] // 64 * 64          # (flat-ish halves: not every block is noise)
            qs = rng.randint(30, 96, size=nj).astype(np.int32)
            imgs_d, qs_d = torch.from_numpy(imgs).to(dev), torch.from_numpy(qs).to(dev)
            got = D.jpeg_batch(imgs_d, qs_d, '4:2:0').cpu().numpy()
            t_gpu = timed(lambda: D.jpeg_batch(imgs_d, qs_d, '4:2:0'))
            ms = []
            for rnd in range(1 + a.cpu_rounds):
                t0 = time.perf_counter()
                ref_j = list(pool.map(pil_jpeg, imgs, qs))
                if rnd:
                    ms.append((time.perf_counter() - t0) * 1e3)
            jpeg.append({'batch': nj, 'side': side, 'gpu_jpeg_batch': t_gpu, 'cpu_pillow_loop': dict(spread(ms), threads=a.threads),
                         'device_equals_pillow': bool(np.array_equal(got, np.stack(ref_j)))})
    from PIL import features
    turbo = bool(features.check_feature('libjpeg_turbo'))
    out = {'probe': 'degrade_batch', 'jpeg': jpeg, 'pillow_on_libjpeg_turbo': turbo, 'device': torch.cuda.get_device_name(0), 'batch': n, 'r_resolution': R, 'l_resolution': Lr, 'kernel': k,
           'gpu_degrade_batch': gpu, 'gpu_blur_only': blur, 'cpu_numpy_pillow': dict(cpu, threads=a.threads),
           'device_equals_cpu_chain': bool(same), 'step_ms': a.step_ms,
           'gpu_share_of_step': round(gpu['median_ms'] / a.step_ms, 5), 'cpu_share_of_step': round(cpu['median_ms'] / a.step_ms, 3)}
    print(json.dumps(out))
    assert same, 'the device chain and the NumPy + Pillow chain differ'
    # (a Pillow on another libjpeg may round differently: the report says so, the committed fixture of tests/golden is the gate)
    assert not turbo or all(j['device_equals_pillow'] for j in jpeg), 'sr3_jpeg_u8 and the Pillow round trip differ'


if __name__ == '__main__':
    main()
