"""The degradation between an HR crop and its conditioning images, on the MI355X (engine extension: the reference only reads
triplets data/prepare_data.py made with one fixed bicubic kernel):

    HR (n, R, R, C) --blur--> resize to (L, L) --noise--> --jpeg--> LR --resize to (R, R)--> SR

Blur (csrc/degrade.hip: sr3_blur_u8) is a per-image Gaussian in 16-bit fixed point, noise (sr3_noise_u8) is additive Gaussian in
8-bit levels on the LR image, JPEG (sr3_jpeg_u8) is the lossy half of Pillow's save / open round trip at a per-image quality (libjpeg's
integer arithmetic, bit for bit), both resizes are data.prepare_data.resize_batch (Pillow bit for bit).  With blur off, noise 0 and
no JPEG the pair is byte-identical to what prepare_data.py writes for the crop.  The per-image draws `deg` = [blur_on, sigma_x,
sigma_y, theta, noise_sigma (, jpeg_quality)] come from the dataset (data/HR_dataset.py); this module holds the config's one
validation, the kernel weights and the device chain."""
import ctypes as C

import numpy as np
import torch
from PIL import Image

from sr3_hip import lib as L

MAX_KERNEL = 21
ONE = 1 << 16                     # fixed-point 1.0 of the blur weights
_RESAMPLE = {'bicubic': Image.BICUBIC, 'bilinear': Image.BILINEAR}
_KEYS = {None: ('blur', 'noise', 'jpeg', 'resample', 'seed'), 'blur': ('prob', 'kernel', 'sigma', 'anisotropic'), 'noise': ('prob', 'sigma'),
         'jpeg': ('prob', 'quality', 'subsampling')}
_SUBSAMPLING = {'4:4:4': 0, '4:2:0': 2}           # Pillow's numbers, the ABI's


def _known(block, name):
    if not isinstance(block, dict):
        raise ValueError('degrade%s: a dict of settings expected, got %r' % ('.' + name if name else '', block))
    for key in block:
        if key not in _KEYS[name]:
            raise ValueError('degrade: unknown key "%s%s" (known: %s)' % (name + '.' if name else '', key, ', '.join(_KEYS[name])))


def _prob(block, name):
    p = block.get('prob', 1.0)           # a block that is present is on unless it says otherwise
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:
        raise ValueError('degrade: %s.prob %r is not a probability in [0, 1]' % (name, p))
    return float(p)


def _range(block, name, default, lo_open):
    s = block.get('sigma', default)
    if not isinstance(s, (list, tuple)) or len(s) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, float)) for v in s):
        raise ValueError('degrade: %s.sigma %r is not a [lo, hi] pair of numbers' % (name, s))
    lo, hi = float(s[0]), float(s[1])
    if not ((0.0 < lo if lo_open else 0.0 <= lo) and lo <= hi and hi < float('inf')):
        raise ValueError('degrade: %s.sigma %r needs %s lo <= hi' % (name, s, '0 <' if lo_open else '0 <='))
    return lo, hi


def _quality(block):
    q = block.get('quality', (30, 95))
    if not isinstance(q, (list, tuple)) or len(q) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in q):
        raise ValueError('degrade: jpeg.quality %r is not a [lo, hi] pair of integers' % (q,))
    if not 1 <= q[0] <= q[1] <= 100:
        raise ValueError('degrade: jpeg.quality %r needs 1 <= lo <= hi <= 100' % (q,))
    return int(q[0]), int(q[1])


def degrade_config(cfg, l_resolution):
    """The one validation of a dataset block's "degrade" value (every key optional; {} = plain bicubic):
        {"blur": {"prob": p, "kernel": k, "sigma": [lo, hi], "anisotropic": bool}, "noise": {"prob": p, "sigma": [lo, hi]},
         "jpeg": {"prob": p, "quality": [lo, hi], "subsampling": "4:2:0" | "4:4:4"}, "resample": "bicubic" | "bilinear", "seed": 0}
    -> the normalised dict degrade_batch and the datasets read (every key present, plus 'l_resolution'; 'jpeg' also says whether the
    key was 'given': draw_deg's result has a sixth number only then).  ValueError names what it refuses: an unknown key, an even
    kernel or one outside 1..21, blur sigmas without 0 < lo <= hi, noise sigmas without 0 <= lo <= hi, JPEG qualities that are not
    integers with 1 <= lo <= hi <= 100, an unknown subsampling, a probability outside [0, 1], an unknown resample, a seed that is
    not an integer."""
    cfg = {} if cfg is None else cfg
    _known(cfg, None)
    blur, noise = cfg.get('blur', {'prob': 0.0}), cfg.get('noise', {'prob': 0.0})
    _known(blur, 'blur')
    _known(noise, 'noise')
    jpeg = cfg['jpeg'] if 'jpeg' in cfg else {'prob': 0.0}
    _known(jpeg, 'jpeg')
    sub = jpeg.get('subsampling', '4:2:0')
    if not isinstance(sub, str) or sub not in _SUBSAMPLING:
        raise ValueError('degrade: jpeg.subsampling %r is not "4:2:0" or "4:4:4"' % (sub,))
    k = blur.get('kernel', MAX_KERNEL)
    if isinstance(k, bool) or not isinstance(k, int) or k < 1 or k > MAX_KERNEL or k % 2 == 0:
        raise ValueError('degrade: blur.kernel %r is not an odd integer in 1..%d' % (k, MAX_KERNEL))
    aniso = blur.get('anisotropic', False)
    if not isinstance(aniso, bool):
        raise ValueError('degrade: blur.anisotropic %r is not a bool' % (aniso,))
    resample = cfg.get('resample', 'bicubic')
    if resample not in _RESAMPLE:
        raise ValueError('degrade: resample %r is not "bicubic" or "bilinear"' % (resample,))
    seed = cfg.get('seed', 0)
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError('degrade: seed %r is not an integer' % (seed,))
    if isinstance(l_resolution, bool) or not isinstance(l_resolution, int) or l_resolution < 1:
        raise ValueError('degrade: l_resolution %r is not a positive integer' % (l_resolution,))
    return {'blur': {'prob': _prob(blur, 'blur'), 'kernel': k, 'sigma': _range(blur, 'blur', (0.2, 3.0), True), 'anisotropic': aniso},
            'noise': {'prob': _prob(noise, 'noise'), 'sigma': _range(noise, 'noise', (0.0, 0.0), False)},
            'jpeg': {'prob': _prob(jpeg, 'jpeg'), 'quality': _quality(jpeg), 'subsampling': sub, 'given': 'jpeg' in cfg},
            'resample': resample, 'seed': seed, 'l_resolution': l_resolution}


def draw_deg(cfg, generator=None):
    """One sample's numbers [blur_on, sigma_x, sigma_y, theta, noise_sigma] (fp32 tensor) from torch's global generator, or from
    `generator` (the validation split's per-index one); a config with a "jpeg" key adds a sixth, the JPEG quality (0 = off).
    Always seven uniform draws, whatever is switched on, so the stream a sample consumes does not depend on the outcome -- nor the
    first five numbers on the "jpeg" key.  Isotropic blur: sigma_y = sigma_x, theta = 0.  JPEG: one draw decides both, on when
    u < prob and then u / prob, uniform in [0, 1), picks the quality uniformly from lo..hi."""
    u = torch.rand(7, generator=generator).tolist()
    b, n, j = cfg['blur'], cfg['noise'], cfg['jpeg']
    blur_on, noise_on = u[0] < b['prob'], u[4] < n['prob']
    sx = b['sigma'][0] + (b['sigma'][1] - b['sigma'][0]) * u[1]
    sy = b['sigma'][0] + (b['sigma'][1] - b['sigma'][0]) * u[2] if b['anisotropic'] else sx
    theta = np.pi * u[3] if b['anisotropic'] else 0.0
    ns = n['sigma'][0] + (n['sigma'][1] - n['sigma'][0]) * u[5] if noise_on else 0.0
    deg = [1.0 if blur_on else 0.0, sx, sy, theta, ns]
    if j['given']:
        lo, hi = j['quality']
        deg.append(float(min(hi, lo + int((u[6] / j['prob']) * (hi - lo + 1)))) if u[6] < j['prob'] else 0.0)
    return torch.tensor(deg, dtype=torch.float32)


def blur_weights(sigma_x, sigma_y, theta, k, on=True):
    """(k, k) int32 Gaussian in 16-bit fixed point, in NumPy float64: w = exp(-(u^2 / sx^2 + v^2 / sy^2) / 2) with (u, v) the tap
    offset rotated by theta, normalised to sum 1, q = floor(w * 65536 + 0.5), and the centre tap takes 65536 - q.sum() so the sum
    is exactly 65536.  on=False: the delta.  sigma_x == sigma_y is a circle: theta is not applied (the same bits for every theta)."""
    k = int(k)
    if k < 1 or k > MAX_KERNEL or k % 2 == 0:
        raise ValueError('blur_weights: k %r is not an odd integer in 1..%d' % (k, MAX_KERNEL))
    q = np.zeros((k, k), dtype=np.int64)
    if not on:
        q[k // 2, k // 2] = ONE
        return q.astype(np.int32)
    sx, sy = float(sigma_x), float(sigma_y)
    if not (sx > 0.0 and sy > 0.0):
        raise ValueError('blur_weights: sigmas must be positive, got (%r, %r)' % (sigma_x, sigma_y))
    t = 0.0 if sx == sy else float(theta)
    dy, dx = np.mgrid[0:k, 0:k].astype(np.float64) - (k // 2)
    u = np.cos(t) * dx + np.sin(t) * dy
    v = -np.sin(t) * dx + np.cos(t) * dy
    w = np.exp(-0.5 * ((u * u) / (sx * sx) + (v * v) / (sy * sy)))
    w = w / w.sum()
    q = np.floor(w * ONE + 0.5).astype(np.int64)
    q[k // 2, k // 2] += ONE - q.sum()
    return q.astype(np.int32)


def _device(t):
    if t.is_cuda:
        return t.device
    if not torch.cuda.is_available():
        raise L.Sr3Error('data.degrade runs on the MI355X engine: no GPU visible and there is no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())


def blur_batch(batch_u8, weights_i32):
    """(n, H, W, C) uint8, (n, k, k) int32 (both on the device) -> the blurred batch: sr3_blur_u8."""
    n, H, W, Cc = batch_u8.shape
    k = int(weights_i32.shape[-1])
    if not (batch_u8.is_cuda and batch_u8.dtype == torch.uint8 and batch_u8.is_contiguous()):
        raise TypeError('blur_batch: a contiguous uint8 batch on the device expected')
    if not (weights_i32.device == batch_u8.device and weights_i32.dtype == torch.int32 and weights_i32.is_contiguous()
            and tuple(weights_i32.shape) == (n, k, k)):
        raise TypeError('blur_batch: weights must be a contiguous (%d, k, k) int32 tensor on the batch\'s device' % n)
    out = torch.empty_like(batch_u8)
    L.check(L.load().sr3_blur_u8(L.ptr(batch_u8), n, H, W, Cc, L.ptr(weights_i32), k, L.ptr(out),
                                 C.c_void_p(torch.cuda.current_stream(batch_u8.device).cuda_stream)))
    return out


def noise_batch(batch_u8, sigma_f32, z_f32, out=None):
    """out = clamp(rint(batch + sigma_i * z)) (uint8; out may be `batch_u8` itself): sr3_noise_u8."""
    n = batch_u8.shape[0]
    if out is None:
        out = torch.empty_like(batch_u8)
    dev = batch_u8.device
    for t, dt, shape in ((batch_u8, torch.uint8, None), (out, torch.uint8, batch_u8.shape), (z_f32, torch.float32, batch_u8.shape),
                         (sigma_f32, torch.float32, (n,))):
        if not (t.is_cuda and t.device == dev and t.dtype == dt and t.is_contiguous() and (shape is None or tuple(t.shape) == tuple(shape))):
            raise TypeError('noise_batch: contiguous device tensors expected -- uint8 batch / out, fp32 z of the batch\'s shape, fp32 sigma (n)')
    L.check(L.load().sr3_noise_u8(L.ptr(batch_u8), n, batch_u8[0].numel(), L.ptr(sigma_f32), L.ptr(z_f32), L.ptr(out),
                                  C.c_void_p(torch.cuda.current_stream(batch_u8.device).cuda_stream)))
    return out


def jpeg_batch(batch_u8, quality_i32, subsampling='4:2:0', out=None):
    """The JPEG round trip of an (n, H, W, C) uint8 batch at per-image qualities (n) int32, both on the device (a quality <= 0 leaves
    its image as it is; out may be `batch_u8` itself): sr3_jpeg_u8, Pillow's save / open bytes."""
    if subsampling not in _SUBSAMPLING:
        raise ValueError('jpeg_batch: subsampling %r is not "4:2:0" or "4:4:4"' % (subsampling,))
    if not (torch.is_tensor(batch_u8) and batch_u8.is_cuda and batch_u8.dtype == torch.uint8 and batch_u8.dim() == 4 and batch_u8.is_contiguous()):
        raise TypeError('jpeg_batch: a contiguous (n, H, W, C) uint8 batch on the device expected (there is no CPU fallback)')
    n, H, W, Cc = batch_u8.shape
    if out is None:
        out = torch.empty_like(batch_u8)
    if not (out.device == batch_u8.device and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == tuple(batch_u8.shape)):
        raise TypeError('jpeg_batch: out must be a contiguous uint8 tensor of the batch\'s shape on its device')
    if not (torch.is_tensor(quality_i32) and quality_i32.device == batch_u8.device and quality_i32.dtype == torch.int32
            and quality_i32.is_contiguous() and tuple(quality_i32.shape) == (n,)):
        raise TypeError('jpeg_batch: quality must be a contiguous (%d) int32 tensor on the batch\'s device' % n)
    lib, sub = L.load(), _SUBSAMPLING[subsampling]
    nbytes = int(lib.sr3_jpeg_scratch_bytes(n, H, W, Cc, sub))
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=batch_u8.device)       # (0: the call below says what it refuses)
    L.check(lib.sr3_jpeg_u8(L.ptr(batch_u8), n, H, W, Cc, L.ptr(quality_i32), sub, L.ptr(out), L.ptr(scratch), nbytes,
                            C.c_void_p(torch.cuda.current_stream(batch_u8.device).cuda_stream)))
    return out


def degrade_batch(hr_u8, deg, cfg, z=None, generator=None):
    """(n, R, R, C) uint8 crops (host or device), deg (n, 5) or (n, 6) per-image draws, cfg from degrade_config -> (lr_u8 (n, L, L, C),
    sr_u8 (n, R, R, C)) on the device.  z: the noise draws, fp32 of lr's shape (default: torch.randn on the device's default
    generator, or on `generator`), read only when a sample's noise sigma is not 0.  The sixth number is the JPEG quality of the LR
    image (0 = none): without it, or with every quality 0, the result is what the five numbers alone give."""
    if not isinstance(cfg, dict) or 'l_resolution' not in cfg:
        raise TypeError('degrade_batch takes the dict degrade_config() returns')
    if hr_u8.dtype != torch.uint8 or hr_u8.dim() != 4:
        raise TypeError('expected an (n, H, W, C) uint8 tensor')
    dev = _device(hr_u8)
    x = hr_u8.to(dev, non_blocking=True).contiguous()
    n, H, W, Cc = x.shape
    d = torch.as_tensor(deg).detach().to('cpu', torch.float64).numpy()
    if d.size not in (5 * n, 6 * n):
        raise ValueError('deg has shape %s, (%d, 5) or (%d, 6) expected' % (tuple(d.shape), n, n))
    d = d.reshape(n, -1)
    Lr, rs, k = cfg['l_resolution'], _RESAMPLE[cfg['resample']], cfg['blur']['kernel']
    if (d[:, 0] != 0).any():
        w = np.stack([blur_weights(r[1], r[2], r[3], k, on=r[0] != 0) for r in d])
        x = blur_batch(x, torch.from_numpy(w).to(dev, non_blocking=True))
    from data.prepare_data import resize_batch
    lr = resize_batch(x, (Lr, Lr), rs)
    if (d[:, 4] != 0).any():
        if z is None:
            z = torch.randn(lr.shape, dtype=torch.float32, device=dev, generator=generator)
        z = z.to(dev, torch.float32).contiguous()
        if tuple(z.shape) != tuple(lr.shape):
            raise ValueError('z has shape %s, the LR batch %s' % (tuple(z.shape), tuple(lr.shape)))
        noise_batch(lr, torch.from_numpy(d[:, 4].astype(np.float32)).to(dev, non_blocking=True), z, out=lr)
    if d.shape[1] == 6 and (d[:, 5] != 0).any():
        jpeg_batch(lr, torch.from_numpy(d[:, 5].astype(np.int32)).to(dev, non_blocking=True), cfg['jpeg']['subsampling'], out=lr)
    return lr, resize_batch(lr, (H, W), rs)
