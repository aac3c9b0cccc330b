"""The degradation between an HR crop and its conditioning images, on the MI355X (engine extension: the reference only reads
triplets data/prepare_data.py made with one fixed bicubic kernel):

    HR (n, R, R, C) --blur--> resize to (L, L) --noise--> --jpeg--> LR --resize to (R, R)--> SR

Blur (csrc/degrade.hip: sr3_blur_u8) is a per-image Gaussian in 16-bit fixed point, noise (sr3_noise_u8) is additive Gaussian in
8-bit levels on the LR image, JPEG (sr3_jpeg_u8) is the lossy half of Pillow's save / open round trip at a per-image quality (libjpeg's
integer arithmetic, bit for bit), both resizes are data.prepare_data.resize_batch (Pillow bit for bit).  With blur off, noise 0 and
no JPEG the pair is byte-identical to what prepare_data.py writes for the crop.  The per-image draws `deg` = [blur_on, sigma_x,
sigma_y, theta, noise_sigma (, jpeg_quality)] come from the dataset (data/HR_dataset.py); this module holds the config's one
validation, the kernel weights and the device chain.

The second-order model (config keys "sinc", "shot", "gray_noise", "second"; per-image draws `deg2`, draw_deg2) runs the same links
twice, through a random intermediate size M with a random filter per resize, and ends on a sinc filter around the second JPEG:

    HR --blur1 (Gaussian | sinc)--> resize to (M, M) --noise1--> jpeg1 --blur2 (Gaussian | sinc)--> resize to (L, L) --noise2-->
       --[final sinc, jpeg2: either order]--> LR --resize to (R, R)--> SR

The sinc (ringing) kernels go through sr3_blur_u8 like the Gaussians (sinc_weights: signed taps, the same fixed point), the noise is
sr3_noise_ex_u8 -- Gaussian or Poisson (an integer CDF table, poisson_table), per channel or gray --, the resizes add Pillow's BOX
filter.  Without any of the new keys nothing here draws or computes anything it did not before."""
import ctypes as C

import numpy as np
import torch
from PIL import Image

from sr3_hip import lib as L

MAX_KERNEL = 21
ONE = 1 << 16                     # fixed-point 1.0 of the blur weights
_RESAMPLE = {'bicubic': Image.BICUBIC, 'bilinear': Image.BILINEAR}
_RESAMPLE2 = dict(_RESAMPLE, box=Image.BOX)       # the filters of the rounds' down-resizes ("second.resample")
_ROUND = ('blur', 'sinc', 'noise', 'shot', 'gray_noise', 'jpeg')       # one degradation round's keys: top level = round 1, "second" = round 2
_KEYS = {None: ('blur', 'noise', 'jpeg', 'resample', 'seed', 'sinc', 'shot', 'gray_noise', 'second'),
         'blur': ('prob', 'kernel', 'sigma', 'anisotropic'), 'noise': ('prob', 'sigma'), 'jpeg': ('prob', 'quality', 'subsampling'),
         'sinc': ('prob', 'omega'), 'shot': ('prob', 'scale'), 'second': ('mid', 'resample') + _ROUND + ('final_sinc',),
         'final_sinc': ('prob', 'kernel', 'omega')}
_EXTENDED = ('sinc', 'shot', 'gray_noise', 'second')                   # a config with one of these draws 'deg2' too
_SUBSAMPLING = {'4:4:4': 0, '4:2:0': 2}           # Pillow's numbers, the ABI's
DEG2 = 20                         # numbers of draw_deg2's vector
POISSON_KMAX = 384                # columns of poisson_table: row 255 saturates at j = 359


def _known(block, name, prefix=''):
    """`name`: the block's key (None: the top level), `prefix`: the dotted path in front of it ('second.' for round 2's blocks)"""
    dotted = prefix + (name or '')
    if not isinstance(block, dict):
        raise ValueError('degrade%s: a dict of settings expected, got %r' % ('.' + dotted if dotted else '', block))
    for key in block:
        if key not in _KEYS[name]:
            raise ValueError('degrade: unknown key "%s%s" (known: %s)' % (dotted + '.' if dotted else '', key, ', '.join(_KEYS[name])))


def _prob(block, name, key='prob'):
    p = block.get(key, 1.0)              # a block that is present is on unless it says otherwise
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:
        raise ValueError('degrade: %s%s %r is not a probability in [0, 1]' % (name + '.' if name else '', key, p))
    return float(p)


def _range(block, name, default, lo_open, key='sigma', hi_max=float('inf')):
    s = block.get(key, default)
    if not isinstance(s, (list, tuple)) or len(s) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, float)) for v in s):
        raise ValueError('degrade: %s.%s %r is not a [lo, hi] pair of numbers' % (name, key, s))
    lo, hi = float(s[0]), float(s[1])
    if hi_max < float('inf'):
        if not (0.0 < lo <= hi <= hi_max):
            raise ValueError('degrade: %s.%s %r needs 0 < lo <= hi <= pi' % (name, key, s))
    elif not ((0.0 < lo if lo_open else 0.0 <= lo) and lo <= hi and hi < float('inf')):
        raise ValueError('degrade: %s.%s %r needs %s lo <= hi' % (name, key, s, '0 <' if lo_open else '0 <='))
    return lo, hi


def _quality(block, name='jpeg'):
    q = block.get('quality', (30, 95))
    if not isinstance(q, (list, tuple)) or len(q) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in q):
        raise ValueError('degrade: %s.quality %r is not a [lo, hi] pair of integers' % (name, q))
    if not 1 <= q[0] <= q[1] <= 100:
        raise ValueError('degrade: %s.quality %r needs 1 <= lo <= hi <= 100' % (name, q))
    return int(q[0]), int(q[1])


def _kernel(block, name, default):
    k = block.get('kernel', default)
    if isinstance(k, bool) or not isinstance(k, int) or k < 1 or k > MAX_KERNEL or k % 2 == 0:
        raise ValueError('degrade: %s.kernel %r is not an odd integer in 1..%d' % (name, k, MAX_KERNEL))
    return k


def _round(cfg, prefix):
    """One round's blocks (cfg: the top level, or the "second" dict with prefix 'second.') -> their normalised values.  The old
    blocks keep exactly their keys; an absent new block is off."""
    blur, noise = cfg.get('blur', {'prob': 0.0}), cfg.get('noise', {'prob': 0.0})
    _known(blur, 'blur', prefix)
    _known(noise, 'noise', prefix)
    jpeg = cfg['jpeg'] if 'jpeg' in cfg else {'prob': 0.0}
    _known(jpeg, 'jpeg', prefix)
    sub = jpeg.get('subsampling', '4:2:0')
    if not isinstance(sub, str) or sub not in _SUBSAMPLING:
        raise ValueError('degrade: %sjpeg.subsampling %r is not "4:2:0" or "4:4:4"' % (prefix, sub))
    k = _kernel(blur, prefix + 'blur', MAX_KERNEL)
    aniso = blur.get('anisotropic', False)
    if not isinstance(aniso, bool):
        raise ValueError('degrade: %sblur.anisotropic %r is not a bool' % (prefix, aniso))
    sinc, shot = cfg.get('sinc', {'prob': 0.0}), cfg.get('shot', {'prob': 0.0})
    _known(sinc, 'sinc', prefix)
    _known(shot, 'shot', prefix)
    return {'blur': {'prob': _prob(blur, prefix + 'blur'), 'kernel': k, 'sigma': _range(blur, prefix + 'blur', (0.2, 3.0), True), 'anisotropic': aniso},
            'noise': {'prob': _prob(noise, prefix + 'noise'), 'sigma': _range(noise, prefix + 'noise', (0.0, 0.0), False)},
            'jpeg': {'prob': _prob(jpeg, prefix + 'jpeg'), 'quality': _quality(jpeg, prefix + 'jpeg'), 'subsampling': sub, 'given': 'jpeg' in cfg},
            'sinc': {'prob': _prob(sinc, prefix + 'sinc'), 'omega': _range(sinc, prefix + 'sinc', (1.05, 3.14), True, 'omega', np.pi)},
            'shot': {'prob': _prob(shot, prefix + 'shot'), 'scale': _range(shot, prefix + 'shot', (0.05, 3.0), True, 'scale')},
            'gray_noise': _prob({'gray_noise': cfg.get('gray_noise', 0.0)}, prefix.rstrip('.'), 'gray_noise')}


def _second(sec, l_resolution, resample):
    """The "second" block -> round 2's normalised values plus 'mid', 'resample' (a tuple of names) and 'final_sinc'."""
    _known(sec, 'second')
    out = _round(sec, 'second.')
    mid = sec.get('mid', (l_resolution, l_resolution))
    if not isinstance(mid, (list, tuple)) or len(mid) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in mid):
        raise ValueError('degrade: second.mid %r is not a [lo, hi] pair of integers' % (mid,))
    if not 1 <= mid[0] <= mid[1]:
        raise ValueError('degrade: second.mid %r needs 1 <= lo <= hi' % (mid,))
    k2 = out['blur']['kernel']
    if 'blur' in sec and k2 // 2 >= mid[0]:
        raise ValueError('degrade: second.mid %r: second.blur.kernel %d reflects past a %d x %d image (kernel // 2 must be below mid)'
                         % (mid, k2, mid[0], mid[0]))
    names = sec.get('resample', [resample])
    if not isinstance(names, (list, tuple)) or len(names) == 0:
        raise ValueError('degrade: second.resample %r is not a non-empty list of filter names' % (names,))
    for nm in names:
        if not isinstance(nm, str) or nm not in _RESAMPLE2:
            raise ValueError('degrade: second.resample %r: %r is not "box", "bilinear" or "bicubic"' % (names, nm))
    fs = sec.get('final_sinc', {'prob': 0.0})
    _known(fs, 'final_sinc', 'second.')
    kf = _kernel(fs, 'second.final_sinc', 7)
    if 'final_sinc' in sec and kf // 2 >= l_resolution:
        raise ValueError('degrade: second.final_sinc.kernel %d reflects past the %d x %d LR image (kernel // 2 must be below l_resolution)'
                         % (kf, l_resolution, l_resolution))
    out.update(mid=(int(mid[0]), int(mid[1])), resample=tuple(names),
               final_sinc={'prob': _prob(fs, 'second.final_sinc'), 'kernel': kf,
                           'omega': _range(fs, 'second.final_sinc', (1.05, 3.14), True, 'omega', np.pi)})
    return out


def degrade_config(cfg, l_resolution):
    """The one validation of a dataset block's "degrade" value (every key optional; {} = plain bicubic):
        {"blur": {"prob": p, "kernel": k, "sigma": [lo, hi], "anisotropic": bool}, "noise": {"prob": p, "sigma": [lo, hi]},
         "jpeg": {"prob": p, "quality": [lo, hi], "subsampling": "4:2:0" | "4:4:4"}, "resample": "bicubic" | "bilinear", "seed": 0}
    -> the normalised dict degrade_batch and the datasets read (every key present, plus 'l_resolution'; 'jpeg' also says whether the
    key was 'given': draw_deg's result has a sixth number only then).  ValueError names what it refuses: an unknown key, an even
    kernel or one outside 1..21, blur sigmas without 0 < lo <= hi, noise sigmas without 0 <= lo <= hi, JPEG qualities that are not
    integers with 1 <= lo <= hi <= 100, an unknown subsampling, a probability outside [0, 1], an unknown resample, a seed that is
    not an integer.

    The second-order keys (all optional, all top-level; 'extended' in the result says whether any was given -- the datasets then draw
    'deg2' as well, draw_deg2):
        "sinc": {"prob": p, "omega": [lo, hi]}    of the samples whose blur is on, this share gets a sinc (ringing) kernel of size
                                                  blur.kernel and cut-off omega instead of the Gaussian; 0 < lo <= hi <= pi
        "shot": {"prob": p, "scale": [lo, hi]}    of the noisy samples, this share gets Poisson noise scaled by `scale` (0 < lo <= hi)
        "gray_noise": p                           the probability that a sample's noise is one value per pixel
        "second": {"mid": [lo, hi], "resample": ["box", "bilinear", "bicubic"], "blur", "sinc", "noise", "shot", "gray_noise", "jpeg":
                   round 2, the same sub-schemas, "final_sinc": {"prob": p, "kernel": k, "omega": [lo, hi]}}
    With "second", round 1 lands on M x M, M one integer of mid per batch (it may exceed r_resolution), each round's down-resize uses
    one filter of second.resample per batch, and a sinc filter runs on the LR image before or after round 2's JPEG.  Refused as
    well: omegas outside 0 < lo <= hi <= pi, a mid that is not integers with 1 <= lo <= hi, a mid that second.blur.kernel or an
    l_resolution that second.final_sinc.kernel would reflect past (kernel // 2 >= size), an empty or unknown second.resample."""
    cfg = {} if cfg is None else cfg
    _known(cfg, None)
    first = _round(cfg, '')
    resample = cfg.get('resample', 'bicubic')
    if resample not in _RESAMPLE:
        raise ValueError('degrade: resample %r is not "bicubic" or "bilinear"' % (resample,))
    seed = cfg.get('seed', 0)
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError('degrade: seed %r is not an integer' % (seed,))
    if isinstance(l_resolution, bool) or not isinstance(l_resolution, int) or l_resolution < 1:
        raise ValueError('degrade: l_resolution %r is not a positive integer' % (l_resolution,))
    second = _second(cfg['second'], l_resolution, resample) if 'second' in cfg else None
    return dict(first, resample=resample, seed=seed, l_resolution=l_resolution, second=second,
                extended=any(key in cfg for key in _EXTENDED))


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


def _lerp(pair, u):
    return pair[0] + (pair[1] - pair[0]) * u


def _pick(lo, hi, u):
    """u uniform in [0, 1) -> an integer of lo..hi, each equally likely"""
    return min(hi, lo + int(u * (hi - lo + 1)))


def draw_deg2(cfg, generator=None):
    """The second-order numbers of one sample (fp32, (20,)); the datasets call it right after draw_deg, and only for a config whose
    'extended' is true.  Always 24 uniform draws (the last is spare), whatever is switched on:
         0 sinc1_on   1 omega1   2 noise1_mode (0 Gaussian colour, 1 Gaussian gray, 2 Poisson colour, 3 Poisson gray)   3 shot1_scale
         4 mid size M   5 resample1   6 resample2 (Pillow's numbers: 2 bilinear, 3 bicubic, 4 box)
         7-10 blur2_on, sigma_x2, sigma_y2, theta2   11 sinc2_on   12 omega2   13 noise2_sigma (0 = off)   14 noise2_mode
        15 shot2_scale   16 jpeg2_quality (0 = off)   17 final_sinc_on   18 omega_f   19 jpeg_before_final_sinc
    Without "second": M = l_resolution, both resamples the top-level filter, 7-19 zero.  Numbers 4-6 are per BATCH: degrade_batch
    reads them from row 0 and ignores the other rows' draws.  A sinc switch only matters where its blur is on, a mode and a shot scale
    only where the noise is (round 1: draw_deg's noise_sigma != 0; in the Poisson modes that sigma only says "on")."""
    u = torch.rand(24, generator=generator).tolist()

    def mode(c, u_shot, u_gray):
        return 2.0 * (u_shot < c['shot']['prob']) + 1.0 * (u_gray < c['gray_noise'])

    top = float(_RESAMPLE[cfg['resample']])
    d = [0.0] * DEG2
    d[0], d[1] = float(u[0] < cfg['sinc']['prob']), _lerp(cfg['sinc']['omega'], u[1])
    d[2], d[3] = mode(cfg, u[2], u[3]), _lerp(cfg['shot']['scale'], u[4])
    d[4], d[5], d[6] = float(cfg['l_resolution']), top, top
    s = cfg.get('second')
    if s is not None:
        b, n, j, f = s['blur'], s['noise'], s['jpeg'], s['final_sinc']
        names = s['resample']
        d[4] = float(_pick(s['mid'][0], s['mid'][1], u[5]))
        d[5] = float(_RESAMPLE2[names[_pick(0, len(names) - 1, u[6])]])
        d[6] = float(_RESAMPLE2[names[_pick(0, len(names) - 1, u[7])]])
        d[7], d[8] = float(u[8] < b['prob']), _lerp(b['sigma'], u[9])
        d[9] = _lerp(b['sigma'], u[10]) if b['anisotropic'] else d[8]
        d[10] = np.pi * u[11] if b['anisotropic'] else 0.0
        d[11], d[12] = float(u[12] < s['sinc']['prob']), _lerp(s['sinc']['omega'], u[13])
        d[13] = _lerp(n['sigma'], u[15]) if u[14] < n['prob'] else 0.0
        d[14], d[15] = mode(s, u[16], u[17]), _lerp(s['shot']['scale'], u[18])
        d[16] = float(_pick(j['quality'][0], j['quality'][1], u[19] / j['prob'])) if u[19] < j['prob'] else 0.0
        d[17], d[18] = float(u[20] < f['prob']), _lerp(f['omega'], u[21])
        d[19] = float(u[22] < 0.5)
    return torch.tensor(d, dtype=torch.float32)


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


def sinc_weights(omega, k):
    """(k, k) int32 ideal circular low-pass of cut-off omega (0 < omega <= pi) in blur_weights' fixed point, in NumPy float64:
    h(r) = omega J1(omega r) / (2 pi r), h(0) = omega^2 / (4 pi) (J1: scipy.special.j1), normalised to sum 1, q = floor(w * 65536 +
    0.5), the centre tap takes 65536 - q.sum().  The side lobes are negative (k >= 7): the blurred image rings, and sr3_blur_u8
    clamps the overshoot.  For 3 <= k <= 21 and omega in [1.05, pi] every |w| <= 5.3e4 and sum |w| * 255 <= 1.0e8 (a 400-point sweep of
    omega per k: 52620 at k = 7, omega = pi; 9.92e7 at k = 21, omega = 2.97): inside what sr3_blur_u8 documents (|w| < 2^23, int32
    accumulator)."""
    from scipy.special import j1
    k = int(k)
    if k < 1 or k > MAX_KERNEL or k % 2 == 0:
        raise ValueError('sinc_weights: k %r is not an odd integer in 1..%d' % (k, MAX_KERNEL))
    om = float(omega)
    if not 0.0 < om <= np.pi:
        raise ValueError('sinc_weights: omega %r is not in (0, pi]' % (omega,))
    dy, dx = np.mgrid[0:k, 0:k].astype(np.float64) - (k // 2)
    r = np.sqrt(dx * dx + dy * dy)
    r[k // 2, k // 2] = 1.0                              # (any value: the centre is set below)
    h = om * j1(om * r) / (2.0 * np.pi * r)
    h[k // 2, k // 2] = om * om / (4.0 * np.pi)
    w = h / h.sum()
    q = np.floor(w * ONE + 0.5).astype(np.int64)
    q[k // 2, k // 2] += ONE - q.sum()
    return q.astype(np.int32)


_POISSON = {}                     # None: the host table; a device: its copy


def poisson_table():
    """(256, 384) int32, T[v][j] = min(floor(CDF_Poisson(lambda = v)(j) * 2^31), 2^31 - 1), by the float64 recurrence p_0 = exp(-v),
    p_j = p_{j-1} v / j (the integers scipy.stats.poisson.cdf gives, on all 256 rows).  Row 0 is all 2^31 - 1; row 255 saturates at
    j = 359.  A Poisson draw of mean v is k = #{j : T[v][j] <= r} for an integer r uniform in [0, 2^31 - 1): integer arithmetic, the
    same on the device (sr3_noise_ex_u8) and in NumPy.  The distribution it implies has |mean - v| <= 1.8e-7, |var - v| <= 6.9e-5."""
    if None not in _POISSON:
        lam = np.arange(256, dtype=np.float64)[:, None]
        p = np.empty((256, POISSON_KMAX), dtype=np.float64)
        p[:, 0] = np.exp(-lam[:, 0])
        for j in range(1, POISSON_KMAX):
            p[:, j] = p[:, j - 1] * lam[:, 0] / j
        t = np.minimum(np.floor(np.cumsum(p, axis=1) * 2.0 ** 31), 2.0 ** 31 - 1).astype(np.int32)
        t.setflags(write=False)
        _POISSON[None] = t
    return _POISSON[None]


def _poisson_on(dev):
    if dev not in _POISSON:
        _POISSON[dev] = torch.from_numpy(poisson_table().copy()).to(dev)
    return _POISSON[dev]


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


def noise_ex_batch(batch_u8, mode_i32, strength_f32, z_f32=None, r_i32=None, out=None):
    """Noise with a per-image kind on an (n, H, W, C) uint8 batch (out may be `batch_u8` itself): sr3_noise_ex_u8.  mode (n) int32 --
    0 Gaussian colour, 1 Gaussian gray, 2 Poisson colour, 3 Poisson gray --, strength (n) fp32 -- sigma resp. the Poisson scale, 0
    copies --, z fp32 and r int32 (uniform in [0, 2^31 - 1)) of the batch's shape; z resp. r may be None when no image with nonzero
    strength has a Gaussian resp. Poisson mode."""
    if not (torch.is_tensor(batch_u8) and batch_u8.is_cuda and batch_u8.dtype == torch.uint8 and batch_u8.dim() == 4 and batch_u8.is_contiguous()):
        raise TypeError('noise_ex_batch: a contiguous (n, H, W, C) uint8 batch on the device expected (there is no CPU fallback)')
    n, H, W, Cc = batch_u8.shape
    if out is None:
        out = torch.empty_like(batch_u8)
    dev = batch_u8.device
    checks = [(out, torch.uint8, batch_u8.shape), (mode_i32, torch.int32, (n,)), (strength_f32, torch.float32, (n,))]
    checks += [(t, dt, batch_u8.shape) for t, dt in ((z_f32, torch.float32), (r_i32, torch.int32)) if t is not None]
    for t, dt, shape in checks:
        if not (torch.is_tensor(t) and t.device == dev and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
            raise TypeError('noise_ex_batch: contiguous tensors on the batch\'s device expected -- uint8 out, fp32 z and int32 r of the '
                            'batch\'s shape, int32 mode (n), fp32 strength (n)')
    table = None if r_i32 is None else _poisson_on(dev)
    L.check(L.load().sr3_noise_ex_u8(L.ptr(batch_u8), n, H, W, Cc, L.ptr(mode_i32), L.ptr(strength_f32), L.ptr(z_f32), L.ptr(r_i32),
                                     L.ptr(table), POISSON_KMAX, L.ptr(out), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
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


def _draws(given, shape, dev, generator, integers):
    """a round's noise draws: the caller's, or fresh ones -- z: torch.randn, r: integers uniform in [0, 2^31 - 1)"""
    if given is None:
        if integers:
            return torch.randint(0, 2 ** 31 - 1, tuple(shape), dtype=torch.int32, device=dev, generator=generator)
        return torch.randn(tuple(shape), dtype=torch.float32, device=dev, generator=generator)
    t = given.to(dev, torch.int32 if integers else torch.float32).contiguous()
    if tuple(t.shape) != tuple(shape):
        raise ValueError('%s has shape %s, the batch it is drawn for %s' % ('r' if integers else 'z', tuple(t.shape), tuple(shape)))
    return t


def _noise_round(x, on, sigma, mode, scale, z, r, generator):
    """One round's noise, in place on x (n, S, S, C): image i is noisy where on[i], Gaussian of sigma[i] or (mode 2, 3) Poisson scaled by
    scale[i].  z is drawn (when not passed) before r, and each only when an image needs it."""
    if not on.any():
        return x
    dev = x.device
    poisson = mode >= 2
    strength = np.where(on, np.where(poisson, scale, sigma), 0.0).astype(np.float32)
    zz = _draws(z, x.shape, dev, generator, False) if (on & ~poisson).any() else None
    rr = _draws(r, x.shape, dev, generator, True) if (on & poisson).any() else None
    return noise_ex_batch(x, torch.from_numpy(mode.astype(np.int32)).to(dev, non_blocking=True),
                          torch.from_numpy(strength).to(dev, non_blocking=True), zz, rr, out=x)


def _kernels(on, sinc_on, omega, sx, sy, theta, k):
    """(n, k, k) int32: image i's delta, Gaussian or (sinc_on[i]) sinc kernel (omega as fp32 may sit one ulp above pi)"""
    return np.stack([blur_weights(sx[i], sy[i], theta[i], k, on=False) if not on[i] else
                     (sinc_weights(min(omega[i], np.pi), k) if sinc_on[i] else blur_weights(sx[i], sy[i], theta[i], k))
                     for i in range(len(on))])


def _degrade_batch2(x, d, d2, cfg, z, r, z2, r2, generator):
    """degrade_batch's second-order chain: x (n, H, W, C) on the device, d (n, 5 | 6) and d2 (n, 20) float64."""
    from data.prepare_data import resize_batch
    dev, n, sec = x.device, x.shape[0], cfg['second']
    H, W, Lr = x.shape[1], x.shape[2], cfg['l_resolution']
    M, rs1, rs2 = int(d2[0, 4]), int(d2[0, 5]), int(d2[0, 6])            # per batch: row 0 speaks for all
    if M < 1 or rs1 not in (2, 3, 4) or rs2 not in (2, 3, 4):
        raise ValueError('deg2 row 0: mid size %r and resamples %r, %r (Pillow\'s 2, 3 or 4) expected' % (d2[0, 4], d2[0, 5], d2[0, 6]))

    def upload(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev, non_blocking=True)

    # round 1: blur (Gaussian | sinc) -> resize to M -> noise -> JPEG
    on = d[:, 0] != 0
    if on.any():
        x = blur_batch(x, upload(_kernels(on, d2[:, 0] != 0, d2[:, 1], d[:, 1], d[:, 2], d[:, 3], cfg['blur']['kernel']), np.int32))
    x = resize_batch(x, (M, M) if sec is not None else (Lr, Lr), rs1)
    x = _noise_round(x, d[:, 4] != 0, d[:, 4], d2[:, 2], d2[:, 3], z, r, generator)
    if d.shape[1] == 6 and (d[:, 5] != 0).any():
        jpeg_batch(x, upload(d[:, 5], np.int32), cfg['jpeg']['subsampling'], out=x)
    if sec is not None:
        # round 2: blur -> resize to L -> noise -> [final sinc, JPEG in the sample's order]
        on = d2[:, 7] != 0
        if on.any():
            x = blur_batch(x, upload(_kernels(on, d2[:, 11] != 0, d2[:, 12], d2[:, 8], d2[:, 9], d2[:, 10], sec['blur']['kernel']), np.int32))
        x = resize_batch(x, (Lr, Lr), rs2)
        x = _noise_round(x, d2[:, 13] != 0, d2[:, 13], d2[:, 14], d2[:, 15], z2, r2, generator)
        # the two orders as two subsets of the batch: a quality 0 passes its image through the JPEG entry, a delta kernel copies
        q, first = d2[:, 16], d2[:, 19] != 0
        fs, kf = d2[:, 17] != 0, sec['final_sinc']['kernel']
        if (first & (q != 0)).any():
            jpeg_batch(x, upload(np.where(first, q, 0), np.int32), sec['jpeg']['subsampling'], out=x)
        if fs.any():
            zero = np.zeros(n)
            x = blur_batch(x, upload(_kernels(fs, fs, d2[:, 18], zero, zero, zero, kf), np.int32))
        if (~first & (q != 0)).any():
            jpeg_batch(x, upload(np.where(first, 0, q), np.int32), sec['jpeg']['subsampling'], out=x)
    return x, resize_batch(x, (H, W), _RESAMPLE[cfg['resample']])


def degrade_batch(hr_u8, deg, cfg, z=None, generator=None, *, deg2=None, r=None, z2=None, r2=None):
    """(n, R, R, C) uint8 crops (host or device), deg (n, 5) or (n, 6) per-image draws, cfg from degrade_config -> (lr_u8 (n, L, L, C),
    sr_u8 (n, R, R, C)) on the device.  z: the noise draws, fp32 of lr's shape (default: torch.randn on the device's default
    generator, or on `generator`), read only when a sample's noise sigma is not 0.  The sixth number is the JPEG quality of the LR
    image (0 = none): without it, or with every quality 0, the result is what the five numbers alone give.

    deg2 (n, 20), draw_deg2's numbers, runs the second-order chain (deg2=None: the chain above, call for call):
        HR --blur1 (Gaussian | sinc)--> resize to M (resample1) --noise1 (mode)--> jpeg1
           --blur2 (Gaussian | sinc)--> resize to L (resample2) --noise2 (mode)
           --[final sinc, jpeg2 in the sample's order]--> LR --resize to R (top-level resample)--> SR
    M, resample1 and resample2 (deg2[:, 4:7]) are per BATCH: they are read from ROW 0 of deg2 and the other rows' values are
    ignored (a validation batch holds one item, so validation stays deterministic per index).  Without "second" in cfg round 1
    resizes straight to L and round 2 and the final stage are skipped.  Noise is sr3_noise_ex_u8: round 1 is on where deg[:, 4] != 0
    (Poisson modes: the strength is deg2[:, 3], deg[:, 4] only says "on"), round 2 where deg2[:, 13] != 0.  Draws that are not passed
    come from `generator` or the device's default one, per round z before r and each only when an image of the batch needs it: z, z2
    fp32 (torch.randn), r, r2 int32 (torch.randint(0, 2**31 - 1)) -- z, r of round 1's (n, M, M, C), z2, r2 of the LR batch's shape."""
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
    if deg2 is not None:
        d2 = torch.as_tensor(deg2).detach().to('cpu', torch.float64).numpy()
        if d2.size != DEG2 * n:
            raise ValueError('deg2 has shape %s, (%d, %d) expected' % (tuple(d2.shape), n, DEG2))
        return _degrade_batch2(x, d, d2.reshape(n, DEG2), cfg, z, r, z2, r2, generator)
    Lr, rs, k =cfg['l_resolution'], _RESAMPLE[cfg['resample']], cfg['blur']['kernel']
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
