"""What is done to the predicted x0 between the network's output and the posterior mix, once: the rules on x0.

A rule owns the whole tail of a reverse step (a HIP entry built on csrc/step_tail.h's frame): consistency (the block-mean projection,
sr3_consistent_step), guidance (classifier-free guidance and the threshold on x0, sr3_guided_step), back-projection (iterative
back-projection under Pillow's resize, sr3_backproject_step), restore (a mask or a channel sum, sr3_restore_step).  RULES is the ordered table EngineDiffusion loops over -- in
set_new_noise_schedule, in its one settings check (_check_settings, which calls check_rule below), in _loop_state (the key, the buffers,
the step form), in _capture (warm_on_capture_stream) and in _sample_shape / _begin_chain (the targets).  The rules exclude one another
and tiling (each owns the tail); a new rule on x0 is one entry here and one kernel.

The config keys (engine extensions, next to "sampler" / "tiling" in the schedule dict, or the setters).  Per step: UNet forward with the
output stored, then the rule's entry in place of the fused tail.
  `"consistency": {"block": 8, "strength": 1.0}` / `set_consistency`: every step shifts each block x block block of x0 so that its mean is
    the target's -- the block means of the conditioning image, or `consistency_target=` (the range / null-space projection for an
    average pool; sr3_consistent_step).
  `"guidance": {"scale": 1.5, "threshold": "dynamic", "percentile": 0.995}` / `set_guidance` (`"cond_drop": p` in model.diffusion, or
    `set_cond_drop`, trains a model for it): classifier-free guidance -- two forwards per step, on the conditioning image and on a zero
    one, combined as out_u + scale (out_c - out_u) before x0 is formed -- and what is done to x0 where it leaves [-1, 1]: the static
    clamp, nothing, or dynamic thresholding (each image's x0 divided by its own percentile of |x0|; sr3_guided_step).
  `"backprojection": {"scale": 8, "iterations": 2, "strength": 1.0, "resample": "bicubic"}` / `set_backprojection`: `iterations` rounds of
    x0 <- x0 + strength * U(y - D(x0)), D / U = Pillow's antialiased resize down / up by `scale` (`resample_tables`), y = the LR image
    (`backprojection_target=`) or the down-sampled conditioning image (sr3_backproject_step).  A contraction, not a projection.
  `"restore": {"operator": "mask" | "gray", "strength": 1.0, "weights": "mean" | "rec601" | [..], "travel": {"length": l, "repeats": r}}` /
    `set_restore`: zero-shot restoration -- every step projects x0 onto what is known of the image (sr3_restore_step).  mask: x0' = w y +
    (1 - w) x0, w = strength * mask, towards `restore_target=(known, mask)` (inpainting, outpainting, a trusted patch).  gray: x0'_c =
    x0_c + strength * p_c (y - a . x0) with the channel weights a and p = a / |a|^2, towards `restore_target=` a gray image [B, 1, H, W]
    or a colour image (reduced with `gray_f32`), by default the conditioning image's gray (colourisation).  travel: every segment of
    `length` step indices runs `repeats` times, the chain diffused back up in between (`travel_walk`, `travel_tables`,
    sr3_travel_back_f32).  The one rule that also runs on the DDPM variant under a sampler: its forward takes the sampler's walk.

A Rule supplies: `name` (the config key, the attribute of EngineDiffusion, the state key and the _loop_state keyword), `noun` (in
messages), `setter`, `entry`; `parse(spec)` -- the config key -> the setter's arguments; `validate(diff, *args)` -- the setter's body ->
the setting as a dict, or None for off; `key(cfg)` -- its component of the loop-state key; `buffers(st, cfg, shape, cond_shape, dev)`;
`check_target` / `prepare` -- the per-chain target (`target_kw`: the keyword of p_sample_loop that carries it, or None); `tail` -- the
entry call behind the forward that stored the output in st['eps'].

Also here, because they belong to the rules: block_means, resample_tables, resample_f32, backprojection_error, quantile_rank,
gray_weights, gray_f32, restore_error, travel_walk, travel_tables.
"""
import ctypes as C

import numpy as np
import torch

from . import lib as L


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


CONSISTENCY_BLOCKS = (2, 4, 8, 16, 32)      # what sr3_consistent_step takes


def block_means(x, block):
    """The means of the block x block blocks of x [B, C, H, W] (a contiguous fp32 GPU tensor): [B, C, H / block, W / block], each summed
    in double and rounded once (sr3_block_mean_f32).  max |block_means(SR, r) - block_means(cond, r)| is the consistency error of a
    result."""
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
        raise L.Sr3Error('block_means needs a (B, C, H, W) fp32 GPU tensor; there is no CPU fallback')
    x = x.contiguous()
    B, Cc, H, W = x.shape
    block = int(block)
    out = torch.empty((B, Cc, H // max(block, 1), W // max(block, 1)), device=x.device)
    L.check(L.load().sr3_block_mean_f32(L.ptr(x), B, Cc, H, W, block, L.ptr(out), C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)))
    return out


RESAMPLES = ('bicubic', 'bilinear')      # the filters of resample_tables: Pillow's BICUBIC (a = -0.5, support 2) and BILINEAR (support 1)
BACKPROJECTION_KEYS = ('scale', 'iterations', 'strength', 'resample')


def _resample_filter(resample):
    if resample == 'bicubic':
        def f(x):
            x = np.abs(x)
            a = -0.5
            return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0,
                            np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))
        return f, 2.0
    if resample == 'bilinear':
        return (lambda x: np.where(np.abs(x) < 1.0, 1.0 - np.abs(x), 0.0)), 1.0
    raise ValueError('resample must be one of %s (got %r)' % (', '.join(repr(k) for k in RESAMPLES), resample))


def resample_tables(in_size, out_size, resample='bicubic'):
    """The banded matrix of Pillow's resize of one axis from in_size to out_size elements (Image.resize with BICUBIC / BILINEAR; its
    precompute_coeffs rule, evaluated in float64): the filter's support scaled by max(in / out, 1) (the antialiasing of a down-sample),
    output xx centred at (xx + 0.5) in / out, taps xmin = max(int(c - support + 0.5), 0) up to xmax = min(int(c + support + 0.5), in),
    weights normalised by their sum.  -> (bounds int32 [out, 2] = (first tap, count), weights fp32 [out, ksize], rounded once from
    float64 and zero past the count): what sr3_resample_f32 / sr3_backproject_step take.  Pure NumPy, no device."""
    for name, v in (('in_size', in_size), ('out_size', out_size)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1:
            raise ValueError('resample_tables: %s must be a positive integer (got %r)' % (name, v))
    filt, support = _resample_filter(resample)
    in_size, out_size = int(in_size), int(out_size)
    scale = np.float64(in_size) / np.float64(out_size)
    fscale = max(scale, np.float64(1.0))
    support = np.float64(support) * fscale
    ksize = int(np.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    w64 = np.zeros((out_size, ksize), dtype=np.float64)
    for xx in range(out_size):
        c = (np.float64(xx) + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        xmax = min(int(c + support + 0.5), in_size)
        n = xmax - xmin
        w = filt((np.arange(n, dtype=np.float64) + xmin - c + 0.5) / fscale)
        s = w.sum()
        if s != 0.0:
            w = w / s
        bounds[xx] = (xmin, n)
        w64[xx, :n] = w
    return bounds, w64.astype(np.float32)      # (ksize = Pillow's: 2 ceil(support) + 1, an upper bound of every row's count)


def _resample_device_tables(in_hw, out_hw, resample, dev):
    """the four tables of one 2-D resample on the device: (bounds_h, weights_h, bounds_v, weights_v); horizontal = the width axis"""
    out = []
    for i, o in ((in_hw[1], out_hw[1]), (in_hw[0], out_hw[0])):
        b, w = resample_tables(i, o, resample)
        out += [torch.from_numpy(b).to(dev), torch.from_numpy(w).to(dev)]
    return tuple(out)


def resample_f32(x, out_hw, resample='bicubic', tables=None):
    """Pillow's resize of the planes of x [B, C, H, W] (a contiguous fp32 GPU tensor) to out_hw = (OH, OW), in fp32 on the device
    (sr3_resample_f32; the tables of `resample_tables`, or `tables` = the four device tensors made for this geometry before)."""
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
        raise L.Sr3Error('resample_f32 needs a (B, C, H, W) fp32 GPU tensor; there is no CPU fallback')
    x = x.contiguous()
    B, Cc, H, W = x.shape
    OH, OW = int(out_hw[0]), int(out_hw[1])
    bh, wh, bv, wv = tables if tables is not None else _resample_device_tables((H, W), (OH, OW), resample, x.device)
    out = torch.empty((B, Cc, OH, OW), device=x.device)
    tmp = torch.empty((B, Cc, H, OW), device=x.device)
    L.check(L.load().sr3_resample_f32(L.ptr(x), B * Cc, H, W, L.ptr(out), OH, OW, L.ptr(bh), L.ptr(wh), wh.shape[1], L.ptr(bv), L.ptr(wv),
                                      wv.shape[1], L.ptr(tmp), None, None, C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)))
    return out


def backprojection_error(sr, y_lr, scale, resample='bicubic'):
    """max |D(sr) - y_lr|: how far the result sr [B, C, H, W] is from the LR image y_lr [B, C, H / scale, W / scale] under the dataset's
    down-sample D (Pillow's resize, sr3_resample_f32).  fp32 GPU tensors."""
    if not torch.is_tensor(sr) or sr.dim() != 4:
        raise L.Sr3Error('backprojection_error needs a (B, C, H, W) fp32 GPU tensor; there is no CPU fallback')
    scale = int(scale)
    B, Cc, H, W = sr.shape
    if scale < 1 or H % scale or W % scale or tuple(y_lr.shape) != (B, Cc, H // scale, W // scale):
        raise L.Sr3Error('backprojection_error: y_lr must be a %s tensor (got %s)' % ((B, Cc, H // max(scale, 1), W // max(scale, 1)), tuple(y_lr.shape)))
    d = resample_f32(sr, (H // scale, W // scale), resample)
    return float((d - y_lr.to(d.device, torch.float32)).abs().max())


THRESHOLDS = ('none', 'static', 'dynamic')      # the mode numbers of sr3_guided_step, in order


def quantile_rank(n, p):
    """Where the p-quantile (p in [0, 1]) of n sorted values sits, as sr3_abs_quantile_f32 takes it: (rank_lo, frac) with
    pos = p (n - 1), rank_lo = floor(pos), frac = pos - rank_lo in [0, 1), all in float64 (numpy.quantile's 'linear' rule).  Pure, no device."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or int(n) < 1:
        raise ValueError('quantile_rank: n must be a positive integer (got %r)' % (n,))
    try:
        pf = float(p)
    except (TypeError, ValueError):
        raise ValueError('quantile_rank: p must be a number (got %r)' % (p,))
    if isinstance(p, bool) or not 0.0 <= pf <= 1.0:
        raise ValueError('quantile_rank: p must lie in [0, 1] (got %r)' % (p,))
    pos = np.float64(pf) * np.float64(int(n) - 1)
    rank_lo = int(np.floor(pos))
    return rank_lo, float(pos - np.float64(rank_lo))

def _number(name, v, ok, want):
    """v as a float: a number (no bool) for which ok(float) holds, else ValueError('<name> must <want> (got ...)')"""
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError('%s must be a number (got %r)' % (name, v))
    if isinstance(v, bool) or not ok(f):
        raise ValueError('%s must %s (got %r)' % (name, want, v))
    return f


def _is_int(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _first_channels(st, Cc):
    """the conditioning image's first Cc channels, contiguous: what a target is made from where none is given"""
    return st['cond'] if st['cond'].shape[1] == Cc else st['cond'][:, :Cc].contiguous()


class Rule:
    target_kw = None                  # the keyword of p_sample_loop / super_resolution that carries the chain's target
    warm_on_capture_stream = False    # _capture: the eager warm-up step runs on the stream the capture runs on
    takes_t_map = False               # its forward hands the sampler's step-index -> timestep map on (the DDPM variant under a sampler)
    key_appended = False              # its loop-state key component is appended behind the older ones, and only where the rule is on

    def key(self, cfg):
        return None if cfg is None else tuple(cfg[k] for k in self.keys)

    def missing_target(self, cfg, conditional):
        """why a chain without `target_kw` cannot run (None: it can: the target comes from the conditioning image)"""
        if conditional:
            return None
        return ('%s on an unconditional model needs %s=: there is no conditioning image to %s' % (self.noun, self.target_kw, self.target_from))

    def check_target(self, cfg, shape, target):
        pass

    def prepare(self, st, cfg, shape, target, dev):
        pass

    def _check_lr_target(self, factor_name, r, shape, target, what):
        """a target one factor r smaller than the image: r divides the image, the target (where given) is a tensor of that shape"""
        if shape[2] % r or shape[3] % r:
            raise L.Sr3Error('p_sample_loop: %s %s %d does not divide the image (%d x %d)' % (self.name, factor_name, r, shape[2], shape[3]))
        want = (shape[0], shape[1], shape[2] // r, shape[3] // r)
        if target is not None and (not torch.is_tensor(target) or tuple(target.shape) != want):
            raise L.Sr3Error('p_sample_loop: %s must be a %s %s (got %s)'
                             % (self.target_kw, want, what, tuple(getattr(target, 'shape', ())) or type(target).__name__))


class Consistency(Rule):
    name, noun, setter, entry = 'consistency', 'consistency', 'set_consistency', 'sr3_consistent_step'
    keys = ('block', 'strength')
    target_kw = 'consistency_target'
    tiled_lacks = 'has no projection in it'
    forward_runs = 'the forward of a consistent step runs'
    target_from = 'take the block means from'

    def parse(self, spec):
        if not hasattr(spec, 'get') or spec.get('block') is None:
            raise ValueError('consistency: "block" is required (got %r)' % (spec,))
        return spec['block'], spec.get('strength', 1.0)

    def validate(self, diff, block=None, strength=1.0):
        if block is None:
            return None
        if not _is_int(block) or int(block) not in CONSISTENCY_BLOCKS:
            raise ValueError('consistency block must be one of %s (got %r)' % (', '.join(str(b) for b in CONSISTENCY_BLOCKS), block))
        return dict(block=int(block), strength=_number('consistency strength', strength, lambda f: 0.0 < f <= 1.0, 'lie in (0, 1]'))

    def buffers(self, st, cfg, shape, cond_shape, dev):
        r = cfg['block']      # the target block means
        st['ymean'] = torch.zeros((shape[0], shape[1], shape[2] // r, shape[3] // r), device=dev)

    def check_target(self, cfg, shape, target):
        self._check_lr_target('block', cfg['block'], shape, target, 'tensor of block means')

    def prepare(self, st, cfg, shape, target, dev):
        if target is not None:
            st['ymean'].copy_(target)
        else:
            B, Cc, H, W = shape
            L.check(L.load().sr3_block_mean_f32(L.ptr(_first_channels(st, Cc)), B, Cc, H, W, cfg['block'], L.ptr(st['ymean']), _stream(dev)))

    def tail(self, st, cfg, z, tables, c3, hist, forward):
        # the tail with the block-mean projection of x0 in it: counter copy + one kernel
        img = st['img']
        B, Cc, H, W = img.shape
        L.check(L.load().sr3_consistent_step(L.ptr(img), L.ptr(st['eps']), L.ptr(z), L.ptr(st['ymean']), B, Cc, H, W, cfg['block'],
                                             cfg['strength'], *[L.ptr(t) for t in tables], L.ptr(st['step']), 1, L.ptr(c3), L.ptr(hist),
                                             _stream(img.device)))


class Guidance(Rule):
    name, noun, setter, entry = 'guidance', 'guidance', 'set_guidance', 'sr3_guided_step'
    keys = ('scale', 'threshold', 'percentile')
    tiled_lacks = 'combines no second forward'
    forward_runs = 'the forwards of a guided step run'

    def parse(self, spec):
        if not hasattr(spec, 'get'):
            raise ValueError('guidance: a dict of "scale", "threshold", "percentile" is expected (got %r)' % (spec,))
        return spec.get('scale', 1.0), spec.get('threshold', 'static'), spec.get('percentile', 0.995)

    def validate(self, diff, scale=None, threshold=None, percentile=0.995):
        if scale is None and threshold is None:
            return None
        if scale is None:
            scale = 1.0
        if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) or not np.isfinite(float(scale)):
            raise ValueError('guidance scale must be a finite number (got %r)' % (scale,))
        if threshold is None:
            threshold = 'static'
        if threshold not in THRESHOLDS:
            raise ValueError('guidance threshold must be one of %s (got %r)' % (', '.join(repr(k) for k in THRESHOLDS), threshold))
        percentile = _number('guidance percentile', percentile, lambda f: 0.0 <= f <= 1.0, 'lie in [0, 1]') if threshold == 'dynamic' else None
        if not diff.conditional:
            raise ValueError('guidance on an unconditional model: there is no conditioning image to drop')
        return dict(scale=float(scale), threshold=threshold, percentile=percentile)

    def buffers(self, st, cfg, shape, cond_shape, dev):
        """the zero conditioning image and the second forward's output (scale != 1 only), the per-image thresholds, and for the
        dynamic threshold x0 of the whole batch, the select's scratch and the ranks of the percentile"""
        st['thr'] = torch.zeros(shape[0], device=dev)
        st['cond0'] = st['eps_u'] = st['x0'] = st['qscratch'] = None
        st['rank_lo'], st['frac'] = 0, 0.0
        if cfg['scale'] != 1.0:
            st['cond0'] = torch.zeros(cond_shape, device=dev)
            st['eps_u'] = torch.zeros(shape, device=dev)
        if cfg['threshold'] == 'dynamic':
            n = int(shape[1] * shape[2] * shape[3])
            st['rank_lo'], st['frac'] = quantile_rank(n, cfg['percentile'])
            st['x0'] = torch.empty(shape, device=dev)
            st['qscratch'] = torch.empty(int(L.load().sr3_abs_quantile_scratch_bytes(shape[0], n)), dtype=torch.uint8, device=dev)

    def tail(self, st, cfg, z, tables, c3, hist, forward):
        # a second forward on the zero conditioning image unless the scale is 1 -- the same plan, batch and workspace, one after the
        # other; the device counter moves only in the tail's last kernel -- then the two outputs combined, the threshold rule on x0
        # (st['thr'] keeps each image's), the p_sample update and the counter decrement
        if st['eps_u'] is not None:
            forward(st['cond0'], st['eps_u'])
        img, qs = st['img'], st['qscratch']
        B, Cc, H, W = img.shape
        L.check(L.load().sr3_guided_step(L.ptr(img), L.ptr(st['eps']), L.ptr(st['eps_u']), cfg['scale'], L.ptr(z), B, Cc, H, W,
                                         *[L.ptr(t) for t in tables], L.ptr(c3), L.ptr(hist), L.ptr(st['step']),
                                         THRESHOLDS.index(cfg['threshold']), st['rank_lo'], st['frac'], L.ptr(st['x0']), L.ptr(qs),
                                         0 if qs is None else qs.numel(), L.ptr(st['thr']), _stream(img.device)))


class Backprojection(Rule):
    name, noun, setter, entry = 'backprojection', 'back-projection', 'set_backprojection', 'sr3_backproject_step'
    keys = BACKPROJECTION_KEYS
    target_kw = 'backprojection_target'
    tiled_lacks = 'has no back-projection in it'
    forward_runs = 'the forward of a back-projected step runs'
    target_from = 'down-sample'
    # it takes no stream of its own out of the pool for the warm-up, so which pool stream -- and with it which hardware queue -- anything
    # created later in the process gets does not depend on how many such states were captured before
    warm_on_capture_stream = True

    def parse(self, spec):
        if not hasattr(spec, 'get') or not hasattr(spec, 'keys'):
            raise ValueError('backprojection: a dict of "scale", "iterations", "strength", "resample" is expected (got %r)' % (spec,))
        for k in spec.keys():
            if k not in BACKPROJECTION_KEYS:
                raise ValueError('backprojection: unknown key %r (known: %s)' % (k, ', '.join('"%s"' % n for n in BACKPROJECTION_KEYS)))
        if spec.get('scale') is None:
            raise ValueError('backprojection: "scale" is required (got %r)' % (spec,))
        return spec['scale'], spec.get('iterations', 1), spec.get('strength', 1.0), spec.get('resample', 'bicubic')

    def validate(self, diff, scale=None, iterations=1, strength=1.0, resample='bicubic'):
        if scale is None:
            return None
        if not _is_int(scale) or int(scale) < 2:
            raise ValueError('backprojection scale must be an integer >= 2 (got %r)' % (scale,))
        if not _is_int(iterations) or not 1 <= int(iterations) <= 16:
            raise ValueError('backprojection iterations must be an integer in 1..16 (got %r)' % (iterations,))
        lam = _number('backprojection strength', strength, lambda f: 0.0 < f < 2.0, 'lie in (0, 2)')
        if not isinstance(resample, str) or resample not in RESAMPLES:
            raise ValueError('backprojection resample must be one of %s (got %r)' % (', '.join(repr(k) for k in RESAMPLES), resample))
        return dict(scale=int(scale), iterations=int(iterations), strength=lam, resample=resample)

    def buffers(self, st, cfg, shape, cond_shape, dev):
        """the LR target, the four tables of the down-sample and of the up-sample (`resample_tables`) and the step's scratch"""
        B, Cc, H, W = shape
        s = cfg['scale']
        st['y_lr'] = torch.zeros((B, Cc, H // s, W // s), device=dev)
        st['bp_down'] = _resample_device_tables((H, W), (H // s, W // s), cfg['resample'], dev)
        st['bp_up'] = _resample_device_tables((H // s, W // s), (H, W), cfg['resample'], dev)
        st['bp_scratch'] = torch.empty(int(L.load().sr3_backproject_scratch_bytes(B, Cc, H, W, s)), dtype=torch.uint8, device=dev)

    def check_target(self, cfg, shape, target):
        self._check_lr_target('scale', cfg['scale'], shape, target, 'LR image')

    def prepare(self, st, cfg, shape, target, dev):
        if target is None:      # the conditioning image down-sampled once
            target = resample_f32(_first_channels(st, shape[1]), tuple(st['y_lr'].shape[2:]), cfg['resample'], tables=st['bp_down'])
        st['y_lr'].copy_(target)

    def tail(self, st, cfg, z, tables, c3, hist, forward):
        # the tail with the back-projection rounds on x0 in it: counter copy + 1 + 3 K kernels
        img = st['img']
        B, Cc, H, W = img.shape
        axes = []
        for tb in (st['bp_down'], st['bp_up']):
            axes += [L.ptr(tb[0]), L.ptr(tb[1]), tb[1].shape[1], L.ptr(tb[2]), L.ptr(tb[3]), tb[3].shape[1]]
        L.check(L.load().sr3_backproject_step(L.ptr(img), L.ptr(st['eps']), L.ptr(z), L.ptr(st['y_lr']), B, Cc, H, W, cfg['scale'],
                                              cfg['iterations'], cfg['strength'], *axes, *[L.ptr(t) for t in tables], L.ptr(st['step']),
                                              1, L.ptr(c3), L.ptr(hist), L.ptr(st['bp_scratch']), st['bp_scratch'].numel(),
                                              _stream(img.device)))


RESTORE_OPERATORS = ('mask', 'gray')      # the op numbers of sr3_restore_step, in order
RESTORE_KEYS = ('operator', 'strength', 'weights', 'travel')
GRAY_WEIGHTS = {'rec601': (0.299, 0.587, 0.114)}      # (and 'mean': 1 / C each)
GRAY_MAX_CHANNELS = 4                      # sr3_restore_step's weights travel by value


def gray_weights(weights, channels):
    """The channel weights a of the gray operator and their pseudo-inverse p = a / sum a^2 (float64, rounded once) as two fp32 arrays of
    `channels` values: weights 'mean' (1 / channels each), 'rec601' (0.299, 0.587, 0.114; three channels) or a list of `channels`
    finite numbers, not all zero.  Pure NumPy, no device."""
    channels = int(channels)
    if channels > GRAY_MAX_CHANNELS:
        raise ValueError('restore weights: the gray operator takes at most %d channels (got %d)' % (GRAY_MAX_CHANNELS, channels))
    if isinstance(weights, str):
        if weights == 'mean':
            a = np.full(channels, 1.0 / channels, dtype=np.float64)
        elif weights in GRAY_WEIGHTS:
            a = np.asarray(GRAY_WEIGHTS[weights], dtype=np.float64)
        else:
            raise ValueError('restore weights must be \'mean\', %s or a list of numbers (got %r)'
                             % (', '.join(repr(k) for k in GRAY_WEIGHTS), weights))
    else:
        try:
            a = np.asarray([_number('restore weights', v, np.isfinite, 'be finite numbers') for v in weights], dtype=np.float64)
        except TypeError:
            raise ValueError('restore weights must be \'mean\', %s or a list of numbers (got %r)'
                             % (', '.join(repr(k) for k in GRAY_WEIGHTS), weights))
    if a.shape[0] != channels:
        raise ValueError('restore weights: %d weights for %d channels (got %r)' % (a.shape[0], channels, weights))
    a = a.astype(np.float32)                   # the a the kernel multiplies by; p is the pseudo-inverse of THAT a
    n = float((a.astype(np.float64) ** 2).sum())
    if n == 0.0:
        raise ValueError('restore weights must not all be zero (got %r)' % (weights,))
    return a, (a.astype(np.float64) / n).astype(np.float32)


def _floats(v):
    return (C.c_float * len(v))(*[float(f) for f in v])


def gray_f32(x, weights='mean'):
    """dst[b, 0, y, x] = ((a0 x[b, 0] + a1 x[b, 1]) + a2 x[b, 2]) + ... of x [B, C, H, W] (a contiguous fp32 GPU tensor, C <= 4), every
    product and sum rounded on its own (sr3_gray_f32): [B, 1, H, W].  weights: as `gray_weights`."""
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
        raise L.Sr3Error('gray_f32 needs a (B, C, H, W) fp32 GPU tensor; there is no CPU fallback')
    x = x.contiguous()
    B, Cc, H, W = x.shape
    a = weights if isinstance(weights, np.ndarray) else gray_weights(weights, Cc)[0]
    out = torch.empty((B, 1, H, W), device=x.device)
    L.check(L.load().sr3_gray_f32(L.ptr(x), B, Cc, H, W, _floats(a), L.ptr(out), _stream(x.device)))
    return out


def restore_error(sr, cfg, target):
    """How far the result sr [B, C, H, W] is from what a restoring chain was given (cfg: EngineDiffusion.restore).  mask: target =
    (known, mask), max |sr - known| over the pixels whose mask is 1.  gray: target = the gray image [B, 1, H, W] (or a colour image,
    reduced as the chain reduces it), max |gray(sr) - target|.  fp32 GPU tensors."""
    if not torch.is_tensor(sr) or sr.dim() != 4:
        raise L.Sr3Error('restore_error needs a (B, C, H, W) fp32 GPU tensor; there is no CPU fallback')
    if cfg['operator'] == 'mask':
        known, mask = target
        d = (sr - known.to(sr.device, torch.float32)).abs() * (mask.to(sr.device, torch.float32) == 1.0)
        return float(d.max())
    a = np.asarray(cfg['weights'], dtype=np.float32)
    y = target.to(sr.device, torch.float32)
    if y.shape[1] != 1:
        y = gray_f32(y, a)
    return float((gray_f32(sr, a) - y).abs().max())


def travel_walk(S, length, repeats):
    """The resampled walk over the step indices S - 1 .. 0 (RePaint's jumps, DDNM's time travel) as a list of passes (top, n): n steps
    from index top down to top - n + 1.  Segment k covers top_k = S - 1 - k length down to max(top_k - length + 1, 0) and runs
    `repeats` times; between two runs of a segment the chain jumps from the counter below it, top - n, back up to top -- wherever a
    pass does not start where the one before it ended.  S repeats steps in all; length >= S or repeats = 1: the plain walk, one pass
    [(S - 1, S)].  Pure Python."""
    for name, v in (('S', S), ('length', length), ('repeats', repeats)):
        if not _is_int(v) or int(v) < 1:
            raise ValueError('travel_walk: %s must be a positive integer (got %r)' % (name, v))
    S, length, repeats = int(S), int(length), int(repeats)
    if repeats == 1 or length >= S:
        return [(S - 1, S)]
    walk = []
    for top in range(S - 1, -1, -length):
        n = top - max(top - length + 1, 0) + 1
        walk += [(top, n)] * repeats
    return walk


def walk_jumps(walk):
    """the jumps of a `travel_walk`: [(c, to)] -- from the counter c the pass before ended at to the next pass's top, to > c"""
    return [(a[0] - a[1], b[0]) for a, b in zip(walk[:-1], walk[1:]) if b[0] != a[0] - a[1]]


def travel_tables(walk, abar, rows=None):
    """The three tables of sr3_travel_back_f32 for a `travel_walk`, indexed by r = c + 1 (c = the counter on entry, -1 .. rows - 2):
    ra[r] = sqrt(abar(to) / abar(c)), rs[r] = sqrt(1 - abar(to) / abar(c)) in float64, rounded once, and to[r]; abar: alphas_cumprod
    of the rule's step indices (float64 [S]), abar(-1) = 1.  A row without a jump holds ra = 1, rs = 0, to = c.  -> (ra fp32, rs fp32,
    to int32), `rows` (default S) entries each."""
    abar = np.asarray(abar, dtype=np.float64)
    rows = int(abar.shape[0]) if rows is None else int(rows)
    ra64, rs64 = np.ones(rows, dtype=np.float64), np.zeros(rows, dtype=np.float64)
    to = np.arange(-1, rows - 1, dtype=np.int32)
    ab = lambda c: 1.0 if c < 0 else abar[c]
    for c, t in walk_jumps(walk):
        if not -1 <= c < t <= rows - 1 or t >= abar.shape[0]:
            raise ValueError('travel_tables: a jump from counter %d to %d does not fit %d rows' % (c, t, rows))
        q = ab(t) / ab(c)
        ra64[c + 1], rs64[c + 1], to[c + 1] = np.sqrt(q), np.sqrt(1.0 - q), t
    return ra64.astype(np.float32), rs64.astype(np.float32), to


class Restore(Rule):
    name, noun, setter, entry = 'restore', 'restore', 'set_restore', 'sr3_restore_step'
    keys = RESTORE_KEYS
    target_kw = 'restore_target'
    tiled_lacks = 'has no mask or gray projection in it'
    forward_runs = 'the forward of a restoring step runs'
    target_from = 'take the gray image from'
    takes_t_map = True                # its forward is sr3_unet_forward_full, which reads the sampler's walk: the DDPM variant under a sampler runs
    key_appended = True

    def parse(self, spec):
        if not hasattr(spec, 'get') or not hasattr(spec, 'keys'):
            raise ValueError('restore: a dict of "operator", "strength", "weights", "travel" is expected (got %r)' % (spec,))
        for k in spec.keys():
            if k not in RESTORE_KEYS:
                raise ValueError('restore: unknown key %r (known: %s)' % (k, ', '.join('"%s"' % n for n in RESTORE_KEYS)))
        if spec.get('operator') is None:
            raise ValueError('restore: "operator" is required (got %r)' % (spec,))
        return spec['operator'], spec.get('strength', 1.0), spec.get('weights', 'mean'), spec.get('travel')

    def validate(self, diff, operator=None, strength=1.0, weights='mean', travel=None):
        if operator is None:
            return None
        if not isinstance(operator, str) or operator not in RESTORE_OPERATORS:
            raise ValueError('restore operator must be one of %s (got %r)' % (', '.join(repr(k) for k in RESTORE_OPERATORS), operator))
        lam = _number('restore strength', strength, lambda f: 0.0 < f <= 1.0, 'lie in (0, 1]')
        a = p = None
        if operator == 'gray':
            a, p = (tuple(float(v) for v in t) for t in gray_weights(weights, diff.channels))
        elif weights != 'mean':
            raise ValueError('restore weights are given (%r) but the operator is \'mask\', not \'gray\'' % (weights,))
        if travel is not None:
            if not hasattr(travel, 'get') or not hasattr(travel, 'keys') or set(travel.keys()) - {'length', 'repeats'}:
                raise ValueError('restore travel: a dict of "length" and "repeats" is expected (got %r)' % (travel,))
            tl, tr = travel.get('length', 1), travel.get('repeats', 1)
            if not _is_int(tl) or int(tl) < 1:
                raise ValueError('restore travel length must be a positive integer (got %r)' % (tl,))
            if not _is_int(tr) or not 1 <= int(tr) <= 64:
                raise ValueError('restore travel repeats must be an integer in 1..64 (got %r)' % (tr,))
            travel = None if int(tr) == 1 else (int(tl), int(tr))      # one run of every segment is the plain walk
        return dict(operator=operator, strength=lam, weights=a, pinv=p, travel=travel)

    def key(self, cfg):
        return None if cfg is None else ('restore',) + tuple(cfg[k] for k in self.keys)

    def missing_target(self, cfg, conditional):
        if cfg['operator'] == 'mask':
            return ('restore with the mask operator needs restore_target=(known, mask): the known image [B, C, H, W] and the mask '
                    '[B, 1 or C, H, W], 1 = known; there is no default')
        return Rule.missing_target(self, cfg, conditional)

    def buffers(self, st, cfg, shape, cond_shape, dev):
        """mask: the known image and the mask (one allocation of C planes, of which a one-plane mask uses the first B H W values);
        gray: the gray target and the weights as the entry takes them"""
        B, Cc, H, W = shape
        st['replays'] = 0                       # graph replays of the chain (the travelled walk's S repeats)
        if cfg['operator'] == 'mask':
            st['rs_known'] = torch.zeros(shape, device=dev)
            st['rs_maskbuf'] = torch.zeros(shape, device=dev)
            st['rs_mc'] = None                  # the mask's channel count the graph was captured with
        else:
            st['rs_gray'] = torch.zeros((B, 1, H, W), device=dev)
            st['rs_a'], st['rs_p'] = _floats(cfg['weights']), _floats(cfg['pinv'])

    def check_target(self, cfg, shape, target):
        B, Cc, H, W = shape
        got = lambda t: tuple(getattr(t, 'shape', ())) or type(t).__name__
        if cfg['operator'] == 'mask':
            if not isinstance(target, (tuple, list)) or len(target) != 2 or not all(torch.is_tensor(t) for t in target):
                raise L.Sr3Error('p_sample_loop: restore_target must be the pair (known, mask) of tensors (got %s)' % type(target).__name__)
            known, mask = target
            if tuple(known.shape) != tuple(shape):
                raise L.Sr3Error('p_sample_loop: restore_target[0] must be a %s known image (got %s)' % (tuple(shape), got(known)))
            if tuple(mask.shape) not in ((B, 1, H, W), (B, Cc, H, W)):
                raise L.Sr3Error('p_sample_loop: restore_target[1] must be a %s or %s mask (got %s)' % ((B, 1, H, W), (B, Cc, H, W), got(mask)))
        else:
            if Cc > GRAY_MAX_CHANNELS or len(cfg['weights']) != Cc:
                raise L.Sr3Error('p_sample_loop: the gray operator was set for %d channels; the image has %d' % (len(cfg['weights']), Cc))
            if target is not None and (not torch.is_tensor(target) or tuple(target.shape) not in ((B, 1, H, W), (B, Cc, H, W))):
                raise L.Sr3Error('p_sample_loop: restore_target must be a %s gray image or a %s colour image (got %s)'
                                 % ((B, 1, H, W), (B, Cc, H, W), got(target)))

    def prepare(self, st, cfg, shape, target, dev):
        B, Cc, H, W = shape
        st['replays'] = 0
        if cfg['operator'] == 'mask':
            known, mask = target
            st['rs_known'].copy_(known)
            mc = int(mask.shape[1])
            if st['rs_mc'] != mc:               # the entry's mask_channels is baked into a captured graph
                st['rs_mc'], st['graph'] = mc, None
            st['rs_mask'] = st['rs_maskbuf'].view(-1)[:B * mc * H * W].view(B, mc, H, W)
            st['rs_mask'].copy_(mask)
            return
        a = np.asarray(cfg['weights'], dtype=np.float32)
        if target is None:
            target = _first_channels(st, Cc)
        target = target.to(dev, torch.float32)
        st['rs_gray'].copy_(target if target.shape[1] == 1 else gray_f32(target, a))

    def tail(self, st, cfg, z, tables, c3, hist, forward):
        # the tail with the mask / gray projection of x0 in it: counter copy + one kernel
        img = st['img']
        B, Cc, H, W = img.shape
        if cfg['operator'] == 'mask':
            op_args = (0, L.ptr(st['rs_known']), L.ptr(st['rs_mask']), st['rs_mc'], None, None)
        else:
            op_args = (1, L.ptr(st['rs_gray']), None, 0, st['rs_a'], st['rs_p'])
        L.check(L.load().sr3_restore_step(L.ptr(img), L.ptr(st['eps']), L.ptr(z), *op_args, B, Cc, H, W, cfg['strength'],
                                          *[L.ptr(t) for t in tables], L.ptr(st['step']), 1, L.ptr(c3), L.ptr(hist), _stream(img.device)))

    def travel_state(self, st, cfg, S, abar, dev):
        """the passes of the travelled walk and its device tables, made once per state"""
        if st.get('rs_walk') is None:
            walk = travel_walk(S, *cfg['travel'])
            st['rs_walk'] = walk
            st['rs_travel'] = tuple(torch.from_numpy(t).to(dev) for t in travel_tables(walk, abar, S))
        return st['rs_walk']

    def jump(self, st, S):
        """x <- ra x + rs z at the counter's row, the counter up to the row's target (sr3_travel_back_f32); z is st['z'], drawn by the caller"""
        img = st['img']
        ra, rs, to = st['rs_travel']
        L.check(L.load().sr3_travel_back_f32(L.ptr(img), L.ptr(st['z']), L.ptr(ra), L.ptr(rs), L.ptr(to), int(S), L.ptr(st['step']),
                                             img.shape[0], img[0].numel(), _stream(img.device)))


CONSISTENCY, GUIDANCE, BACKPROJECTION, RESTORE = RULES = (Consistency(), Guidance(), Backprojection(), Restore())
# ^ the order of parsing, of the checks and (reversed, for the rules whose key is not appended) of the loop-state key


def check_rule(rule, cfgs, sampler_on_ddpm, tiling):
    """NotImplementedError where `rule`'s setting in cfgs (name -> setting or None) does not go with tiling, with an earlier rule of the
    table that is on, or with a sampler on the DDPM variant"""
    if cfgs.get(rule.name) is None:
        return
    off = 'switch %s off (%s(None))' % (rule.noun, rule.setter)
    if tiling is not None:
        raise NotImplementedError('%s with tiling: sr3_tiled_step owns the tail of a tiled step and %s; use whole-image steps '
                                  '(set_tiling(None)) or %s' % (rule.noun, rule.tiled_lacks, off))
    for other in RULES[:RULES.index(rule)]:
        if cfgs.get(other.name) is not None:
            raise NotImplementedError('%s with %s: %s and %s each own the whole tail of a step; switch one of them off (%s(None) / %s(None))'
                                      % (rule.noun, other.noun, rule.entry, other.entry, rule.setter, other.setter))
    if sampler_on_ddpm and not rule.takes_t_map:
        raise NotImplementedError('%s of the DDPM variant under a sampler (DDIM, DPM-Solver++): %s through sr3_unet_forward, which has no '
                                  'step-index -> timestep map (t_map); use the ancestral sampler (set_sampler(None)) or %s'
                                  % (rule.noun, rule.forward_runs, off))
