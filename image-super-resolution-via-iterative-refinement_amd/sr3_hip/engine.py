"""Host-side handle of one UNet plan: parameter arena packing and the forward call.

The compute is entirely inside libsr3_mi355x.so; torch supplies device memory, the current
stream and tensor views -- nothing else.
"""
import ctypes as C
import math

import torch

from . import lib as L


def make_desc(variant, in_channel, out_channel, inner_channel, norm_groups, channel_mults, attn_res,
              res_blocks, image_size):
    d = L.UnetDesc()
    d.variant = {'sr3': 0, 'ddpm': 1}[variant]
    d.in_channel = int(in_channel)
    d.out_channel = int(out_channel if out_channel is not None else in_channel)
    d.inner_channel = int(inner_channel)
    d.norm_groups = int(norm_groups)
    mults = list(channel_mults)
    attn = [attn_res] if isinstance(attn_res, int) else list(attn_res)
    if len(mults) > 8 or len(attn) > 8:
        raise L.Sr3Error('at most 8 channel multipliers / attention resolutions')
    d.n_mults = len(mults)
    for i, m in enumerate(mults):
        d.channel_mults[i] = int(m)
    d.n_attn_res = len(attn)
    for i, a in enumerate(attn):
        d.attn_res[i] = int(a)
    d.res_blocks = int(res_blocks)
    d.image_size = int(image_size)
    return d


class Plan(object):
    """Owns an sr3_plan*; exposes the parameter table."""

    def __init__(self, variant, in_channel, out_channel, inner_channel, norm_groups, channel_mults, attn_res,
                 res_blocks, image_size, scale_shift_norm=False):
        self.lib = L.load()
        self.variant = variant
        self.inner = int(inner_channel)
        self.in_channel = int(in_channel)
        self.out_channel = int(out_channel if out_channel is not None else in_channel)
        self.image_size = int(image_size)
        self.var_channels = 0      # plan option var_channels: the last rows of the output conv that are a learned-variance head
        self.desc = make_desc(variant, in_channel, out_channel, inner_channel, norm_groups, channel_mults,
                              attn_res, res_blocks, image_size)
        # scale-shift time conditioning (SR3_UNET_SCALE_SHIFT_NORM): a res block's projection has 2 Cout rows, (scale, shift) of its second
        # GroupNorm -- GN2(h) (1 + scale) + shift -- in place of a row added to conv1's output
        self.scale_shift_norm = bool(scale_shift_norm)
        h = C.c_void_p()
        if self.scale_shift_norm:
            L.check(self.lib.sr3_plan_create_ex(C.byref(self.desc), L.UNET_SCALE_SHIFT_NORM, C.byref(h)))
        else:
            L.check(self.lib.sr3_plan_create(C.byref(self.desc), C.byref(h)))
        self.handle = h
        self.options = {}          # plan options set through set_option (key -> value)
        self._own_cache = None     # plan option feat_cache: the feature cache of the forwards that are handed none (own_feature_cache)
        self.generation = 0        # identifies the launch list: changes with every set_option and with the geometry -- part of the
                                   # reverse-loop graph cache key.  A geometry seen before (under the same options) gets its old value back
        self.options_epoch = 0     # bumped by set_option only: what the derived filters depend on (the geometry does not touch them)
        self.divisor = 1 << (len(list(channel_mults)) - 1)
        self.geometry = (self.image_size, self.image_size)
        self._next_generation = 1
        self._geometry_generation = {self.geometry: 0}
        self.param_floats = int(self.lib.sr3_plan_param_floats(h))
        self.table = []
        pi = L.ParamInfo()
        for i in range(self.lib.sr3_plan_num_params(h)):
            L.check(self.lib.sr3_plan_param_info(h, i, C.byref(pi)))
            self.table.append(dict(name=pi.name.decode(), shape=tuple(pi.shape[:pi.ndim]), pack=int(pi.pack),
                                   offset=int(pi.offset), numel=int(pi.numel)))

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                self.lib.sr3_plan_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def set_option(self, key, value):
        if key == 'feat_cache':        # (a plan option with an entry of its own: the depth of the shallow forward, 0 = off)
            rc = self.lib.sr3_plan_set_feature_cache(self.handle, int(value))
        else:
            rc = self.lib.sr3_plan_set_option(self.handle, key.encode(), int(value))
        if rc < 0:
            L.check(rc)
        self.options[key] = int(value)
        if key == 'var_channels':
            self.var_channels = int(value)
        # anything compiled / captured against the previous options is stale, at every geometry
        self.generation = self._next_generation
        self._next_generation += 1
        self._geometry_generation = {self.geometry: self.generation}
        self.options_epoch += 1
        return rc

    def set_geometry(self, height, width):
        """Height and width of the images the next forward / reverse step / workspace query works on (sr3_plan_set_geometry);
        (0, 0) restores image_size x image_size.  Host only."""
        height, width = int(height), int(width)
        if (height, width) == (0, 0):
            height = width = self.image_size
        if (height, width) == self.geometry:
            return
        if height <= 0 or width <= 0 or height % self.divisor or width % self.divisor:
            raise L.Sr3Error('image size %d x %d: height and width must be positive multiples of %d (the UNet halves the image %d times)'
                             % (height, width, self.divisor, self.desc.n_mults - 1))
        L.check(self.lib.sr3_plan_set_geometry(self.handle, height, width))
        self.geometry = (height, width)
        gen = self._geometry_generation.get(self.geometry)
        if gen is None:
            gen = self._geometry_generation[self.geometry] = self._next_generation
            self._next_generation += 1
        self.generation = gen

    @property
    def image_channels(self):
        """Channels of x, z and eps of a step: out_channel without the variance head."""
        return self.out_channel - self.var_channels

    def workspace_bytes(self, batch):
        n = int(self.lib.sr3_workspace_bytes(self.handle, int(batch)))
        if n == 0:
            raise L.Sr3Error('sr3_workspace_bytes failed: %s' % L.hint((self.lib.sr3_last_error() or b'').decode()))
        return n

    def feature_cache_bytes(self, batch):
        """Bytes of the feature cache for `batch` images at the plan's geometry (sr3_feature_cache_bytes); 0 without plan option feat_cache."""
        return int(self.lib.sr3_feature_cache_bytes(self.handle, int(batch)))

    def new_feature_cache(self, batch, device):
        """A 256-byte aligned uint8 tensor of feature_cache_bytes(batch) on `device`, or None without plan option feat_cache."""
        need = self.feature_cache_bytes(batch)
        if need == 0:
            return None
        buf = torch.empty(need + 256, dtype=torch.uint8, device=device)
        off = (-buf.data_ptr()) % 256
        return buf[off:off + need]

    def own_feature_cache(self, batch, device):
        """Under plan option feat_cache every forward writes the branch tensor somewhere: the cache of the calls that bring none of their
        own (a plain forward, p_sample) -- never one a sampling loop's cached steps read."""
        need = self.feature_cache_bytes(batch)
        c = self._own_cache
        if c is None or c.numel() < need or c.device != device:
            c = self._own_cache = self.new_feature_cache(batch, device)
        return c

    def shallow_op_list(self, batch):
        """The launch list of a cached forward (plan option feat_cache; sr3_plan_op_info_cached), as op_list's entries.  Host only."""
        n = int(self.lib.sr3_plan_num_ops_cached(self.handle, int(batch)))
        if n < 0:
            raise L.Sr3Error('sr3_plan_num_ops_cached failed: %s' % (self.lib.sr3_last_error() or b'').decode())
        info = L.OpInfo()
        out = []
        for i in range(n):
            L.check(self.lib.sr3_plan_op_info_cached(self.handle, int(batch), i, C.byref(info)))
            out.append({k: getattr(info, k) for k, _ in L.OpInfo._fields_})
        return out

    def forward_flops(self, batch):
        return float(self.lib.sr3_plan_forward_flops(self.handle, int(batch)))

    def num_ops(self, batch):
        return int(self.lib.sr3_plan_num_ops(self.handle, int(batch)))

    def op_list(self, batch):
        """The ordered launch list of one forward at this batch size (host-only inspection)."""
        info = L.OpInfo()
        side, wait = C.c_int(), C.c_int()
        out = []
        for i in range(self.num_ops(batch)):
            L.check(self.lib.sr3_plan_op_info(self.handle, int(batch), i, C.byref(info)))
            o = {k: getattr(info, k) for k, _ in L.OpInfo._fields_}
            L.check(self.lib.sr3_plan_op_side(self.handle, int(batch), i, C.byref(side), C.byref(wait)))
            if side.value >= 0 or wait.value >= 0:      # plan option fork_side: ops on the side stream / the consumers that join them
                o['side_id'], o['wait_id'] = side.value, wait.value
            out.append(o)
        return out

    def fold_list(self, batch):
        """Per op of op_list(batch): (fold, mod_row) of sr3_plan_op_fold -- fold 0 none, 1 a fold launch, 2 the tail of this split-K conv's
        reduce, 3 the tail of this statistics pass; mod_row >= 0: the FiLM-table rows that modulate the pairs (scale_shift_norm), else -1."""
        fold, row = C.c_int(), C.c_int()
        out = []
        for i in range(self.num_ops(batch)):
            L.check(self.lib.sr3_plan_op_fold(self.handle, int(batch), i, C.byref(fold), C.byref(row)))
            out.append((fold.value, row.value))
        return out

    def taps(self):
        out = []
        name = C.create_string_buffer(64)
        off = C.c_size_t()
        c, h, w = C.c_int(), C.c_int(), C.c_int()
        for i in range(self.lib.sr3_plan_num_taps(self.handle)):
            L.check(self.lib.sr3_plan_tap_info(self.handle, i, name, 64, C.byref(off), C.byref(c), C.byref(h), C.byref(w)))
            out.append((name.value.decode(), int(off.value), c.value, h.value, w.value))
        return out

    # ---- arena <-> reference state-dict views ---------------------------------------------
    def view(self, arena, entry):
        """A view of `arena` with the reference shape (OIHW for convs) -- writes go through."""
        flat = arena[entry['offset']:entry['offset'] + entry['numel']]
        shape = entry['shape']
        if entry['pack'] == 1:
            o, i, kh, kw = shape
            return flat.view(o, kh, kw, i).permute(0, 3, 1, 2)
        return flat.view(*shape)

    def default_freq(self):
        """Frequency table of PositionalEncoding (sr3 unet.py:24-28) / TimeEmbedding.inv_freq
        (ddpm unet.py:23-26), computed with the same fp32 torch expressions as the reference."""
        dim = self.inner
        if self.variant == 'sr3':
            count = dim // 2
            step = torch.arange(count, dtype=torch.float32) / count
            return torch.exp(-math.log(1e4) * step)
        return torch.exp(torch.arange(0, dim, 2, dtype=torch.float32) * (-math.log(10000) / dim))


class Workspace(object):
    """Per-(device, batch) scratch owned by torch's caching allocator (graph-capture friendly)."""

    def __init__(self):
        self.buf = None
        self.batch = None

    def get(self, plan, batch, device):
        need = plan.workspace_bytes(batch)
        if self.buf is None or self.buf.numel() < need or self.buf.device != device:
            self.buf = torch.empty(need + 256, dtype=torch.uint8, device=device)
        self.batch = batch
        off = (-self.buf.data_ptr()) % 256
        return self.buf[off:off + need], need


def _check_same_size(x, cond):
    if cond is not None and (cond.dim() != 4 or cond.shape[0] != x.shape[0] or tuple(cond.shape[2:]) != tuple(x.shape[2:])):
        raise L.Sr3Error('conditioning image %s and input %s differ in batch or size' % (tuple(cond.shape), tuple(x.shape)))


def _feature_cache(plan, feat_cache, refresh, batch, device):
    """The cache a forward runs with: none on a plan without option feat_cache (a cached step is refused there); else the caller's, or --
    a refresh only -- the plan's own."""
    if not plan.options.get('feat_cache'):
        if not refresh:
            raise L.Sr3Error('a cached step (refresh=False) needs plan option feat_cache')
        return None
    if feat_cache is None:
        if not refresh:
            raise L.Sr3Error('a cached step (refresh=False) needs the feature cache the refresh filled')
        return plan.own_feature_cache(batch, device)
    if feat_cache.dtype != torch.uint8 or not feat_cache.is_contiguous() or feat_cache.device != device:
        raise L.Sr3Error('feat_cache must be a contiguous uint8 tensor on the device of x (Plan.new_feature_cache)')
    return feat_cache


def reverse_step(plan, arena, freq, ws, x, z, tables, step2, cond=None, level_table=None, clip_denoised=True, eps_out=None,
                 t_map=None, c3=None, hist=None, feat_cache=None, refresh=True):
    """One whole reverse step in place on `x` (sr3_reverse_step_hist): eps = UNet(cat([cond, x], 1), level(t)); x <- p_sample update;
    t <- t - 1, with t = step2[1] (int32 tensor of two).  `tables` = (a, b, c1, c2, sigma) schedule tables on the device, indexed
    by t like `level_table`.  `z` None: no noise is read (= 0).  `t_map` (int32 device tensor, one entry per value t takes): the
    timestep the DDPM UNet is conditioned on at counter value t -- a sampler's walk through a subset of the timesteps; None: t.
    `c3`, `hist` (both or neither): a multistep sampler's table of the previous x0's coefficient and the buffer, shaped like `x`, that
    carries that x0 from step to step (x <- ... + c3[t] hist; hist <- this step's x0).  Plan option feat_cache
    (sr3_reverse_step_cached): `feat_cache` (Plan.new_feature_cache) is written by a step with refresh=True, the full forward, and read
    by one with refresh=False, the shallow forward; None: the plan's own cache, full steps only."""
    if not x.is_cuda or not x.is_contiguous() or x.dtype != torch.float32:
        raise L.Sr3Error('reverse_step needs a contiguous fp32 GPU tensor (got %s, %s); there is no CPU fallback' % (x.device, x.dtype))
    B = x.shape[0]
    cc = 0
    if cond is not None:
        cond = cond.contiguous()
        cc = cond.shape[1]
    if x.dim() != 4 or x.shape[1] + cc != plan.in_channel or x.shape[1] != plan.image_channels:
        raise L.Sr3Error('input shape %s (+%d cond channels) does not match the plan (in_channel %d, out_channel %d)'
                         % (tuple(x.shape), cc, plan.in_channel, plan.image_channels))
    _check_same_size(x, cond)
    plan.set_geometry(x.shape[2], x.shape[3])
    if step2.dtype != torch.int32 or step2.numel() != 2 or step2.device != x.device:
        raise L.Sr3Error('step2 must be two int32 on the device of x')
    wsbuf, need = ws.get(plan, B, x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    a, b, c1, c2, sg = tables
    if t_map is not None and (t_map.dtype != torch.int32 or not t_map.is_contiguous() or t_map.device != x.device):
        raise L.Sr3Error('t_map must be a contiguous int32 tensor on the device of x')
    if hist is not None and (hist.dtype != torch.float32 or not hist.is_contiguous() or hist.device != x.device or hist.shape != x.shape):
        raise L.Sr3Error('hist must be a contiguous fp32 tensor of the shape and on the device of x')
    args = (plan.handle, L.ptr(x), L.ptr(cond), cc, L.ptr(freq), L.ptr(level_table), L.ptr(step2), L.ptr(arena), L.ptr(wsbuf), need,
            L.ptr(z), L.ptr(a), L.ptr(b), L.ptr(c1), L.ptr(c2), L.ptr(sg), 1 if clip_denoised else 0, L.ptr(eps_out), B, C.c_void_p(stream),
            L.ptr(t_map), L.ptr(c3), L.ptr(hist))
    cache = _feature_cache(plan, feat_cache, refresh, B, x.device)
    if cache is None:
        L.check(plan.lib.sr3_reverse_step_hist(*args))
    else:
        L.check(plan.lib.sr3_reverse_step_cached(*args, L.ptr(cache), cache.numel(), 1 if refresh else 0))
    return x


def unet_forward(plan, arena, freq, ws, x, cond=None, noise_level=None, timestep=None, level_table=None,
                 step_dev=None, out=None, full=False, t_map=None, feat_cache=None, refresh=True):
    """eps = UNet(cat([cond, x], 1), level)   (all tensors on the GPU, fp32, NCHW contiguous).  `full` (a plan with a variance head,
    option var_channels): all out_channel rows -- the prediction, then the variance head (sr3_unet_forward_full); otherwise the
    prediction rows alone.  `t_map` (with `full` and step_dev, DDPM variant): the timestep is t_map[*step_dev].  `feat_cache`,
    `refresh`: as reverse_step's (sr3_unet_forward_cached; on a plan without a variance head its rows are sr3_unet_forward's)."""
    if not x.is_cuda:
        raise L.Sr3Error('the MI355X engine only runs on a GPU tensor (got %s); there is no CPU fallback' % x.device)
    B = x.shape[0]
    x = x.contiguous()
    cc = 0
    if cond is not None:
        cond = cond.contiguous()
        cc = cond.shape[1]
    if x.dtype != torch.float32 or (cond is not None and cond.dtype != torch.float32):
        raise L.Sr3Error('fp32 tensors expected')
    if x.dim() != 4 or x.shape[1] + cc != plan.in_channel:
        raise L.Sr3Error('input shape %s (+%d cond channels) does not match the plan (in_channel %d)'
                         % (tuple(x.shape), cc, plan.in_channel))
    _check_same_size(x, cond)
    plan.set_geometry(x.shape[2], x.shape[3])
    if noise_level is not None:
        noise_level = noise_level.reshape(-1).contiguous().float()
        if noise_level.numel() != B:
            raise L.Sr3Error('noise_level must have one value per sample')
    if timestep is not None:
        timestep = timestep.reshape(-1).contiguous().long()
        if timestep.numel() != B:
            raise L.Sr3Error('timestep must have one value per sample')
    wsbuf, need = ws.get(plan, B, x.device)
    rows = plan.out_channel if full else plan.image_channels
    if out is None:
        out = torch.empty(B, rows, x.shape[2], x.shape[3], device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != (B, rows, x.shape[2], x.shape[3]) or not out.is_contiguous():
        raise L.Sr3Error('out must be a contiguous %s tensor (got %s)' % ((B, rows, x.shape[2], x.shape[3]), tuple(out.shape)))
    stream = torch.cuda.current_stream(x.device).cuda_stream
    if t_map is not None and (not full or t_map.dtype != torch.int32 or not t_map.is_contiguous() or t_map.device != x.device):
        raise L.Sr3Error('t_map goes with full=True and must be a contiguous int32 tensor on the device of x')
    cache = _feature_cache(plan, feat_cache, refresh, B, x.device)
    if cache is not None:
        if not full and plan.var_channels:
            raise L.Sr3Error('plan option feat_cache on a learned-variance plan: the forward takes full=True (sr3_unet_forward_cached stores every row)')
        L.check(plan.lib.sr3_unet_forward_cached(plan.handle, L.ptr(x), L.ptr(cond), cc, L.ptr(noise_level), L.ptr(timestep),
                                                 L.ptr(freq), L.ptr(level_table), L.ptr(step_dev), L.ptr(arena), L.ptr(wsbuf),
                                                 need, L.ptr(out), B, C.c_void_p(stream), L.ptr(t_map), L.ptr(cache), cache.numel(),
                                                 1 if refresh else 0))
        return out
    if full:
        L.check(plan.lib.sr3_unet_forward_full(plan.handle, L.ptr(x), L.ptr(cond), cc, L.ptr(noise_level), L.ptr(timestep),
                                               L.ptr(freq), L.ptr(level_table), L.ptr(step_dev), L.ptr(arena), L.ptr(wsbuf),
                                               need, L.ptr(out), B, C.c_void_p(stream), L.ptr(t_map)))
        return out
    L.check(plan.lib.sr3_unet_forward(plan.handle, L.ptr(x), L.ptr(cond), cc, L.ptr(noise_level), L.ptr(timestep),
                                      L.ptr(freq), L.ptr(level_table), L.ptr(step_dev), L.ptr(arena), L.ptr(wsbuf),
                                      need, L.ptr(out), B, C.c_void_p(stream)))
    return out
