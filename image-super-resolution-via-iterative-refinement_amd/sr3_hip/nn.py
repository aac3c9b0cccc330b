"""nn.Module faces of the engine: the objects `define_G` hands to the reference's callers.

`EngineUNet` is what `GaussianDiffusion.denoise_fn` is in the reference
(model/sr3_modules/unet.py:161-259, model/ddpm_modules/unet.py:147-243): same constructor
arguments, same `forward(x, time)`, same state-dict keys and shapes -- but it owns one packed
parameter arena and every FLOP runs in libsr3_mi355x.so.
"""
import contextlib
import math
from collections import OrderedDict

import torch
from torch import nn

from . import engine as E
from . import lib as L


def _is_norm(name):
    return '.block.0.' in name or '.norm.' in name


class EngineUNet(nn.Module):
    variant = 'sr3'

    def __init__(self, in_channel=6, out_channel=3, inner_channel=32, norm_groups=32,
                 channel_mults=(1, 2, 4, 8, 8), attn_res=(8), res_blocks=3, dropout=0,
                 with_noise_level_emb=True, image_size=128, *, long_attention=False, learned_variance=False, n_head=1, head_dim=None,
                 scale_shift_norm=False, use_affine_level=False):
        super().__init__()
        if use_affine_level:
            raise NotImplementedError('use_affine_level=True (an affine of conv1\'s output in front of the second GroupNorm) is not built; '
                                      'scale_shift_norm=True (config key model.unet.scale_shift_norm) modulates the second GroupNorm instead')
        if not isinstance(scale_shift_norm, bool):
            raise ValueError('scale_shift_norm must be true or false (got %r)' % (scale_shift_norm,))
        if not with_noise_level_emb:
            raise NotImplementedError('the engine always conditions on the noise level / timestep '
                                      '(define_G never disables it: model/networks.py:91-101)')
        # config key model.unet.scale_shift_norm (plan flag SR3_UNET_SCALE_SHIFT_NORM; ADM's use_scale_shift_norm): the time / noise embedding
        # enters a res block as (scale, shift) of its second GroupNorm, GN2(h) (1 + scale) + shift, not as a row added to conv1's output.
        # The projection's keys keep their names, their shapes become [2 Cout, inner] / [2 Cout]: a checkpoint of the other form fails
        # to load on the shape, with the key named
        self.scale_shift_norm = scale_shift_norm
        self.plan = E.Plan(self.variant, in_channel, out_channel, inner_channel, norm_groups, channel_mults,
                           attn_res, res_blocks, image_size, scale_shift_norm=scale_shift_norm)
        # config key model.unet.long_attention (plan option attn_long): attention levels with more tokens than the score-strip
        # kernels hold in LDS run on the key-blocked kernel instead of refusing the image size
        self.long_attention = bool(long_attention)
        if self.long_attention:
            self.plan.set_option('attn_long', 1)
        # config keys model.unet.n_head / model.unet.head_dim (plan options attn_heads / attn_head_dim): multi-head SelfAttention, n_head
        # heads at every attention level or heads of head_dim channels each.  The weights keep their shapes: the head count is the
        # config's to carry, no checkpoint records it.  A value a level cannot take is refused by the library, in its words
        if head_dim is not None and int(n_head) != 1:
            raise ValueError('n_head (%d) and head_dim (%d) are mutually exclusive: set one' % (int(n_head), int(head_dim)))
        self.n_head, self.head_dim = int(n_head), (None if head_dim is None else int(head_dim))
        if self.head_dim is not None:
            if self.head_dim < 1:
                raise ValueError('head_dim must be a positive channel count (got %d)' % self.head_dim)
            self.plan.set_option('attn_head_dim', self.head_dim)
        elif self.n_head != 1:
            self.plan.set_option('attn_heads', self.n_head)
        # config key model.diffusion.learned_variance (plan option var_channels): the second half of the out_channel rows is the variance
        # head.  Without it a plan with more than 4 output rows builds no launch list: refused here, by the library, in its words
        self.learned_variance = bool(learned_variance)
        if self.learned_variance:
            if self.plan.out_channel % 2:
                raise ValueError('learned_variance needs an even out_channel (got %d)' % self.plan.out_channel)
            self.plan.set_option('var_channels', self.plan.out_channel // 2)
        elif self.plan.out_channel > 4:
            L.check(self.plan.lib.sr3_plan_op_info(self.plan.handle, 1, 0, L.OpInfo()))
        self.dropout = float(dropout)
        self.arena = nn.Parameter(torch.zeros(self.plan.param_floats, dtype=torch.float32), requires_grad=False)
        self.register_buffer('freq', self.plan.default_freq(), persistent=False)
        self._ws = E.Workspace()
        # derived weights (Winograd-transformed 3x3 filters): engine-owned device buffer, never part of a state dict;
        # rebuilt whenever the arena content, its storage or the plan options changed
        self._derived = None
        self._derived_key = None
        self._weights_epoch = 0
        # exponential moving average of the weights (config train.ema_scheduler.enabled): a second arena-shaped tensor, allocated by
        # enable_ema() only.  Neither a parameter nor a buffer: it is in no state dict and no parameter count; it has its own export
        # (ema_state_dict).  Its address never changes (captured reverse loops bake it in); `use_weights` selects which arena runs
        self.ema_arena = None
        self._use_ema = False
        # config train.optimizer.accumulate (set by EngineAdam): micro-batches per optimizer step; train_step scales its gradients by 1 / K
        self.accumulate = 1
        self.reset_parameters()

    # ---- initialisation: same distributions AND same RNG consumption order as the reference ----
    def reset_parameters(self):
        """PyTorch default init of Conv2d / Linear / GroupNorm, drawn in the reference's module
        construction order so a given torch seed yields the reference's weights."""
        fan_in = 1
        for e in self.plan.table:
            v = self.plan.view(self.arena.detach(), e)
            name = e['name']
            if _is_norm(name):
                v.fill_(1.0 if name.endswith('weight') else 0.0)
            elif len(e['shape']) >= 2:
                t = torch.empty(e['shape'], dtype=torch.float32)
                nn.init.kaiming_uniform_(t, a=math.sqrt(5))
                fan_in = t[0].numel()
                v.copy_(t)
            else:
                bound = 1.0 / math.sqrt(fan_in) if fan_in > 0 else 0.0
                t = torch.empty(e['shape'], dtype=torch.float32)
                nn.init.uniform_(t, -bound, bound)
                v.copy_(t)

    def init_scheme(self, init_type='orthogonal', scale=1, std=0.02):
        """weights_init_normal / _kaiming / _orthogonal (model/networks.py:14-55) over every Conv2d / Linear, drawn in
        `net.apply` order so a torch seed gives the reference's weights; biases are zeroed, GroupNorm is left alone
        (the reference's BatchNorm2d branch never matches a module of these networks)."""
        if init_type not in ('normal', 'kaiming', 'orthogonal'):
            raise NotImplementedError('initialization method [{:s}] not implemented'.format(init_type))
        for e in self.plan.table:
            name = e['name']
            if _is_norm(name):
                continue
            v = self.plan.view(self.arena.detach(), e)
            if len(e['shape']) >= 2:
                t = torch.empty(e['shape'], dtype=torch.float32)
                if init_type == 'orthogonal':
                    nn.init.orthogonal_(t, gain=1)
                elif init_type == 'normal':
                    nn.init.normal_(t, 0.0, std)
                else:
                    nn.init.kaiming_normal_(t, a=0, mode='fan_in')
                    t *= scale
                v.copy_(t.to(v.device))
            else:
                v.zero_()

    def init_orthogonal(self):
        self.init_scheme('orthogonal')

    # ---- the two sets of weights ---------------------------------------------------------------------
    def enable_ema(self):
        """Allocate the EMA arena (once) as a copy of the weights; +4 bytes per parameter of device memory."""
        if self.ema_arena is None:
            self.ema_arena = self.arena.data.clone()
        return self.ema_arena

    def ema_from_weights(self):
        """ema <- weights, in place (the EMA's start value: the weights the model starts from)."""
        self.enable_ema().copy_(self.arena.data)

    def weights(self):
        """The arena forward / reverse_step read: the live parameters, or the EMA inside `use_weights('ema')`."""
        return self.ema_arena if self._use_ema else self.arena.data

    @contextlib.contextmanager
    def use_weights(self, which):
        """Run forward / reverse_step (and everything built on them: the sampling loops) on 'ema' or 'live' weights.  The derived
        filters follow through ensure_derived, which re-prepares them from the arena in use; training always reads and writes the
        live arena and refuses to run inside an 'ema' selection."""
        if which not in ('ema', 'live'):
            raise ValueError("use_weights: 'ema' or 'live' (got %r)" % (which,))
        if which == 'ema' and self.ema_arena is None:
            raise L.Sr3Error('use_weights(\'ema\'): this model keeps no EMA weights (config train.ema_scheduler.enabled)')
        prev, self._use_ema = self._use_ema, which == 'ema'
        try:
            yield self
        finally:
            self._use_ema = prev

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        if self.ema_arena is not None:         # (a plain attribute: nn.Module moves parameters and buffers only)
            self.ema_arena = fn(self.ema_arena)
        return self

    # ---- derived weights ---------------------------------------------------------------------------
    def weights_changed(self):
        """Engine-side writes to the arena through raw pointers (fused Adam) are invisible to torch's version counter:
        the writer calls this."""
        self._weights_epoch += 1
        # the library refuses to run on filters it was told are stale (include/sr3_mi355x.h); ensure_derived re-prepares
        L.check(self.plan.lib.sr3_plan_invalidate_derived(self.plan.handle))

    def ensure_derived(self):
        """(Re)build the Winograd filters if the parameters moved or changed since the last build, or the other set of weights
        (`use_weights`) was selected.  Views handed out by named_parameters()/state-dict loading share the arena's version
        counter, so in-place edits through them are seen; a no-op (one tuple compare) otherwise."""
        arena = self.weights()
        if not arena.is_cuda:
            return
        key = (arena.data_ptr(), arena._version, self._weights_epoch, self.plan.options_epoch)
        if key == self._derived_key:
            return
        import ctypes as C
        lib = self.plan.lib
        need = int(lib.sr3_plan_derived_bytes(self.plan.handle))
        if need == 0:
            self._derived_key = key
            return
        if self._derived is None or self._derived.device != arena.device or self._derived.numel() * 4 < need:
            self._derived = torch.empty((need + 3) // 4, dtype=torch.float32, device=arena.device)
            L.check(lib.sr3_plan_bind_derived(self.plan.handle, L.ptr(self._derived), self._derived.numel() * 4))
        stream = C.c_void_p(torch.cuda.current_stream(arena.device).cuda_stream)
        L.check(lib.sr3_plan_prepare_derived(self.plan.handle, L.ptr(arena), stream))
        self._derived_key = key

    # ---- parameter / state-dict surface --------------------------------------------------------
    def named_parameters(self, prefix='', recurse=True, remove_duplicate=True):
        for e in self.plan.table:
            yield (prefix + ('.' if prefix else '') + e['name'], self.plan.view(self.arena.detach(), e))

    def parameters(self, recurse=True):
        for _, p in self.named_parameters():
            yield p

    def _export(self, arena, destination, prefix):
        if self.variant == 'ddpm':
            destination[prefix + 'time_mlp.0.inv_freq'] = self.freq.detach().clone()
        for e in self.plan.table:
            destination[prefix + e['name']] = self.plan.view(arena, e).detach().clone().contiguous()

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        self._export(self.arena.detach(), destination, prefix)

    def ema_state_dict(self, prefix=''):
        """The EMA weights under the keys, shapes and layouts (OIHW) of state_dict()."""
        if self.ema_arena is None:
            raise L.Sr3Error('ema_state_dict: this model keeps no EMA weights (config train.ema_scheduler.enabled)')
        destination = OrderedDict()
        self._export(self.ema_arena, destination, prefix)
        return destination

    def load_ema_state_dict(self, state_dict, prefix='', strict=True):
        """Fill the EMA arena from a state dict of that form (keys outside `prefix` -- the schedule buffers of a `*_ema.pth`
        -- are not this module's); the frequency table belongs to the live model and is not touched."""
        missing, unexpected, errors = [], [], []
        self._import(self.enable_ema(), state_dict, prefix, strict, missing, unexpected, errors, load_freq=False)
        if errors or (strict and (missing or unexpected)):
            raise RuntimeError('EMA weights: %s' % '; '.join(errors + ['missing %s' % k for k in missing]
                                                            + ['unexpected %s' % k for k in unexpected]))

    def state_dict(self, *args, destination=None, prefix='', keep_vars=False):
        # reference key order: buffers of a submodule come after its parameters; rebuild in table order
        if destination is None:
            destination = OrderedDict()
        self._save_to_state_dict(destination, prefix, keep_vars)
        return destination

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        self._import(self.arena.detach(), state_dict, prefix, strict, missing_keys, unexpected_keys, error_msgs)

    def _import(self, arena, state_dict, prefix, strict, missing_keys, unexpected_keys, error_msgs, load_freq=True):
        known = set()
        for e in self.plan.table:
            key = prefix + e['name']
            known.add(key)
            if key not in state_dict:
                missing_keys.append(key)
                continue
            src = state_dict[key]
            if tuple(src.shape) != tuple(e['shape']):
                error_msgs.append('size mismatch for %s: checkpoint %s vs model %s'
                                  % (key, tuple(src.shape), tuple(e['shape'])))
                continue
            self.plan.view(arena, e).copy_(src.to(arena.device, torch.float32))
        fkey = prefix + 'time_mlp.0.inv_freq'
        if self.variant == 'ddpm':
            known.add(fkey)
            if fkey in state_dict:
                if load_freq:
                    self.freq.copy_(state_dict[fkey].to(self.freq.device, torch.float32))
            else:
                missing_keys.append(fkey)
        if strict:
            for k in state_dict.keys():
                if k.startswith(prefix) and k not in known:
                    unexpected_keys.append(k)

    # ---- forward ---------------------------------------------------------------------------
    def forward(self, x, time, *, cond=None, level_table=None, step_dev=None, out=None, ws=None, full=False, t_map=None, feat_cache=None,
                refresh=True):
        """eps = UNet(x, time).  `x` may already contain the conditioning channels (reference call
        convention `denoise_fn(torch.cat([cond, x], 1), level)`), or they can be passed separately as
        `cond`, which the input conv reads as a virtual concat (nothing is materialised).  `ws`: a caller-owned
        engine.Workspace (the captured reverse loop keeps its own so no other call can move the buffer its graph
        has baked in).  `full`: a learned-variance network's variance rows too, [B, 2C, H, W] (engine.unet_forward).  `feat_cache`,
        `refresh` (plan option feat_cache): the feature cache a full forward writes and a cached one (refresh=False) reads."""
        self.ensure_derived()
        kw = {}
        if full:
            kw.update(full=True, t_map=t_map)
        if step_dev is None:
            if self.variant == 'sr3':
                kw['noise_level'] = time
            else:
                kw['timestep'] = time
        return E.unet_forward(self.plan, self.weights(), self.freq, self._ws if ws is None else ws, x, cond=cond,
                              level_table=level_table, step_dev=step_dev, out=out, feat_cache=feat_cache, refresh=refresh, **kw)

    def reverse_step(self, x, z, tables, step2, *, cond=None, level_table=None, clip_denoised=True, eps_out=None, ws=None,
                     t_map=None, c3=None, hist=None, feat_cache=None, refresh=True):
        """One whole iteration of the reverse loop in place on `x` (engine.reverse_step): what `GaussianDiffusion.p_sample_loop`
        captures into its hipGraph.  `feat_cache`, `refresh`: as forward's."""
        self.ensure_derived()
        return E.reverse_step(self.plan, self.weights(), self.freq, self._ws if ws is None else ws, x, z, tables, step2,
                              cond=cond, level_table=level_table, clip_denoised=clip_denoised, eps_out=eps_out, t_map=t_map, c3=c3,
                              hist=hist, feat_cache=feat_cache, refresh=refresh)

    # ---- training step (forward + backward inside the engine) ------------------------------------
    def train_step(self, hr, cond, z, ca, cb, level, tstep, grad_scale, drop_seed=None, objective=None, hybrid=None, per_image=None,
                   vlb_weight=None):
        """One fused forward + backward: returns the sum-reduced loss (0-dim tensor, summed over all data-parallel
        ranks) and leaves d(loss * grad_scale)/d params -- rank-summed -- in `grad_arena`.  `objective`: None (the network predicts
        z, unweighted, the plan's loss) or (tgt_z, tgt_x0, weight, loss_kind, huber_delta) of sr3_train_step_ex, the first three
        [B] device tensors or all None.  `hybrid` (a learned-variance network): (step_scalars [B, 8] fp32 on the device, lambda) of
        sr3_train_step_ex2 -- the loss is then L_simple + lambda L_vlb, and `last_vlb` holds the sum of L_vlb in bits (rank-summed).
        `per_image` (the loss-aware timestep sampler): the step_scalars [B, 8] of the drawn steps -- hybrid's own where both are given --
        sends the step through sr3_train_step_ex3, and `last_per_image` holds this rank's [B, 2] = {vb in bits / dim, x0 mse}; a pair
        (step_scalars, out) writes them into the caller's [B, 2] fp32 tensor.  `vlb_weight` (with per_image and hybrid; [B] fp32 on
        the device): per image, lambda * vlb_weight[b] weights L_vlb -- the importance weight of a step drawn by its loss, which the
        objective's `weight` carries to L_simple alone."""
        p_drop = self.dropout if self.training else 0.0
        if drop_seed is None:          # a fresh mask every step, drawn from torch's CPU generator
            drop_seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if p_drop > 0 else 0
        dev = hr.device
        if getattr(self, 'grad_arena', None) is None or self.grad_arena.device != dev:
            self.grad_arena = torch.zeros_like(self.arena.data)
        loss = torch.zeros(1, device=dev)
        # data parallel (one process per GPU): gradients are summed over ranks, so the 1/(b c h w) factor
        # uses the GLOBAL batch (model/model.py:52-53 under DataParallel); buckets reduce as they get ready
        import torch.distributed as tdist
        dp = self.dp_reducing()
        red, marks = None, (0, None, None)
        if self.accumulate > 1:        # the optimizer applies the sum of K micro-batch gradients: their mean
            grad_scale = grad_scale / self.accumulate
        if dp:
            red = self._grad_reducer(dev)
            grad_scale = grad_scale / tdist.get_world_size()
            if self.accumulate == 1:
                marks = red.mark_args()
        kw = {} if objective is None else {'objective': objective}
        self.last_vlb = None
        if hybrid is not None:
            vlb = torch.zeros(1, device=dev)
            kw['hybrid'] = (hybrid[0], float(hybrid[1]), vlb)
        self.last_per_image = None
        if per_image is not None:
            kw['per_image'] = tuple(per_image) if isinstance(per_image, (tuple, list)) else (per_image, torch.empty((hr.shape[0], 2), device=dev))
            if vlb_weight is not None:
                kw['per_image'] += (vlb_weight,)
        elif vlb_weight is not None:
            raise L.Sr3Error('training: vlb_weight goes with per_image (sr3_train_step_ex3)')
        self._engine_train_step(hr, cond, z, ca, cb, level, tstep, grad_scale, p_drop, drop_seed, marks, loss, **kw)
        sums = [loss] if hybrid is None else [loss, vlb]
        if dp:
            if self.accumulate == 1:
                red.reduce(self.grad_arena, extra=sums)
            else:                      # the arena is reduced once per optimizer step, accumulated (reduce_arena): only the loss here
                for t in sums:
                    tdist.all_reduce(t, op=tdist.ReduceOp.SUM)
        if hybrid is not None:
            self.last_vlb = vlb[0]
        if per_image is not None:
            self.last_per_image = kw['per_image'][1]
        return loss[0]

    def dp_reducing(self):
        """True when train_step's gradients are summed over data-parallel ranks (more than one, or a forced 1-rank job)."""
        import torch.distributed as tdist
        from . import dist as _dist
        return _dist.dp_world_size() > 1 or ((getattr(self, 'force_dp', False) or _dist.force_collectives)
                                             and tdist.is_available() and tdist.is_initialized())

    def _grad_reducer(self, dev):
        import torch.distributed as tdist
        from .dist import GradReducer
        red = getattr(self, '_reducer', None)
        if red is None or red.device != dev:
            red = self._reducer = GradReducer(self.arena.numel(), dev, tdist)
        return red

    def reduce_arena(self, arena):
        """Sum-all-reduce an arena-shaped tensor over the ranks, bucket by bucket on the current stream: the accumulated gradient
        of K > 1 micro-batches, once per optimizer step (EngineAdam).  Not overlapped with the last backward."""
        red = self._grad_reducer(arena.device)
        for lo, hi in red.buckets:
            red.dist.all_reduce(arena[lo:hi], op=red.dist.ReduceOp.SUM)

    def _engine_train_step(self, hr, cond, z, ca, cb, level, tstep, grad_scale, p_drop, drop_seed, marks, loss, objective=None,
                           hybrid=None, per_image=None):
        """The sr3_train_step_ex call itself (q_sample -> UNet forward -> loss -> backward, `marks` = the gradient-ready
        events of the data-parallel buckets); objective None is sr3_train_step's (NULL, NULL, NULL, -1, 0)."""
        import ctypes as C
        dev = hr.device
        if dev.type != 'cuda':
            raise L.Sr3Error('training needs the model on a GPU; there is no CPU fallback')
        if self._use_ema:
            raise L.Sr3Error("training inside use_weights('ema'): the training step reads and updates the live weights")
        self.ensure_derived()          # the train plan's block1 / Upsample convs run on the Winograd kernel
        B = hr.shape[0]
        plan = self.plan
        # the image size comes from the batch, as in the reference (p_losses trains on whatever the loader yields; image_size is
        # read by `sample` only): the training plan follows it (plan option train_geom, set when the first other size arrives)
        if hr.dim() != 4:
            raise L.Sr3Error('training: a (B, C, H, W) HR batch is expected (got %s)' % (tuple(hr.shape),))
        H, W = int(hr.shape[2]), int(hr.shape[3])
        if H <= 0 or W <= 0 or H % plan.divisor or W % plan.divisor:
            raise L.Sr3Error('image size %d x %d: height and width must be positive multiples of %d (the UNet halves the image %d times)'
                             % (H, W, plan.divisor, plan.desc.n_mults - 1))
        if cond is not None and (cond.shape[0] != B or tuple(cond.shape[2:]) != (H, W)):
            raise L.Sr3Error('training: the conditioning batch %s must have the batch and image size of HR %s'
                             % (tuple(cond.shape), tuple(hr.shape)))
        if tuple(z.shape) != tuple(hr.shape):
            raise L.Sr3Error('training: the noise %s must have the shape of HR %s' % (tuple(z.shape), tuple(hr.shape)))
        if (H, W) != (plan.image_size, plan.image_size) and not plan.options.get('train_geom'):
            plan.set_option('train_geom', 1)
            self.ensure_derived()      # (an option change invalidates the derived filters)
        plan.set_geometry(H, W)        # (a validation pass or the previous batch may have left the plan at another image size)
        cc = 0 if cond is None else cond.shape[1]
        need = int(plan.lib.sr3_train_workspace_bytes(plan.handle, B, cc))
        if need == 0:
            raise L.Sr3Error('training at image size %d x %d: %s' % (H, W, L.hint((plan.lib.sr3_last_error() or b'').decode())))
        ws = getattr(self, '_train_ws', None)
        if ws is None or ws.numel() < need + 256 or ws.device != dev:
            ws = self._train_ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
        off = (-ws.data_ptr()) % 256
        wsv = ws[off:off + need]
        n_marks, offs, evs = marks
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        tgt_z, tgt_x0, weight, kind, delta = (None, None, None, -1, 0.0) if objective is None else objective
        for t in (tgt_z, tgt_x0, weight):
            if t is not None and (t.device != dev or t.dtype != torch.float32 or t.numel() != B or not t.is_contiguous()):
                raise L.Sr3Error('training: tgt_z / tgt_x0 / weight must be contiguous fp32 tensors of %d elements on %s' % (B, dev))
        # the entry: sr3_train_step_ex; a learned-variance network's hybrid loss, _ex2; with the step's per-image terms of the bound
        # (with or without a variance head), _ex3.  Each takes the common arguments, then its own tail, then the stream
        entry, tail = plan.lib.sr3_train_step_ex, ()
        if per_image is not None or hybrid is not None:
            scal = (hybrid if per_image is None else per_image)[0]
            lam, vlb = (0.0, None) if hybrid is None else hybrid[1:]
            if per_image is not None:
                out, vw = (tuple(per_image) + (None,))[1:3]
                if tuple(out.shape) != (B, 2) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
                    raise L.Sr3Error('training: per_image_out must be a contiguous fp32 [%d, 2] tensor on %s' % (B, dev))
                if vw is not None and (hybrid is None or vw.device != dev or vw.dtype != torch.float32 or vw.numel() != B or not vw.is_contiguous()):
                    raise L.Sr3Error('training: vlb_weight goes with hybrid and must be a contiguous fp32 tensor of %d elements on %s' % (B, dev))
            if scal.device != dev or scal.dtype != torch.float32 or tuple(scal.shape) != (B, 8) or not scal.is_contiguous():
                raise L.Sr3Error('training: step_scalars must be a contiguous fp32 [%d, 8] tensor on %s' % (B, dev))
            entry, tail = plan.lib.sr3_train_step_ex2, (L.ptr(scal), C.c_float(lam), L.ptr(vlb))
            if per_image is not None:
                if hybrid is not None and hybrid[0] is not scal:
                    raise L.Sr3Error('training: per_image and hybrid must share one step_scalars tensor')
                nb = int(plan.lib.sr3_vlb_terms_partials_bytes(B))
                sc = getattr(self, '_vlb_scratch', None)
                if sc is None or sc.numel() != nb // 8 or sc.device != dev:
                    sc = self._vlb_scratch = torch.empty(nb // 8, dtype=torch.float64, device=dev)
                entry, tail = plan.lib.sr3_train_step_ex3, tail + (L.ptr(out), L.ptr(sc), nb, L.ptr(vw))
        L.check(entry(plan.handle, L.ptr(hr), L.ptr(cond), cc, L.ptr(z), L.ptr(ca), L.ptr(cb), L.ptr(level), L.ptr(tstep), L.ptr(self.freq),
                      L.ptr(self.arena.data), L.ptr(self.grad_arena), L.ptr(wsv), need, L.ptr(loss), C.c_float(grad_scale), C.c_float(p_drop),
                      C.c_uint(drop_seed & 0xFFFFFFFF), n_marks, offs, evs, B, L.ptr(tgt_z), L.ptr(tgt_x0), L.ptr(weight), int(kind),
                      C.c_float(delta), *tail, stream))

    def named_gradients(self):
        """(reference key, gradient view in the reference shape) after a train_step."""
        for e in self.plan.table:
            yield e['name'], self.plan.view(self.grad_arena, e)

    def extra_repr(self):
        d = self.plan.desc
        heads = 'head_dim=%d' % self.head_dim if self.head_dim is not None else 'n_head=%d' % self.n_head
        return 'variant=%s, in=%d, out=%d, inner=%d, groups=%d, mults=%s, attn_res=%s, %s, scale_shift_norm=%s, res_blocks=%d, image=%d, ' \
               'params=%d (packed arena, libsr3_mi355x)' % (
                   self.variant, d.in_channel, d.out_channel, d.inner_channel, d.norm_groups,
                   list(d.channel_mults[:d.n_mults]), list(d.attn_res[:d.n_attn_res]), heads, self.scale_shift_norm, d.res_blocks, d.image_size,
                   sum(e['numel'] for e in self.plan.table))
