"""Network factory of the drop-in `model` package (reference: model/networks.py:83-116).

`define_G(opt)` reads the same `opt['model']` subtree and returns a GaussianDiffusion whose
denoiser runs on libsr3_mi355x.  Differences by design: no nn.DataParallel wrap -- multi-GPU
is one process per GPU (see sr3_hip/dist.py); `distributed` in opt is accepted and ignored.
"""
import logging

logger = logging.getLogger('base')


def init_weights(net, init_type='kaiming', scale=1, std=0.02):
    """model/networks.py:58-77: `scale` applies to 'kaiming', `std` to 'normal'; define_G uses 'orthogonal'.  The draws
    happen in the reference's `net.apply` order (sr3_hip.nn.EngineUNet.init_scheme)."""
    logger.info('Initialization method [{:s}]'.format(init_type))
    net.denoise_fn.init_scheme(init_type, scale=scale, std=std)


def define_G(opt):
    model_opt = opt['model']
    which = model_opt['which_model_G']
    if which == 'ddpm':
        from .ddpm_modules import diffusion, unet
    elif which == 'sr3':
        from .sr3_modules import diffusion, unet
    else:
        raise NotImplementedError('which_model_G [{}]'.format(which))
    u = model_opt['unet']
    if ('norm_groups' not in u) or u['norm_groups'] is None:
        u['norm_groups'] = 32
    # engine key model.diffusion.learned_variance: {"lambda": 0.001} -- the UNet emits 2 x channels rows, the prediction and a variance head
    # (set_learned_variance); without the key an out_channel above 4 is refused as ever
    lv = model_opt['diffusion'].get('learned_variance')
    if lv is not None and lv is not False:
        want = 2 * int(model_opt['diffusion']['channels'])
        if int(u['out_channel']) != want:
            raise ValueError('learned_variance needs unet.out_channel = %d (2 x %d image channels: the prediction and the variance head); '
                             'the config has out_channel %d' % (want, int(model_opt['diffusion']['channels']), int(u['out_channel'])))
    else:
        lv = None
    # engine keys model.unet.n_head / model.unet.head_dim: multi-head SelfAttention (the reference module's n_head, which its constructors
    # never expose) -- n_head heads at every attention level, or heads of head_dim channels each (ADM's num_head_channels).  Absent = one
    # head.  The weights keep their shapes, so *_gen.pth does not record the head count: the config carries it
    heads = {k: int(u[k]) for k in ('n_head', 'head_dim') if u.get(k) is not None}
    if len(heads) == 2:
        raise ValueError('model.unet.n_head (%d) and model.unet.head_dim (%d) are mutually exclusive: set one' % (heads['n_head'], heads['head_dim']))
    # engine key model.unet.scale_shift_norm: true -- the time / noise embedding enters a res block as (scale, shift) of its second GroupNorm,
    # GN2(h) (1 + scale) + shift (ADM's use_scale_shift_norm), not as a row added to conv1's output.  Absent or false: the reference's
    # blocks.  The projection's shapes double, so a checkpoint of the other form fails to load on the shape; the config carries the key
    ssn = u.get('scale_shift_norm', False)
    if not isinstance(ssn, bool):
        raise ValueError('model.unet.scale_shift_norm must be true or false (got %r)' % (ssn,))
    if u.get('use_affine_level'):
        raise NotImplementedError('model.unet.use_affine_level is not built (the reference\'s constructors never forward it); '
                                  'model.unet.scale_shift_norm: true modulates the second GroupNorm of every res block instead')
    if ssn:
        heads['scale_shift_norm'] = True
    denoiser = unet.UNet(
        **heads,
        in_channel=u['in_channel'], out_channel=u['out_channel'], norm_groups=u['norm_groups'],
        inner_channel=u['inner_channel'], channel_mults=u['channel_multiplier'], attn_res=u['attn_res'],
        res_blocks=u['res_blocks'], dropout=u['dropout'], image_size=model_opt['diffusion']['image_size'],
        long_attention=bool(u.get('long_attention', False)),      # (engine key: images whose attention level exceeds the LDS score strip)
        **({} if lv is None else {'learned_variance': True}))
    netG = diffusion.GaussianDiffusion(
        denoiser, image_size=model_opt['diffusion']['image_size'], channels=model_opt['diffusion']['channels'],
        loss_type='l1', conditional=model_opt['diffusion']['conditional'],
        schedule_opt=model_opt['beta_schedule']['train'])
    # engine keys of model.diffusion (absent in the reference's configs; absent = the reference's objective): "prediction": "eps" | "v" |
    # "x0", what the network's output stands for, and "loss": {"type": "l1" | "l2" | "huber", "delta", "weight": "uniform" | "min_snr",
    # "gamma"} (sr3_hip/diffusion.py: set_prediction, set_objective); "cond_drop": p, the probability that a training image's conditioning
    # is zeroed -- what a model needs to have seen for guided sampling (set_cond_drop).  *_gen.pth does not record them: the config
    # carries them
    d = model_opt['diffusion']
    if d.get('prediction') is not None:
        netG.set_prediction(d['prediction'])
    loss = d.get('loss')
    if loss is not None:
        netG.set_objective(loss.get('type', 'l1'), loss.get('delta'), loss.get('weight', 'uniform'), loss.get('gamma'))
    if d.get('cond_drop') is not None:
        netG.set_cond_drop(d['cond_drop'])
    if lv is not None:
        from sr3_hip.schedules import parse_learned_variance
        netG.set_learned_variance(parse_learned_variance(lv))
    # "t_sampler": {"type": "loss_second_moment", "history": 10, "uniform": 0.001} -- p_losses draws t by its loss (set_t_sampler; behind
    # learned_variance, which an SR3 model needs for it); absent: uniform draws, today's launches and checkpoint keys
    if d.get('t_sampler') is not None and d.get('t_sampler') is not False:
        from sr3_hip.t_sampler import parse_t_sampler
        netG.set_t_sampler(**parse_t_sampler(d['t_sampler']))
    # "self_condition": {"prob": 0.5} | true -- the network reads its own last x0 as extra input channels (set_self_condition; unet.in_channel
    # is then conditioning channels + 2 x channels)
    if d.get('self_condition') is not None:
        from sr3_hip.schedules import parse_self_condition
        netG.set_self_condition(parse_self_condition(d['self_condition']))
    # "cond_augment": {"max_level": 0.5, "sample_level": 0.1, "level_channel": true} -- the network reads the conditioning image diffused to
    # a level of its own, and that level as one more input plane (set_cond_augment; unet.in_channel is then conditioning channels + 1 + channels)
    if d.get('cond_augment') is not None:
        from sr3_hip.schedules import parse_cond_augment
        netG.set_cond_augment(**parse_cond_augment(d['cond_augment']))
    if opt['phase'] == 'train':
        init_weights(netG, init_type='orthogonal')
    return netG
