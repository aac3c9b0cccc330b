"""DDPM model wrapper of the drop-in `model` package.

Same public methods and attributes as the reference wrapper (model/model.py:12-166): netG, device,
begin_step, begin_epoch, optG, log_dict, SR, data, schedule_phase; feed_data, optimize_parameters,
test, sample, set_loss, set_new_noise_schedule, get_current_log, get_current_visuals,
print_network, save_network, load_network -- so sr.py / infer.py / sample.py run unchanged.
"""
import contextlib
import logging
import os
from collections import OrderedDict

import torch

from sr3_hip import dist as _dist

from . import networks
from .base_model import BaseModel

logger = logging.getLogger('base')


class DDPM(BaseModel):
    def __init__(self, opt):
        super(DDPM, self).__init__(opt)
        self.netG = self.set_device(networks.define_G(opt))
        self.schedule_phase = None
        self._distill_state = None      # {'steps', 'walk'} of a distilled student: set by train.distill, or read from a checkpoint
        self.SR = None
        self.data = None
        self.set_loss()
        self.set_new_noise_schedule(opt['model']['beta_schedule']['train'], schedule_phase='train')
        # EMA of the weights: the reference's configs carry train.ema_scheduler {step_start_ema, update_ema_every, ema_decay} and never
        # use it; here the engine key `enabled` (default false) switches it on.  Without it nothing below allocates, writes or reads anything
        train_opt = opt.get('train') or {}
        ema_opt = train_opt.get('ema_scheduler') or {}
        self.ema_opt = dict(ema_opt) if ema_opt.get('enabled') else None
        if self.opt['phase'] == 'train':
            self.netG.train()
            if opt['model']['finetune_norm']:
                # model/model.py:26-35: every parameter is frozen and only names containing 'transformer' are
                # optimised -- no such name exists in either UNet, so the reference hands
                # torch.optim.Adam an empty list, which raises.  Same outcome here, same message.
                names = [k for k, _ in self.netG.named_parameters() if k.find('transformer') >= 0]
                if not names:
                    raise ValueError('optimizer got an empty parameter list')
                raise NotImplementedError('finetune_norm over %d "transformer" parameters' % len(names))
            from sr3_hip.optim import make_optimizer
            if self.ema_opt is not None:
                self.netG.denoise_fn.enable_ema()         # starts as the initial weights; load_network replaces it on a resume
            # engine keys of train.optimizer (absent in the reference's configs; absent = today's step): `accumulate` K micro-batches per
            # optimizer step, `clip_grad_norm` the global gradient norm to clip to (sr3_hip/optim.py)
            self.optG = make_optimizer(self.netG, lr=opt['train']['optimizer']['lr'],
                                       warmup_steps=int(opt['train']['optimizer'].get('warmup_steps') or 0), ema=self.ema_opt,
                                       accumulate=opt['train']['optimizer'].get('accumulate'),
                                       clip_grad_norm=opt['train']['optimizer'].get('clip_grad_norm'))
            self.log_dict = OrderedDict()
        self.load_network()
        # progressive distillation (engine key train.distill, absent by default: nothing below runs without it)
        self.distiller = None
        if self.opt['phase'] == 'train' and train_opt.get('distill') is not None:
            self._setup_distillation(train_opt['distill'])
        # data parallel: equalise the replicas once (each process initialised its own weights; a resumed checkpoint is
        # already identical) -- the counterpart of DataParallel's per-step replicate (model/networks.py:113-115)
        self._sam_wave = None
        if _dist.dp_active():
            _dist.sync_replicas(self.netG.denoise_fn)
        self.print_network()

    # ---- data / step ---------------------------------------------------------------------------
    def feed_data(self, data):
        self.data = self.set_device(data)

    def optimize_parameters(self):
        self.optG.zero_grad()
        # forward + backward run inside the engine; the gradients already carry the 1/(b*c*h*w) factor
        l_pix = self.netG(self.data) if self.distiller is None else self.distiller.step(self.data)
        b, c, h, w = self.data['HR'].shape
        # data parallel: the engine returns the loss summed over ALL ranks, so normalise by the global element count
        # (the reference's `l_pix.sum() / int(b*c*h*w)` over DataParallel's gathered per-replica sums, :52-53)
        l_pix = l_pix.sum() / int(b * c * h * w * _dist.dp_world_size())
        self.optG.step()
        gn = self.optG.last_grad_norm()
        if getattr(self.netG, 't_sampler', None) is not None and self.distiller is None:
            self.netG.flush_t_sampler()      # the step's per-image terms into the history: [B] floats, next to the loss's own copy below
        # learned variance: L_vlb of the step in bits per dimension (the engine's sum is over every rank's batch)
        vlb = getattr(self.netG, 'last_vlb', None) if getattr(self.netG, 'learned_variance', None) is not None else None
        names, vals = ['l_pix'], [l_pix]
        if gn is not None:      # clip_grad_norm: the norm of the last optimizer step taken, read in the same device-to-host copy as the loss
            names.append('grad_norm'), vals.append(gn)
        if vlb is not None:
            names.append('l_vlb'), vals.append(vlb / _dist.dp_world_size())
        if len(vals) == 1:
            self.log_dict['l_pix'] = l_pix.item()
        else:
            self.log_dict.update(zip(names, torch.stack([v.reshape(()).float() for v in vals]).tolist()))

    def _setup_distillation(self, dopt):
        """train.distill = {"teacher": "<checkpoint prefix>", "steps": N, "walk": "logsnr", "guidance_scale": null}: build the frozen teacher
        from <prefix>_gen.pth -- a second network of this config, on its own plan and arena -- and the Distiller that optimize_parameters
        steps in place of p_losses (sr3_hip/distill.py).  A teacher that is itself a distilled student recorded its walk in
        <prefix>_opt.pth (engine.distill.walk): that list is this round's teacher walk, which is how rounds chain.  Without a
        resume_state the student starts from the teacher's weights."""
        from sr3_hip import lib as L
        from sr3_hip.distill import Distiller
        if not hasattr(dopt, 'get') or dopt.get('teacher') is None or dopt.get('steps') is None:
            raise ValueError('train.distill: "teacher" (a checkpoint prefix) and "steps" are required (got %r)' % (dopt,))
        if getattr(self.netG, 'learned_variance', None) is not None:
            raise NotImplementedError('train.distill of a learned-variance model: the student\'s step trains the pixel loss alone and has no '
                                      'target for the variance rows; distil a model without model.diffusion.learned_variance')
        if self.device.type != 'cuda':
            raise L.Sr3Error('train.distill needs the model on a GPU (set gpu_ids); there is no CPU fallback')
        gen_path, opt_path = self._ckpt_paths(dopt['teacher'])
        sd = torch.load(gen_path, map_location='cpu')
        engine = (torch.load(opt_path, map_location='cpu').get('engine') or {}) if os.path.exists(opt_path) else {}
        t_opt = dict(self.opt, phase='val')            # (no initialisation draws: the weights come from the checkpoint)
        teacher = self.set_device(networks.define_G(t_opt))
        sched = self.opt['model']['beta_schedule']['train']
        teacher.set_new_noise_schedule({k: sched[k] for k in ('schedule', 'n_timestep', 'linear_start', 'linear_end')}, self.device)
        teacher.set_prediction(engine.get('prediction', 'eps'))
        teacher.load_state_dict(sd, strict=True)
        teacher.eval()
        walk = (engine.get('distill') or {}).get('walk')
        if walk is None:
            walk = dopt.get('walk') or 'logsnr'
        self.distiller = Distiller(self.netG, teacher, int(dopt['steps']), walk=walk, guidance_scale=dopt.get('guidance_scale'))
        self._distill_state = self.distiller.state()
        if self.opt['path']['resume_state'] is None:
            self.netG.load_state_dict(sd, strict=True)
            if self.ema_opt is not None:
                self.netG.denoise_fn.ema_from_weights()
        logger.info('Distilling [{:s}] ({:d} steps) into {:d} steps'.format(gen_path, 2 * self.distiller.steps, self.distiller.steps))

    def _apply_distilled_sampler(self, schedule_opt):
        """A distilled student is sampled on its own walk (DDIM, eta 0) wherever the phase's config names no sampler."""
        ds = self._distill_state
        if ds is not None and (not hasattr(schedule_opt, 'get') or schedule_opt.get('sampler') is None):
            self.netG.set_sampler(int(ds['steps']), 0.0, kind='ddim', walk=list(ds['walk']))

    def _sampling_weights(self):
        """Train phase with EMA enabled: validation and sampling run on the EMA weights (everything below netG's sampling loops,
        the ValWave / SampleWave paths included, reads the arena this selects); training goes on with the live ones."""
        un = self.netG.denoise_fn
        if self.opt['phase'] == 'train' and self.ema_opt is not None and un.ema_arena is not None:
            return un.use_weights('ema')
        return contextlib.nullcontext()

    def _backprojection_target(self):
        """Under the "backprojection" key: the batch's real LR image (data['LR'], [B, C, H / scale, W / scale]) as the chain's target;
        None -- the down-sampled conditioning image -- when the key is off or the batch carries no LR image of that shape."""
        bp = getattr(self.netG, 'backprojection', None)
        lr = self.data.get('LR') if isinstance(self.data, dict) else None
        sr = self.data.get('SR') if isinstance(self.data, dict) else None
        if bp is None or not torch.is_tensor(lr) or not torch.is_tensor(sr) or lr.dim() != 4 or sr.dim() != 4:
            return None
        s = bp['scale']
        B, _, H, W = sr.shape
        if H % s or W % s or tuple(lr.shape) != (B, self.netG.channels, H // s, W // s):
            return None
        return lr

    def _restore_target(self):
        """Under the "restore" key: the batch's own target -- (data['known'], data['mask']) for the mask operator, data['gray'] for the
        gray operator -- or None (the gray operator's default; the mask operator then says what it needs) when the key is off or the
        batch carries none."""
        rs = getattr(self.netG, 'restore', None)
        data = getattr(self, 'data', None)
        data = data if isinstance(data, dict) else {}
        if rs is None:
            return None
        if rs['operator'] == 'mask':
            known, mask = data.get('known'), data.get('mask')
            return (known, mask) if torch.is_tensor(known) and torch.is_tensor(mask) else None
        gray = data.get('gray')
        return gray if torch.is_tensor(gray) else None

    def test(self, continous=False):
        self.netG.eval()
        with torch.no_grad(), self._sampling_weights():
            wave = self.data.get('_dp_wave') if isinstance(self.data, dict) else None
            if getattr(self.netG, 'restore', None) is not None:      # (a restoring chain runs on the batch as it was fed)
                self.SR = self.netG.super_resolution(self.data['SR'], continous, restore_target=self._restore_target())
            elif wave is not None:
                # the validation loader groups consecutive items into waves (sr3_hip.dist.ValWave): the chains of a wave run once,
                # a rank's items as one batch (and, data parallel, dealt over the ranks); every caller gets its item's image back
                self.SR = wave.result(self.netG, self.data['_dp_pos'], continous)
            else:
                lr = self._backprojection_target()
                if lr is None:
                    self.SR = self.netG.super_resolution(self.data['SR'], continous)
                else:
                    self.SR = self.netG.super_resolution(self.data['SR'], continous, backprojection_target=lr)
        self.netG.train()

    def calc_bpd(self, steps=None):
        """The variational bound of the fed batch by timestep (EngineDiffusion.calc_bpd_loop): a dict of vb [B, S], x0_mse [B, S],
        prior_bpd [B], total_bpd [B] in bits per dimension; on the EMA weights where the train phase keeps them."""
        self.netG.eval()
        with torch.no_grad(), self._sampling_weights():
            out = self.netG.calc_bpd_loop(self.data if self.netG.conditional else self.data['HR'], steps=steps)
        self.netG.train()
        return out

    def sample(self, batch_size=1, continous=False):
        self.netG.eval()
        with torch.no_grad(), self._sampling_weights():
            if getattr(self.netG, 'restore', None) is not None:
                self.SR = self.netG.sample(batch_size, continous, restore_target=self._restore_target())
            elif _dist.dp_active():
                if self._sam_wave is None:
                    self._sam_wave = _dist.SampleWave()
                self.SR = self._sam_wave.next(self.netG, batch_size, continous)
            else:
                self.SR = self.netG.sample(batch_size, continous)
        self.netG.train()

    def set_loss(self):
        self.netG.set_loss(self.device)

    def set_new_noise_schedule(self, schedule_opt, schedule_phase='train'):
        if self.schedule_phase is None or self.schedule_phase != schedule_phase:
            self.schedule_phase = schedule_phase
            self.netG.set_new_noise_schedule(schedule_opt, self.device)
            self._apply_distilled_sampler(schedule_opt)

    # ---- reporting -----------------------------------------------------------------------------
    def get_current_log(self):
        return self.log_dict

    def get_current_visuals(self, need_LR=True, sample=False):
        out = OrderedDict()
        if sample:
            out['SAM'] = self.SR.detach().float().cpu()
            return out
        out['SR'] = self.SR.detach().float().cpu()
        out['INF'] = self.data['SR'].detach().float().cpu()
        out['HR'] = self.data['HR'].detach().float().cpu()
        if need_LR and 'LR' in self.data:
            out['LR'] = self.data['LR'].detach().float().cpu()
        else:
            out['LR'] = out['INF']
        return out

    def print_network(self):
        if not _dist.is_primary():
            return
        s, n = self.get_network_description(self.netG)
        logger.info('Network G structure: {}, with parameters: {:,d}'.format(self.netG.__class__.__name__, n))
        logger.info(s)

    # ---- checkpoints: the reference's file names and key schema (model/model.py:124-166) ----------
    def _ckpt_paths(self, stem):
        return '{}_gen.pth'.format(stem), '{}_opt.pth'.format(stem)

    @staticmethod
    def _ema_path(stem):
        return '{}_ema.pth'.format(stem)

    def save_network(self, epoch, iter_step):
        stem = os.path.join(self.opt['path']['checkpoint'], 'I{}_E{}'.format(iter_step, epoch))
        gen_path, opt_path = self._ckpt_paths(stem)
        if _dist.is_primary():          # replicas are identical: one writer
            state = OrderedDict((k, v.cpu()) for k, v in self.netG.state_dict().items())
            torch.save(state, gen_path)
            if self.opt['phase'] == 'train' and self.ema_opt is not None:
                # the key set, shapes and dtypes of *_gen.pth (schedule buffers included) with the EMA weights in the UNet's
                # entries: renamed to *_gen.pth it loads anywhere a generator checkpoint does
                state.update((k, v.cpu()) for k, v in self.netG.denoise_fn.ema_state_dict('denoise_fn.').items())
                torch.save(state, self._ema_path(stem))
            ck = {'epoch': epoch, 'iter': iter_step, 'scheduler': None, 'optimizer': self.optG.state_dict()}
            if self.netG.prediction != 'eps':
                # what the weights predict (model.diffusion.prediction): *_gen.pth keeps the reference's format, so the training state
                # records it; an eps model's file has the reference's keys only
                ck['engine'] = {'prediction': self.netG.prediction}
            if self._distill_state is not None:
                # a distilled student: the chain it was trained for -- what it is sampled on, and the next round's teacher walk
                ck.setdefault('engine', {})['distill'] = {'steps': int(self._distill_state['steps']),
                                                          'walk': [int(v) for v in self._distill_state['walk']]}
            if getattr(self.netG, 't_sampler', None) is not None:
                # the loss-aware timestep sampler's history (this rank's), under the key alone
                self.netG.flush_t_sampler()
                ck['t_sampler'] = {k: torch.from_numpy(v) if hasattr(v, 'dtype') else v for k, v in self.netG.t_sampler.state_dict().items()}
            torch.save(ck, opt_path)
            logger.info('Saved model in [{:s}] ...'.format(gen_path))
        _dist.barrier()                 # nobody runs ahead (or resumes) before the files are complete

    def load_network(self):
        stem = self.opt['path']['resume_state']
        if stem is None:
            return
        logger.info('Loading pretrained model for G [{:s}] ...'.format(stem))
        gen_path, opt_path = self._ckpt_paths(stem)
        ema_path = self._ema_path(stem)
        strict = not self.opt['model']['finetune_norm']
        if self.opt['phase'] != 'train' and self.ema_opt is not None:
            # validation / inference with EMA enabled: the model's weights ARE the EMA weights
            if not os.path.exists(ema_path):
                raise FileNotFoundError('train.ema_scheduler.enabled is set but [{:s}] does not exist'.format(ema_path))
            gen_path = ema_path
        self.netG.load_state_dict(torch.load(gen_path, map_location='cpu'), strict=strict)
        if self.opt['phase'] == 'train' and self.ema_opt is not None:
            un = self.netG.denoise_fn
            if os.path.exists(ema_path):
                un.load_ema_state_dict(torch.load(ema_path, map_location='cpu'), prefix='denoise_fn.', strict=strict)
            else:
                logger.warning('EMA weights [{:s}] not found: the EMA starts from the loaded weights'.format(ema_path))
                un.ema_from_weights()
        if self.opt['phase'] != 'train' and os.path.exists(opt_path):
            # a distilled student's training state records its chain: sampled on it unless the config names a sampler
            ds = (torch.load(opt_path, map_location='cpu').get('engine') or {}).get('distill')
            if ds is not None:
                self._distill_state = {'steps': int(ds['steps']), 'walk': [int(v) for v in ds['walk']]}
                self._apply_distilled_sampler(self.opt['model']['beta_schedule'].get(self.schedule_phase))
        if self.opt['phase'] == 'train':
            ck = torch.load(opt_path, map_location='cpu')
            saved = (ck.get('engine') or {}).get('prediction', 'eps')
            if saved != self.netG.prediction:
                raise ValueError('[{:s}] was trained with prediction {!r} but the config\'s model.diffusion.prediction is {!r}'.format(
                    opt_path, saved, self.netG.prediction))
            self.optG.load_state_dict(ck['optimizer'])
            if getattr(self.netG, 't_sampler', None) is not None and ck.get('t_sampler') is not None:
                self.netG.t_sampler.load_state_dict(ck['t_sampler'])
            self.begin_step = ck['iter']
            self.begin_epoch = ck['epoch']
            _dist.resume_epoch = int(ck['epoch'])
