'''create dataset and dataloader -- drop-in for the reference's data/__init__.py (create_dataloader, create_dataset:
same arguments), with the per-sample float transform moved onto the MI355X: the torch DataLoader collates uint8
batches, DeviceBatches turns each into the reference's batch dict ({'HR', 'SR', ['LR'], 'Index'}: fp32 NCHW in
[-1, 1]) already resident on the device, which DDPM.feed_data then takes as is.  Engine extensions: a dataset block with a
"degrade" key trains from an HR-only folder -- the LR / SR images are made on the device per batch (data/degrade.py,
data/HR_dataset.py) -- and "mode": "LR" super-resolves a folder of plain LR images.'''
import logging
import os

import torch
import torch.utils.data


class DeviceBatches(object):
    """Iterable over a uint8 DataLoader that yields the reference's batch dicts with device-resident fp32 tensors.
    `len()`, iteration order and the dict keys are the DataLoader's; `.dataset` / `.batch_size` pass through."""

    def __init__(self, loader, device=None, min_max=(-1, 1), deal_waves=False):
        self.loader = loader
        self.device = device
        self.min_max = min_max
        self.dataset = loader.dataset
        self.batch_size = loader.batch_size
        self.epoch = 0               # reshuffles a rank-sharded sampler every pass (DistributedSampler.set_epoch)
        self.deal_waves = deal_waves

    def __len__(self):
        return len(self.loader)

    def _device_batches(self):
        import data.util as Util
        sampler = getattr(self.loader, 'sampler', None)
        if hasattr(sampler, 'set_epoch'):
            if self.epoch == 0:
                from sr3_hip import dist as _dist
                self.epoch = _dist.resume_epoch      # a resumed run continues the reshuffle sequence
            sampler.set_epoch(self.epoch)
        self.epoch += 1
        lr_scale = getattr(self.dataset, 'lr_scale', None)
        for batch in self.loader:
            flip = batch.pop('flip', None)
            if 'deg' in batch:
                batch = self._degraded(batch)
            elif lr_scale is not None:
                batch = self._upscaled(batch, lr_scale)
            out = {}
            for k, v in batch.items():
                if torch.is_tensor(v) and v.dtype == torch.uint8 and v.dim() == 4:
                    out[k] = Util.u8_batch_to_f32(v, flip, self.min_max, self.device)
                else:
                    out[k] = v
            if lr_scale is not None:
                out['HR'] = out['SR']        # no ground truth: the conditioning image stands in (infer.py saves it as it is)
            yield out

    def _on_device(self, t):
        dev = self.device
        if dev is None and torch.cuda.is_available():
            dev = torch.device('cuda', torch.cuda.current_device())
        return t if dev is None else t.to(dev, non_blocking=True)      # (no GPU: the engine call that follows says so)

    def _degraded(self, batch):
        """A batch of an HR-only folder (data/HR_dataset.py: HRCropDataset): uint8 crops plus each sample's degradation draws ->
        the uint8 HR / SR (/ LR) batch of a prepared dataset, made on the device (data/degrade.py: blur, resize, noise, JPEG, resize;
        'deg' is (n, 5), or (n, 6) with the JPEG qualities when the config has a "jpeg" block).  The noise: training draws from
        the device's default generator; validation from a device generator seeded seed + index, the same on every pass."""
        from data.degrade import degrade_batch
        cfg, hr = self.dataset.degrade, self._on_device(batch['HR'])
        gen = None
        if self.dataset.split != 'train':
            if hr.shape[0] != 1:
                raise ValueError('validation batches of an HR-only folder hold one image (the per-index noise stream)')
            gen = torch.Generator(device=hr.device).manual_seed(cfg['seed'] + int(batch['Index'][0]))
        lr, sr = degrade_batch(hr, batch['deg'], cfg, generator=gen, deg2=batch.get('deg2'))      # ('deg2': a second-order config's draws)
        out = {'HR': hr, 'SR': sr, 'Index': batch['Index']}
        if self.dataset.need_LR:
            out['LR'] = lr
        return out

    def _upscaled(self, batch, scale):
        """"mode": "LR" (data/HR_dataset.py: LRFolderDataset): the conditioning image is the LR image resized by `scale`."""
        from data.prepare_data import resize_batch
        from data.degrade import _RESAMPLE
        lr = self._on_device(batch['LR'])
        sr = resize_batch(lr, (lr.shape[1] * scale, lr.shape[2] * scale), _RESAMPLE[self.dataset.resample])
        return {'SR': sr, 'LR': lr, 'Index': batch['Index']}

    def __iter__(self):
        _, world = _dp()
        from sr3_hip.dist import dp_active, val_chain_batch
        chain = val_chain_batch() if self.deal_waves else 1
        # (SR3_VAL_ITEM_STREAMS=1 set explicitly: one-item waves too, so a one-chain-per-image run draws the per-item streams a
        # batched run draws -- the comparison the streams exist for; unset, a plain batch-1 run keeps the default generator)
        force = self.deal_waves and os.environ.get('SR3_VAL_ITEM_STREAMS') == '1'
        if not (self.deal_waves and (dp_active() or chain > 1 or force)):
            yield from self._device_batches()
            return
        # validation: every rank walks ALL items in order, `world * chain` at a time; the wave object lets DDPM.test run the
        # reverse chains once per wave -- a rank's items as one chain batch -- and share the finished images (sr3_hip.dist.ValWave)
        from sr3_hip.dist import ValWave
        world = world if dp_active() else 1
        group = []
        first = 0                     # index of group[0] in this pass over the validation set: item k draws stream k in every pass

        def flush():
            wave = ValWave([b['SR'] for b in group], first_item=first)
            for pos, b in enumerate(group):
                b['_dp_wave'], b['_dp_pos'] = wave, pos
                yield b
        for b in self._device_batches():
            if group and b['SR'].shape != group[0]['SR'].shape:      # a wave holds items of one size ("mode": "LR" folders mix them)
                yield from flush()
                first += len(group)
                group = []
            group.append(b)
            if len(group) == world * chain:
                yield from flush()
                first += len(group)
                group = []
        if group:
            yield from flush()


def _dp():
    """(rank, world) of the data-parallel job this process belongs to; (0, 1) for a single process.  sr.py builds its
    loaders BEFORE the model (sr.py:52-66), so this is where a torchrun-started script usually joins the job."""
    from sr3_hip.dist import bootstrap
    rank, world, _ = bootstrap()
    return rank, world


def create_dataloader(dataset, dataset_opt, phase, device=None):
    '''create dataloader.  Data parallel (one process per GPU): `batch_size` stays the GLOBAL batch of the config, as
    under the reference's nn.DataParallel, which scatters each loader batch over the GPUs (model/networks.py:113-115);
    every rank draws batch_size / world samples per step from its own disjoint shard of the (shuffled) index list.'''
    if phase == 'train':
        rank, world = _dp()
        bs, sampler, shuffle = dataset_opt['batch_size'], None, dataset_opt['use_shuffle']
        if world > 1:
            if bs % world:
                raise ValueError('batch_size %d is not divisible by the %d data-parallel ranks' % (bs, world))
            bs //= world
            # the permutation seed comes from the global torch RNG like RandomSampler's (so `torch.manual_seed` governs
            # the order as it does in the reference) -- rank 0's draw, shared, so the shards stay disjoint
            from sr3_hip.dist import broadcast_int
            seed = broadcast_int(int(torch.empty((), dtype=torch.int64).random_().item()) & 0x7FFFFFFF)
            sampler = torch.utils.data.distributed.DistributedSampler(dataset, num_replicas=world, rank=rank,
                                                                      shuffle=bool(shuffle), seed=seed, drop_last=False)
            shuffle = False
        loader = torch.utils.data.DataLoader(dataset, batch_size=bs, shuffle=shuffle, sampler=sampler,
                                             num_workers=dataset_opt['num_workers'], pin_memory=True)
    elif phase == 'val':
        _dp()
        loader = torch.utils.data.DataLoader(dataset, batch_size=1, shuffle=False, num_workers=1, pin_memory=True)
        return DeviceBatches(loader, device, deal_waves=True)
    else:
        raise NotImplementedError('Dataloader [{:s}] is not found.'.format(phase))
    return DeviceBatches(loader, device)


def create_dataset(dataset_opt, phase):
    '''create dataset'''
    mode = dataset_opt['mode']
    args = dict(dataroot=dataset_opt['dataroot'], datatype=dataset_opt['datatype'], l_resolution=dataset_opt['l_resolution'],
                r_resolution=dataset_opt['r_resolution'], split=phase, data_len=dataset_opt['data_len'])
    if mode == 'LR':                         # a folder of plain LR images to super-resolve
        from data.HR_dataset import LRFolderDataset
        dataset = LRFolderDataset(resample=dataset_opt.get('resample', 'bicubic'), **args)
    elif 'degrade' in dataset_opt:           # an HR-only folder: crops, degraded on the device
        from data.HR_dataset import HRCropDataset
        dataset = HRCropDataset(need_LR=(mode == 'LRHR'), degrade=dataset_opt['degrade'], **args)
    else:
        from data.LRHR_dataset import LRHRDataset as D
        dataset = D(need_LR=(mode == 'LRHR'), **args)
    logging.getLogger('base').info('Dataset [{:s} - {:s}] is created.'.format(dataset.__class__.__name__, dataset_opt['name']))
    return dataset
