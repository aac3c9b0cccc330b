"""Datasets over plain image folders (engine extension; the reference reads only the prepared hr_R / sr_L_R / lr_L triplets of
data/LRHR_dataset.py):

  HRCropDataset   -- training / validation from an HR-only folder of images of any size: __getitem__ decodes and slices an
                     (R, R, 3) uint8 crop and draws the sample's flip and degradation numbers (five; six, the last the JPEG
                     quality, when the config has a "jpeg" block; plus the twenty of 'deg2' when it has a second-order key); the LR and SR images are made on the MI355X for the whole
                     batch (data/degrade.py, data/__init__.py: DeviceBatches).
  LRFolderDataset -- "mode": "LR": a folder of plain low-resolution images to super-resolve; DeviceBatches resizes each by the
                     config's scale to make the conditioning image.
"""
import torch
from PIL import Image
from torch.utils.data import Dataset

import data.util as Util
from data.degrade import degrade_config, draw_deg, draw_deg2


class HRCropDataset(Dataset):
    def __init__(self, dataroot, datatype, l_resolution=16, r_resolution=128, split='train', data_len=-1, need_LR=False, degrade=None):
        if datatype == 'lmdb':
            raise NotImplementedError('"degrade" reads an image folder: datatype "lmdb" is not built for it, use "img"')
        if datatype != 'img':
            raise NotImplementedError('data_type [{:s}] is not recognized.'.format(datatype))
        self.degrade = degrade_config(degrade, l_resolution)      # DeviceBatches reads it
        self.datatype = datatype
        self.l_res = l_resolution
        self.r_res = r_resolution
        self.need_LR = need_LR
        self.split = split
        self.paths = Util.get_paths_from_images(dataroot)
        self.dataset_len = len(self.paths)
        self.data_len = self.dataset_len if data_len <= 0 else min(data_len, self.dataset_len)

    def __len__(self):
        return self.data_len

    def __getitem__(self, index):
        path = self.paths[index]
        img = Util.image_to_u8(Image.open(path).convert('RGB'))
        H, W, R = img.shape[0], img.shape[1], self.r_res
        if H < R or W < R:
            raise ValueError('%s is %d x %d: smaller than r_resolution %d' % (path, W, H, R))
        if self.split == 'train':
            # crop offset, flip (the draw LRHRDataset makes) and the degradation numbers, all on torch's global generator:
            # DataLoader worker seeding and torch.manual_seed govern them
            top = int(torch.randint(0, H - R + 1, (1,)).item())
            left = int(torch.randint(0, W - R + 1, (1,)).item())
            flip = bool(torch.rand(1).item() < 0.5)
            gen = None
        else:
            # the validation set is the same images on every pass: centre crop, no flip, draws seeded by the index
            top, left, flip = (H - R) // 2, (W - R) // 2, False
            gen = torch.Generator().manual_seed(self.degrade['seed'] + index)
        item = {'HR': img[top:top + R, left:left + R].contiguous(), 'Index': index, 'flip': flip, 'deg': draw_deg(self.degrade, gen)}
        if self.degrade['extended']:              # a second-order config: twenty more numbers, drawn right behind the first
            item['deg2'] = draw_deg2(self.degrade, gen)
        return item


class LRFolderDataset(Dataset):
    """Every image below `dataroot`, any size, as {'LR': (h, w, 3) uint8, 'Index'}; `scale` = r_resolution // l_resolution."""

    def __init__(self, dataroot, datatype, l_resolution=16, r_resolution=128, split='val', data_len=-1, resample='bicubic'):
        if datatype != 'img':
            raise NotImplementedError('"mode": "LR" reads an image folder: datatype "img" only')
        if split != 'val':
            raise NotImplementedError('"mode": "LR" has no ground truth: validation / inference datasets only')
        if r_resolution % l_resolution or r_resolution <= l_resolution:
            raise ValueError('"mode": "LR": r_resolution %d is not a multiple (> 1) of l_resolution %d' % (r_resolution, l_resolution))
        if resample not in ('bicubic', 'bilinear'):
            raise ValueError('resample %r is not "bicubic" or "bilinear"' % (resample,))
        self.lr_scale = r_resolution // l_resolution               # DeviceBatches reads these two
        self.resample = resample
        self.split = split
        self.need_LR = True
        self.paths = Util.get_paths_from_images(dataroot)
        self.data_len = len(self.paths) if data_len <= 0 else min(data_len, len(self.paths))

    def __len__(self):
        return self.data_len

    def __getitem__(self, index):
        return {'LR': Util.image_to_u8(Image.open(self.paths[index]).convert('RGB')), 'Index': index}
