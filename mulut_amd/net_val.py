"""Validation of a trained network on the fused forward: the twin of sr/1_train_model.py:70-117 (`valid_steps`) over a NetEngine,
built from what the fine-tune validation already has (ft_val.iter_val_pairs, the naming scheme of ft_val.val_png_name)."""
import os

import numpy as np
import torch
from PIL import Image

from . import ft_val
from .metrics import psnr, rgb2ycbcr


def net_png_name(ds, fn, suffix="net"):
    """ft_val.val_png_name's scheme (the last '_'-separated token of "{dataset}_{stem}", sr/1_train_model.py:109-114) with the
    suffixes of the training script: _net, _input, _gt."""
    return '{}_{}.png'.format((ds + '_' + fn[:-4]).split('_')[-1], suffix)


def net_valid_steps(net_engine, opt, it, log=print):
    """Each validation image through NetEngine.predict (bytes to bytes on the device), Y-PSNR with shave = scale on the host
    (:103-104), `{valoutDir}/{dataset}/{name}_net.png` (and _input / _gt below iteration 10000, :106-111), one line per dataset.
    Returns {dataset: float64 array [images]} of the PSNRs."""
    results = {}
    for ds, pairs in ft_val._by_dataset(opt):
        out_dir = os.path.join(opt.valoutDir, ds)
        os.makedirs(out_dir, exist_ok=True)
        psnrs = []
        for _, fn, im, lb in pairs:
            x = torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1)[None])).to(net_engine.device)
            pred = net_engine.predict(x)[0].permute(1, 2, 0).contiguous().cpu().numpy()
            psnrs.append(psnr(rgb2ycbcr(pred)[:, :, 0], rgb2ycbcr(lb)[:, :, 0], opt.scale))
            if it < 10000:
                Image.fromarray(im).save(os.path.join(out_dir, net_png_name(ds, fn, "input")))
                Image.fromarray(lb).save(os.path.join(out_dir, net_png_name(ds, fn, "gt")))
            Image.fromarray(pred).save(os.path.join(out_dir, net_png_name(ds, fn)))
        results[ds] = np.asarray(psnrs, dtype=np.float64)
        log('Iter {} | Dataset {} | AVG Val PSNR: {}'.format(it, ds, np.mean(results[ds])))
    return results
