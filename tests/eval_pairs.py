"""Full-frame image pairs for the evaluation tests (GPU-free, seeded): test_metrics_cpu.py checks on them that the reference's
float32 mean and a float64 sum agree within the PSNR bar, test_gpu_eval.py scores them with mulut_eval_y."""
import os

import numpy as np

from conftest import GOLDEN


def big_pairs():
    """{name: (gt, out, shave)}: the pairs test_gpu_eval.py scores beyond mulut_eval_y's first grid-stride pass (262,144 interior
    pixels) and first 256 SSIM tiles.  Two 1080 x 1920 HR frames, one photograph (the DIV2K sample, mirror-tiled) and one
    photograph-like frame under heavy noise, each against itself plus rounding noise as gen_golden_metrics.py builds its random
    pairs; and two frames whose 'valid' SSIM map (H - 10, W - 10) is one pixel above / below a multiple of the 32-pixel tile."""
    from mulut_amd.synth import natural_frames, real_frames
    rng = np.random.default_rng(21)
    photo = real_frames(1, 1080, 1920, os.path.join(GOLDEN, "DIV2K_LR_X4", "0001x4.png"), seed=2)[0]
    noisy = np.clip(natural_frames(1, 1080, 1920, 3, seed=3)[0] + rng.normal(0, 30, (1080, 1920, 3)), 0, 255).astype(np.uint8)
    edge_hi = natural_frames(1, 10 + 32 * 17 + 1, 10 + 32 * 19 + 1, 3, seed=4)[0]
    edge_lo = natural_frames(1, 10 + 32 * 17 - 1, 10 + 32 * 19 - 1, 3, seed=5)[0]
    out = {}
    for name, gt, sigma, shave in (("photo_1080p", photo, 6, 4), ("noisy_1080p", noisy, 16, 4), ("tiles_plus_1", edge_hi, 9, 4),
                                   ("tiles_minus_1", edge_lo, 9, 3)):
        out[name] = (gt, np.clip(np.round(gt + rng.normal(0, sigma, gt.shape)), 0, 255).astype(np.uint8), shave)
    return out
