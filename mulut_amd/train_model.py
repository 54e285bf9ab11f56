"""GPU twin of the reference's training driver (sr/1_train_model.py:122-233): trains an `SRNets` on the fused HIP forward and backward.

    python -m mulut_amd.train_model --stages 2 --modes sdy -e <expDir> --trainDir <DIV2K-like dir> --valDir <benchmark dir>

Options are the reference's `TrainOptions` (`options.TrainOptions`).  The network's stages run through `net_train.NetTrainer`
(`mulut_net_stage_sum` forward, `mulut_net_stage_backward` backward); `p.grad`, `torch.optim.Adam` and `LambdaLR` are used as the
reference uses them.  `--torchPath` runs the same loop on `network.SRNets` as torch operators: the baseline of the benchmark and of
the tests.  Batches come from `ft_data.DeviceCropProvider` (`--hostData`: `CropProvider`), validation from `NetEngine.load_weights` plus
`net_val.net_valid_steps`, and `Model_{:06d}.pth` is `torch.save(model_G)`, which `network.load_checkpoint` and so
`transfer_to_lut` (with `--fused` too) read.  The log lines are the reference's.  TensorBoard scalars are written only if
`torch.utils.tensorboard` imports.  `--startIter N` loads `Model_{N:06d}.pth` as the reference intends (its own call is broken) and
advances the schedule to N; the optimiser state starts fresh, because the reference never saved it -- unless the run that wrote
the checkpoint had `--saveOpt`: then `Opt_{N:06d}.pth` (the name the reference's own resume asks for, :163) lies beside it with
`opt_G.state_dict()` and the state of the crop draws' generator, both are loaded, and the run goes on exactly where the other stood.
`--deterministic` trains on `mulut_net_stage_backward_exact`: the input gradient of a stage is gathered in a fixed order, so with
`--seed` two runs write the same `Model_*.pth`, tensor for tensor (it has no meaning for `--torchPath` and is refused with it).
`--valResident` keeps the validation sets on the device for the whole run (`net_val.NetValSet`, built once before the loop under half
the free device memory; a set that needs more is said and validated by `net_valid_steps`): a point is then one list launch of the
cascade per stage and dataset (`NetPlan.run`) and one read-back of the results, scored with the host loop's arithmetic and encoded
behind the loop on `--valWorkers` threads, per `--valSave every|last|never`; the writer is joined, and a failed write raised, before `Complete`.
`--gpuNum > 1` is refused.
"""
import math
import os
import time

import torch
import torch.nn.functional as F
import torch.optim as optim

from . import network
from .ft_data import CropProvider, DeviceCropProvider, TrainingSetTooLarge
from .net_engine import NetEngine
from .net_train import NetTrainer, torch_predict
from .ft_val import ValidationSetTooLarge
from .net_val import NetValSet, net_valid_steps, resident_net_valid_steps
from .options import TrainOptions


def save_checkpoint(model_G, opt, i, log, opt_G=None, train_iter=None):
    """sr/1_train_model.py:58-67; with --saveOpt also what an exact resume needs: the optimiser's state and the state of the crop
    draws' generator as it stands before the draw of iteration i + 1."""
    torch.save(model_G, os.path.join(opt.expDir, 'Model_{:06d}{}.pth'.format(i, '')))
    if opt.saveOpt:
        torch.save({"opt_G": opt_G.state_dict(), "rng": train_iter.rng.getstate()}, os.path.join(opt.expDir, 'Opt_{:06d}.pth'.format(i)))
    log("Checkpoint saved {}".format(str(i)))


def resident_val_set(opt, log=print):
    """--valResident: the validation sets on the device, built once, under half the free device memory; None, and said, if they
    need more -- the run then validates with net_valid_steps."""
    try:
        return NetValSet(opt, max_bytes=torch.cuda.mem_get_info()[0] // 2, workers=opt.valWorkers)
    except ValidationSetTooLarge as e:
        log("{} | validation set of {} bytes exceeds half the free device memory ({}): validation runs on the host loop".format(opt.expDir, e.nbytes, e.limit))
        return None


def train(opt, log=print):
    if opt.gpuNum > 1:
        raise SystemExit("--gpuNum {}: this driver trains on one GPU (DataParallel is out of scope)".format(opt.gpuNum))
    if opt.deterministic and opt.torchPath:
        raise SystemExit("--deterministic selects a backward of the fused HIP kernels and cannot be combined with --torchPath")
    try:
        from torch.utils.tensorboard import SummaryWriter
        writer = SummaryWriter(log_dir=opt.expDir)
    except Exception:
        writer = None
        log("{} | torch.utils.tensorboard is not available: TensorBoard scalars are skipped".format(opt.expDir))
    if opt.seed is not None:
        torch.manual_seed(opt.seed)
    modes, stages = [m for m in opt.modes], opt.stages
    model_G = getattr(network, opt.model)(nf=opt.nf, scale=opt.scale, modes=modes, stages=stages).cuda()
    params_G = list(filter(lambda p: p.requires_grad, model_G.parameters()))
    opt_G = optim.Adam(params_G, lr=opt.lr0, betas=(0.9, 0.999), eps=1e-8, weight_decay=opt.weightDecay, amsgrad=False)
    if opt.lr1 < 0:
        lf = lambda x: (((1 + math.cos(x * math.pi / opt.totalIter)) / 2) ** 1.0) * 0.8 + 0.2   # noqa: E731
    else:
        lr_b = opt.lr1 / opt.lr0
        lr_a = 1 - lr_b
        lf = lambda x: (((1 + math.cos(x * math.pi / opt.totalIter)) / 2) ** 1.0) * lr_a + lr_b   # noqa: E731
    resume = None
    if opt.startIter > 0:      # :158-164 as intended: the module's parameters; the schedule goes on from startIter
        lm = network.load_checkpoint(os.path.join(opt.expDir, 'Model_{:06d}.pth'.format(opt.startIter)))
        model_G.load_state_dict(lm.state_dict(), strict=True)
        opt_path = os.path.join(opt.expDir, 'Opt_{:06d}.pth'.format(opt.startIter))
        if os.path.exists(opt_path):      # --saveOpt wrote it: the optimiser goes on where it stood, and below the crop draws do
            resume = torch.load(opt_path, map_location=next(model_G.parameters()).device, weights_only=False)
            opt_G.load_state_dict(resume["opt_G"])
            log("{} | optimiser state loaded from {}".format(opt.expDir, opt_path))
    start = opt.startIter
    scheduler = optim.lr_scheduler.LambdaLR(opt_G, lr_lambda=lambda x: lf(x + start))
    trainer = None if opt.torchPath else NetTrainer(model_G, deterministic=opt.deterministic)
    if opt.deterministic:
        log("{} | deterministic backward: the input gradient of every stage is gathered per pixel in a fixed order{}".format(
            opt.expDir, "" if opt.seed is not None else " (no --seed: the weights and the draws are not fixed)"))
    if opt.hostData:
        train_iter = CropProvider(opt.trainDir, opt.scale, opt.cropSize, opt.batchSize, opt.seed, log=log)
    else:
        try:
            train_iter = DeviceCropProvider(opt.trainDir, opt.scale, opt.cropSize, opt.batchSize, opt.seed,
                                            max_bytes=torch.cuda.mem_get_info()[0] // 2, log=log)
        except TrainingSetTooLarge as e:
            log("{} | training set of {} bytes exceeds half the free device memory ({}): batches are cut on the host".format(opt.expDir, e.nbytes, e.limit))
            train_iter = e.host
    if resume is not None:
        train_iter.rng.setstate(resume["rng"])
    engine = None
    if not os.path.isdir(opt.valDir):      # (the reference's SRBenchmark would fail here; a run without validation sets is allowed, and said)
        log("{} | valDir {} is not a directory: validation is skipped".format(opt.expDir, opt.valDir))
    vset = resident_val_set(opt, log) if opt.valResident and os.path.isdir(opt.valDir) else None
    l_accum = [0., 0., 0.]
    dT = 0.
    rT = 0.
    accum_samples = 0
    losses = []
    opt.lrTrace = []      # the learning rate of every iteration run, for callers
    try:
        for i in range(opt.startIter + 1, opt.totalIter + 1):
            model_G.train()
            st = time.time()
            im, lb = train_iter.next()
            dT += time.time() - st

            st = time.time()
            opt_G.zero_grad()
            opt.lrTrace.append(opt_G.param_groups[0]['lr'])
            pred = torch_predict(model_G, im, modes, stages, 'train') if trainer is None else trainer.predict(im, 'train')
            loss_G = F.mse_loss(pred, lb)
            loss_G.backward()
            opt_G.step()
            scheduler.step()
            rT += time.time() - st

            accum_samples += opt.batchSize
            losses.append(loss_G.item())
            l_accum[0] += losses[-1]
            if i % opt.displayStep == 0:
                if writer is not None:
                    writer.add_scalar('loss_Pixel', l_accum[0] / opt.displayStep, i)
                log("{} | Iter:{:6d}, Sample:{:6d}, GPixel:{:.2e}, dT:{:.4f}, rT:{:.4f}".format(
                    opt.expDir, i, accum_samples, l_accum[0] / opt.displayStep, dT / opt.displayStep, rT / opt.displayStep))
                l_accum = [0., 0., 0.]
                dT = 0.
                rT = 0.
            if i % opt.saveStep == 0:
                save_checkpoint(model_G, opt, i, log, opt_G, train_iter)
            if i % opt.valStep == 0 and os.path.isdir(opt.valDir):
                if engine is None:
                    engine = NetEngine(model_G, device=next(model_G.parameters()).device.index)
                engine.load_weights(model_G)
                res = net_valid_steps(engine, opt, i, log) if vset is None else resident_net_valid_steps(engine, vset, opt, i, log)
                if writer is not None:
                    for ds, psnrs in res.items():
                        writer.add_scalar('PSNR_valid/{}'.format(ds), float(psnrs.mean()), i)
                    writer.flush()
        if vset is not None:      # the files of the last point are on disk, or the writer's failure is raised here
            vset.join()
    finally:      # (also when a step or a point raised: the set's threads, plans and pinned buffer do not wait for the collector)
        if vset is not None:
            vset.close()
    log("Complete")
    if engine is not None:
        engine.close()
    if trainer is not None:
        trainer.close()
    return model_G, losses


def main(argv=None):
    opt_inst = TrainOptions()
    opt = opt_inst.parse(argv)
    return train(opt)


if __name__ == "__main__":
    main()
