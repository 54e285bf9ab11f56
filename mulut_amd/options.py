"""The reference's test-time command line (common/option.py:15-29,189-199), kept flag for flag.

Deviations, both documented in DESIGN.md:
  * ``parse()`` does not copy every ``*.py`` under cwd into ``<expDir>/code`` (common/option.py:104-110,155-156);
    pass ``--saveCode`` to get that side effect back.  ``--debug`` is accepted and means what it meant.
  * new optional flags (``--device``, ``--datasets``, ``--batch``, ``--ioWorkers``, ``--timing``, ``--bicubicBaseline``) default to the reference's behaviour.
    ``--bicubicBaseline`` takes effect here: ``parse()`` has ``mulut_amd.resample.add_baseline_line`` wrap the test script's
    ``eltr.run``, which then prints one more line per dataset behind the summary; ``mulut_amd/test_lut.py`` itself is as it was.
"""
import argparse
import os


class TestOptions:
    def __init__(self, debug=False):
        self.debug = debug
        self.isTrain = False

    def initialize(self, parser):
        # experiment specifics (BaseOptions.initialize, common/option.py:13-31)
        parser.add_argument('--model', type=str, default='SRNets')
        parser.add_argument('--task', '-t', type=str, default='sr')
        parser.add_argument('--scale', '-r', type=int, default=4, help="up scale factor")
        parser.add_argument('--sigma', '-s', type=int, default=25, help="noise level")
        parser.add_argument('--qf', '-q', type=int, default=20, help="deblocking quality factor")
        parser.add_argument('--nf', type=int, default=64, help="number of filters of convolutional layers")
        parser.add_argument('--stages', type=int, default=2, help="stages of MuLUT")
        parser.add_argument('--modes', type=str, default='sdy', help="sampling modes to use in every stage")
        parser.add_argument('--interval', type=int, default=4, help='N bit uniform sampling')
        parser.add_argument('--modelRoot', type=str, default='../models')
        parser.add_argument('--expDir', '-e', type=str, default='', help="experiment folder")
        parser.add_argument('--load_from_opt_file', action='store_true', default=False)
        parser.add_argument('--debug', default=False, action='store_true')
        # TestOptions.initialize, common/option.py:190-196
        parser.add_argument('--loadIter', '-i', type=int, default=200000)
        parser.add_argument('--testDir', type=str, default='../data/SRBenchmark')
        parser.add_argument('--resultRoot', type=str, default='../results')
        parser.add_argument('--lutName', type=str, default='LUT_ft')
        # additions
        parser.add_argument('--device', type=int, default=0, help="GPU index")
        parser.add_argument('--datasets', type=str, default='Set5', help="comma separated (reference: ['Set5'])")
        parser.add_argument('--deviceMetrics', action='store_true', default=False,
                            help="score PSNR/SSIM on the GPU (same numbers; saves the host-side SciPy convolutions)")
        parser.add_argument('--ioWorkers', type=int, default=4,
                            help='PNG decode threads ahead of the GPU and encode / score threads behind it (1 = strictly serial)')
        parser.add_argument('--timing', action='store_true', default=False, help='also print end-to-end images/s per dataset')
        parser.add_argument('--bicubicBaseline', action='store_true', default=False,
                            help="after each dataset's summary, also print the PSNR / SSIM of the LR images upscaled by Pillow's "
                                 "bicubic filter on the GPU (the baseline column of an SR table)")
        parser.add_argument('--saveCode', action='store_true', default=False,
                            help="copy *.py under cwd into <expDir>/code like the reference's parse()")
        return parser

    def parse(self, argv=None):
        parser = self.initialize(argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter))
        opt = parser.parse_args([] if self.debug else argv)
        opt.isTrain = False
        opt.flag = opt.scale if "sr" in opt.task else (opt.sigma if "dn" in opt.task else opt.qf if "db" in opt.task else "0")
        if opt.expDir == '':
            # common/option.py:119-131: fresh ../models/debug/expr_N
            opt.modelDir = os.path.join(opt.modelRoot, "debug")
            os.makedirs(opt.modelDir, exist_ok=True)
            count = 1
            while os.path.isdir(os.path.join(opt.modelDir, 'expr_{}'.format(count))):
                count += 1
            opt.expDir = os.path.join(opt.modelDir, 'expr_{}'.format(count))
            os.mkdir(opt.expDir)
        elif not os.path.isdir(opt.expDir):
            os.makedirs(opt.expDir)
        opt.modelPath = os.path.join(opt.expDir, "Model.pth")
        if opt.saveCode and not opt.debug:
            import shutil
            from pathlib import Path
            for f in Path("./").rglob("*.py"):
                trg = os.path.join(opt.expDir, "code", f)
                os.makedirs(os.path.dirname(trg), exist_ok=True)
                shutil.copy(f, trg, follow_symlinks=False)
        if opt.bicubicBaseline:
            # the test script's evaluator, under the name it was started by (python -m mulut_amd.test_lut runs it as __main__)
            import sys
            from .resample import add_baseline_line
            main_mod = sys.modules.get("__main__")
            if getattr(getattr(main_mod, "__spec__", None), "name", None) == "mulut_amd.test_lut":
                add_baseline_line(main_mod.eltr)
            else:
                from . import test_lut
                add_baseline_line(test_lut.eltr)
        self.opt = opt
        return opt


def add_resident_validation(parser):
    """--valResident, --valSave, --valWorkers: the flags, choices and defaults of the fine-tune parser (finetune_lut.build_parser); the
    help says what they do for the network's validation (net_val.NetValSet), which scores on the host where the fine-tune driver's scores on the device."""
    parser.add_argument('--valResident', default=False, action='store_true',
                        help='validate from a device-resident set (NetValSet): decoded and uploaded once per run, one list launch of '
                             'the network per stage and dataset, one read-back of the results per point, scored on the host as '
                             'without the flag, PNGs written behind the loop -- the same log lines, numbers and files as without it')
    parser.add_argument('--valSave', choices=['every', 'last', 'never'], default='every',
                        help='with --valResident: write the PNGs of every validation point, of the final one only, or none')
    parser.add_argument('--valWorkers', type=int, default=4,
                        help='with --valResident: threads that score the results of a point, and as many that encode the PNGs behind the loop')


class TrainOptions:
    """The reference's training command line (common/option.py:13-31,160-187), flag for flag with its defaults, for
    ``mulut_amd.train_model``.  ``parse()`` makes ``expDir`` and ``{expDir}/val`` (``opt.valoutDir``), writes ``opt.txt`` as the
    reference does, applies ``--debug``'s short schedule (:147-151) and, like ``TestOptions``, copies the code only with
    ``--saveCode``.  Additions default to the reference's behaviour: ``--torchPath``, ``--hostData``, ``--seed``, ``--deterministic``, ``--saveOpt``, ``--valResident`` with ``--valSave`` and ``--valWorkers``."""

    def __init__(self, debug=False):
        self.debug = debug
        self.isTrain = True

    def initialize(self, parser):
        parser.add_argument('--model', type=str, default='SRNets')
        parser.add_argument('--task', '-t', type=str, default='sr')
        parser.add_argument('--scale', '-r', type=int, default=4, help="up scale factor")
        parser.add_argument('--sigma', '-s', type=int, default=25, help="noise level")
        parser.add_argument('--qf', '-q', type=int, default=20, help="deblocking quality factor")
        parser.add_argument('--nf', type=int, default=64, help="number of filters of convolutional layers")
        parser.add_argument('--stages', type=int, default=2, help="stages of MuLUT")
        parser.add_argument('--modes', type=str, default='sdy', help="sampling modes to use in every stage")
        parser.add_argument('--interval', type=int, default=4, help='N bit uniform sampling')
        parser.add_argument('--modelRoot', type=str, default='../models')
        parser.add_argument('--expDir', '-e', type=str, default='', help="experiment folder")
        parser.add_argument('--load_from_opt_file', action='store_true', default=False)
        parser.add_argument('--debug', default=False, action='store_true')
        # data
        parser.add_argument('--batchSize', type=int, default=32)
        parser.add_argument('--cropSize', type=int, default=48, help='input LR training patch size')
        parser.add_argument('--trainDir', type=str, default="../data/DIV2K")
        parser.add_argument('--valDir', type=str, default='../data/SRBenchmark')
        # training
        parser.add_argument('--startIter', type=int, default=0,
                            help='Set 0 for from scratch, else will load saved params and trains further')
        parser.add_argument('--totalIter', type=int, default=200000, help='Total number of training iterations')
        parser.add_argument('--displayStep', type=int, default=100, help='display info every N iteration')
        parser.add_argument('--valStep', type=int, default=2000, help='validate every N iteration')
        parser.add_argument('--saveStep', type=int, default=2000, help='save models every N iteration')
        parser.add_argument('--lr0', type=float, default=1e-3)
        parser.add_argument('--lr1', type=float, default=1e-4)
        parser.add_argument('--weightDecay', type=float, default=0)
        parser.add_argument('--gpuNum', '-g', type=int, default=1)
        parser.add_argument('--workerNum', '-n', type=int, default=8)
        # additions
        parser.add_argument('--torchPath', action='store_true', default=False,
                            help="run the network as torch operators (network.SRNets) instead of the fused HIP kernels: the baseline")
        parser.add_argument('--hostData', action='store_true', default=False,
                            help="cut the batches on the host (CropProvider, the reference's path) instead of on the device")
        parser.add_argument('--seed', type=int, default=None, help="seed of the initial weights and of the crops")
        parser.add_argument('--deterministic', action='store_true', default=False,
                            help="bit-reproducible gradients: the input gradient of every stage is gathered per pixel in a fixed "
                                 "order (mulut_net_stage_backward_exact) instead of added with float atomics")
        parser.add_argument('--saveOpt', action='store_true', default=False,
                            help="beside every Model_{i:06d}.pth also write Opt_{i:06d}.pth (the optimiser's state and the crop "
                                 "draws' generator state), which --startIter loads when it exists: an exact resume")
        parser.add_argument('--saveCode', action='store_true', default=False,
                            help="copy *.py under cwd into <expDir>/code like the reference's parse()")
        add_resident_validation(parser)
        return parser

    def parse(self, argv=None):
        parser = self.initialize(argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter))
        opt = parser.parse_args([] if self.debug else argv)
        opt.isTrain = True
        if opt.expDir == '':
            opt.modelDir = os.path.join(opt.modelRoot, "debug")
            os.makedirs(opt.modelDir, exist_ok=True)
            count = 1
            while os.path.isdir(os.path.join(opt.modelDir, 'expr_{}'.format(count))):
                count += 1
            opt.expDir = os.path.join(opt.modelDir, 'expr_{}'.format(count))
            os.mkdir(opt.expDir)
        elif not os.path.isdir(opt.expDir):
            os.makedirs(opt.expDir)
        opt.modelPath = os.path.join(opt.expDir, "Model.pth")
        opt.valoutDir = os.path.join(opt.expDir, 'val')
        os.makedirs(opt.valoutDir, exist_ok=True)
        with open(os.path.join(opt.expDir, 'opt.txt'), 'wt') as opt_file:          # save_options, common/option.py:66-74
            for k, v in sorted(vars(opt).items()):
                default = parser.get_default(k)
                comment = '\t[default: %s]' % str(default) if v != default else ''
                opt_file.write('{:>25}: {:<30}{}\n'.format(str(k), str(v), comment))
        if opt.debug:                                                               # :147-151
            opt.displayStep, opt.saveStep, opt.valStep, opt.totalIter = 10, 100, 50, 200
        if opt.saveCode and not opt.debug:
            import shutil
            from pathlib import Path
            for f in Path("./").rglob("*.py"):
                trg = os.path.join(opt.expDir, "code", f)
                os.makedirs(os.path.dirname(trg), exist_ok=True)
                shutil.copy(f, trg, follow_symlinks=False)
        self.opt = opt
        return opt
