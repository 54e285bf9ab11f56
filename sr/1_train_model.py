#!/usr/bin/env python3
"""Drop-in for the reference's `python 1_train_model.py --stages 2 --modes sdy -e <expDir>` (run from sr/): trains the SR network
on the fused HIP forward and backward kernels (mulut_amd.train_model).  `--torchPath` runs the same loop on torch operators."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mulut_amd.train_model import main  # noqa: E402

if __name__ == "__main__":
    main()
