#!/usr/bin/env python3
"""The reference's script of the same name with its two hard-coded paths as arguments:

    cd sr && python Test_dataset.py ../data/Test/HR ../data/Test

writes ../data/Test/LR/X{2,3,4}/<stem>x{scale}.png, the bytes Pillow's bicubic resize gives, made on the GPU.
Everything happens in mulut_amd.resample (``--layout benchmark`` writes LR_bicubic/X{scale}/<stem>.png instead)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mulut_amd.resample import main  # noqa: E402

if __name__ == "__main__":
    main()
