"""Writes tests/golden/wnmf_mask.npz: W, H and cost of the float64 statement tests/wnmf_oracle.py for the (7, 5, 3) and (70, 90, 5) mask cases of
tests/wnmf_inputs.py, all three divergences, 30 iterations with the stop rule off.  tests/test_gpu_wnmf.py::test_golden compares the HIP path with them.

    python tests/golden/make_wnmf_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import wnmf_inputs as I  # noqa: E402


def main():
    out = {}
    for shape in [(7, 5, 3), (70, 90, 5)]:
        for div in I.DIVS:
            W, H, c = I.oracle(shape, "mask", div)
            key = "%dx%dx%d_%s_" % (shape + (div,))
            out[key + "W"], out[key + "H"], out[key + "cost"] = W, H, c
    np.savez(os.path.join(HERE, "wnmf_mask.npz"), **out)


if __name__ == "__main__":
    main()
