"""Writes tests/golden/wcnmf_mask.npz: W, H and cost of the float64 statement tests/wcnmf_oracle.py for the (7, 5, 3, 2) and (70, 90, 5, 4) mask cases of
tests/wcnmf_inputs.py, all three divergences, 30 iterations with the stop rule off.  tests/test_gpu_wcnmf.py::test_golden compares the HIP path with them and
tests/test_wcnmf_host.py::test_golden_is_the_statement the statement.

    python tests/golden/make_wcnmf_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import wcnmf_inputs as I  # noqa: E402

SHAPES = [(7, 5, 3, 2), (70, 90, 5, 4)]


def main():
    out = {}
    for shape in SHAPES:
        for div in I.DIVS:
            W, H, c = I.oracle(shape, "mask", div)
            key = "%s_%s_" % (I.ident(shape), div)
            out[key + "W"], out[key + "H"], out[key + "cost"] = W, H, c
    np.savez(os.path.join(HERE, "wcnmf_mask.npz"), **out)


if __name__ == "__main__":
    main()
