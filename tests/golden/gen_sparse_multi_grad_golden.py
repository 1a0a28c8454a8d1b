#!/usr/bin/env python3
"""Writes tests/golden/sparse_multi_grad_mp_k<kid>.npz: the P = 3 columns' bounds of the sparse (inducing-point) fit and the
gradient of their sum in theta and in the inducing inputs Z, on the (X, Z, theta) of gen_sparse_grad_golden.py's problems (N = 40,
m = 7), by that file's DENSE N x N statement in mpmath at 50 digits, once per column: F = sum_p F_p is linear in the columns, so
its gradient is the sum of theirs -- nothing is shared between the columns here, and nothing of the oracle or the engine is used.
The columns are test_gpu_sparse_multi.add_columns' (inputs only).

   python tests/golden/gen_sparse_multi_grad_golden.py          (needs mpmath; the fixtures are committed, the tests do not)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
sys.path.insert(2, HERE)
import gen_sparse_grad_golden as one        # noqa: E402  (the dense statement of one column)
import test_gpu_sparse_multi as tm          # noqa: E402  (the problem generator of the GPU tests: inputs only)

P = 3

if __name__ == "__main__":
    for kid in range(5):
        pin = np.load(os.path.join(HERE, f"sparse_grad_mp_k{kid}.npz"))
        X, Z, theta = pin["X"], pin["Z"], pin["theta"]
        Y = tm.add_columns(X[None], theta[None], kid, P, 700 + kid)[0]
        cols = [one.dense_gradient(kid, theta, X, y, Z) for y in Y]
        bound = np.array([c[0] for c in cols])
        grad, gradZ = sum(c[1] for c in cols), sum(c[2] for c in cols)
        path = os.path.join(HERE, f"sparse_multi_grad_mp_k{kid}.npz")
        np.savez(path, kid=kid, theta=theta, X=X, Y=Y, Z=Z, bound=bound, grad=grad, gradZ=gradZ, source="mpmath")
        print(path, "bound", bound, "grad", grad)
