#!/usr/bin/env python3
"""Generate tests/golden/cmfwisa_*.npz from the float64 oracle tests/cmfwisa_oracle.py (cmfwisa.m restated in numpy).

Inputs are regenerated from seeds by tests/cmfwisa_inputs.py and are not stored except where noted; every fixture carries `stamp`, the
SHA-256 of the oracle's source it was made with (tests/test_cmfwisa_host.py checks it against the oracle in the tree).

    PYTHONPATH=. python tests/golden/make_cmfwisa_golden.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from cmfwisa_inputs import CASES, case_inputs  # noqa: E402
import cmfwisa_oracle as CO  # noqa: E402


def stamp():
    with open(os.path.join(os.path.dirname(HERE), "cmfwisa_oracle.py"), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def main():
    for name in CASES:
        V, Ks, cfg = case_inputs(name)
        W, H, P, cost = CO.cmfwisa(V, Ks, cfg)
        P = P if isinstance(P, list) else [P]
        sub = 8 if V.size > 200000 else 1
        Vhat = sum((W[i] @ H[i]) * P[i] for i in range(len(Ks)))
        # the oracle's own movement when V, W_init, H_init and P_init are rounded to fp32 once: the bar where it exceeds the contract
        r32 = lambda x: x.astype(np.complex64).astype(np.complex128) if np.iscomplexobj(x) else x.astype(np.float32).astype(np.float64)
        c32 = dict(cfg, W_init=[r32(np.asarray(w)) for w in cfg["W_init"]], H_init=[r32(np.asarray(h)) for h in cfg["H_init"]])
        if "P_init" in cfg:
            c32["P_init"] = [r32(p) for p in cfg["P_init"]]
        W2, H2, P2, cost2 = CO.cmfwisa(r32(np.asarray(V)), Ks, c32)
        P2 = P2 if isinstance(P2, list) else [P2]
        rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
        # (P and V_hat on the same every-sub-th grid the fixture stores and the tests compare: the P error is heavy-tailed, a few ill-conditioned elements)
        Vhat2 = sum((W2[i] @ H2[i]) * P2[i] for i in range(len(Ks)))
        sens = np.array([max(rel(a, b) for a, b in zip(W2, W)), max(rel(a, b) for a, b in zip(H2, H)),
                         max(rel(a[::sub, ::sub], b[::sub, ::sub]) for a, b in zip(P2, P)),
                         np.max(np.abs(cost2 - cost) / cost) if len(cost2) == len(cost) else np.inf, rel(Vhat2[::sub, ::sub], Vhat[::sub, ::sub])])
        np.savez_compressed(os.path.join(HERE, "cmfwisa_%s.npz" % name), stamp=np.array(stamp()), sub=np.array(sub), W=np.hstack(W), H=np.vstack(H),
                            P=np.stack([p[::sub, ::sub] for p in P], axis=2), Vhat=Vhat[::sub, ::sub], cost=cost, sens_WHPcV=sens)
        print(name, V.shape, Ks, "cost len", len(cost), "sub", sub, "fp32-input sensitivity W H P cost V_hat", sens)


if __name__ == "__main__":
    main()
