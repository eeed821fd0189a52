"""Layered (row-serial) tanh sum-product in numpy float64 for any H: a plain restatement of the LDPC_F_LAYERED /
LDPC_ALGO_TANH_SP specification (include/ldpc_abi.h), vectorised over codewords.  The checker of
tests/test_gpu_layered_sp.py; nothing in the library uses it."""
import numpy as np

from ldpc_amd.codes import Graph

RMAX = 16777215.0                                   # the fp32 module's p clamp: |p| <= (RMAX - 1) / (RMAX + 1)


def layered_sp_f64(H, llr, iters, clamp, early_stop=False):
    g = H if isinstance(H, Graph) else Graph.from_H(H)
    rp, ci = np.asarray(g.row_ptr), np.asarray(g.col_idx)
    cap, pmax = min(float(clamp), np.log(RMAX)), (RMAX - 1.0) / (RMAX + 1.0)
    app = -np.asarray(llr, np.float64)
    B = app.shape[0]
    c2v = np.zeros((B, g.E))
    used = np.full(B, iters, np.int32)
    run = np.ones(B, bool)                          # codewords still decoding; a stopped one stays frozen
    for it in range(iters):
        if not run.any():
            break
        a, m = app[run], c2v[run]
        for c in range(g.m):
            e = slice(rp[c], rp[c + 1])
            s = a[:, ci[e]] - m[:, e]
            t = np.tanh(0.5 * s)
            one = np.ones((t.shape[0], 1))
            pre = np.cumprod(np.c_[one, t[:, :-1]], axis=1)                    # prod of the edges before
            suf = np.cumprod(np.c_[one, t[:, :0:-1]], axis=1)[:, ::-1]         # ... and of those after
            p = np.clip(pre * suf, -pmax, pmax)
            new = np.clip(np.log((1.0 + p) / (1.0 - p)), -cap, cap)
            m[:, e] = new
            a[:, ci[e]] = s + new
        app[run], c2v[run] = a, m
        if early_stop:
            hard = (app < 0).astype(np.int64)
            ok = run & ~(np.add.reduceat(hard[:, ci], rp[:-1], axis=1) & 1).any(axis=1)
            used[ok] = it + 1
            run &= ~ok
    z = 0.5 * app
    return dict(bits=(z < 0).astype(np.uint8), z=z, iters_used=used)
