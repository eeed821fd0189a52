"""Layered (row-serial) min-sum in numpy float32 for any H: a plain restatement of the LDPC_F_LAYERED
specification (include/ldpc_abi.h), vectorised over codewords, every step one float32 operation in the stated
order.  The checker of tests/test_gpu_layered.py; nothing in the library uses it."""
import numpy as np

from ldpc_amd.codes import Graph

F = np.float32
ZTHR = np.array([0xB43FFFFF], np.uint32).view(F)[0]   # the fp32 hard-decision threshold (csrc/common.h kZthrF32)


def layered_ms_f32(H, llr, iters, clamp, alpha=1.0, beta=0.0, early_stop=False):
    g = H if isinstance(H, Graph) else Graph.from_H(H)
    rp, ci = np.asarray(g.row_ptr), np.asarray(g.col_idx)
    clamp, alpha, beta = F(clamp), F(alpha), F(beta)
    llr = np.asarray(llr, F)
    B = llr.shape[0]
    app = -llr + F(0.0)
    c2v = np.zeros((B, g.E), F)
    used = np.full(B, iters, np.int32)
    run = np.ones(B, bool)                          # codewords still decoding; a stopped one stays frozen
    for it in range(iters):
        if not run.any():
            break
        a, m = app[run], c2v[run]
        k = np.arange(a.shape[0])
        for c in range(g.m):
            e = slice(rp[c], rp[c + 1])
            v = ci[e]
            t = a[:, v] - m[:, e]
            mag = np.abs(t)
            two = np.partition(mag, 1, axis=1) if mag.shape[1] > 1 else np.c_[mag, np.full_like(mag, np.inf)]
            mm = np.repeat(two[:, :1], mag.shape[1], axis=1)
            mm[k, np.argmin(mag, axis=1)] = two[:, 1]
            out = np.minimum(clamp, np.maximum(alpha * mm - beta, F(0.0)))
            sb = np.signbit(t)
            new = np.where(np.logical_xor.reduce(sb, axis=1)[:, None] ^ sb, -out, out)
            m[:, e] = new
            a[:, v] = t + new
        app[run], c2v[run] = a, m
        if early_stop:
            hard = (app <= F(2.0) * ZTHR).astype(np.int64)
            ok = run & ~(np.add.reduceat(hard[:, ci], rp[:-1], axis=1) & 1).any(axis=1)
            used[ok] = it + 1
            run &= ~ok
    z = F(0.5) * app
    assert z.dtype == F
    return dict(bits=(z <= ZTHR).astype(np.uint8), z=z, iters_used=used)
