"""Layered min-sum on an IRA graph in numpy float32: a plain restatement of the IRA form of the LDPC_F_LAYERED
specification (include/ldpc_abi.h) from the graph's CSR and q alone — layer a = checks {c : c mod q == a}, every
check of a layer from the posteriors as they stood before it, one fp32 operation per step in the stated order.
The checker of tests/test_gpu_ira_layered.py; nothing in the library uses it."""
import numpy as np

from layered_ref import ZTHR, F


def ira_layered_ms_f32(H, q, llr, iters, clamp, alpha=1.0, beta=0.0, early_stop=False):
    rp, ci = np.asarray(H.row_ptr), np.asarray(H.col_idx)
    clamp, alpha, beta = F(clamp), F(alpha), F(beta)
    layers = []
    for a in range(q):
        cs = np.arange(a, H.m, q)
        e = np.concatenate([np.arange(rp[c], rp[c + 1]) for c in cs])
        seg = np.concatenate([[0], np.cumsum(rp[cs + 1] - rp[cs])[:-1]])
        v = ci[e]
        o = np.argsort(v, kind="stable")
        dup = np.flatnonzero(v[o][1:] == v[o][:-1])
        assert not (np.diff(dup) == 1).any(), "a variable with three edges in one layer"
        one = np.ones(len(e), bool)
        one[o[dup]] = one[o[dup + 1]] = False
        layers.append((e, v, seg, np.repeat(np.arange(len(cs)), rp[cs + 1] - rp[cs]), one, o[dup], o[dup + 1]))
    llr = np.asarray(llr, F)
    B = llr.shape[0]
    app = -llr + F(0.0)
    c2v = np.zeros((B, rp[-1]), F)
    used, run = np.full(B, iters, np.int32), np.ones(B, bool)
    differs = 0          # two-edge sums that are not what the two updates one after the other would give
    for it in range(iters):
        if not run.any():
            break
        ap, m = app[run], c2v[run]
        for e, v, seg, sid, one, e1, e2 in layers:
            old = m[:, e]
            t = ap[:, v] - old
            mag = np.abs(t)
            min1 = np.minimum.reduceat(mag, seg, axis=1)[:, sid]
            at = mag == min1
            rest = np.minimum.reduceat(np.where(at, F(np.inf), mag), seg, axis=1)[:, sid]
            min2 = np.where(np.add.reduceat(at.astype(np.int32), seg, axis=1)[:, sid] >= 2, min1, rest)
            out = np.minimum(clamp, np.maximum(alpha * np.where(at, min2, min1) - beta, F(0.0)))
            sb = np.signbit(t)
            new = np.where(np.logical_xor.reduceat(sb, seg, axis=1)[:, sid] ^ sb, -out, out)
            two = ap[:, v[e1]] + ((new[:, e1] - old[:, e1]) + (new[:, e2] - old[:, e2]))
            differs += int(((((t[:, e1] + new[:, e1]) - old[:, e2]) + new[:, e2]).view(np.uint32) != two.view(np.uint32)).sum())
            ap[:, v[one]] = (t + new)[:, one]
            ap[:, v[e1]] = two
            m[:, e] = new
        app[run], c2v[run] = ap, m
        if early_stop:
            hard = (app <= F(2.0) * ZTHR).astype(np.int64)
            ok = run & ~(np.add.reduceat(hard[:, ci], rp[:-1], axis=1) & 1).any(axis=1)
            used[ok] = it + 1
            run &= ~ok
    z = F(0.5) * app
    return dict(bits=(z <= ZTHR).astype(np.uint8), z=z, iters_used=used, pair_differs=differs)
