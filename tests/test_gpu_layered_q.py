"""k_qc_qms_lay (csrc/qc_lay_pk.hip, algo="qms" with schedule="layered") against a numpy integer restatement of its
specification (include/ldpc_abi.h, LDPC_F_LAYERED, quantized form): bits, z (by value: zero has no sign there) and
iters_used are equal — the schedule reorders nothing and the arithmetic is exact, so there is nothing to tolerate.
Inputs: encoded codewords over BPSK/AWGN in the (1296,2/3) waterfall."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ldpc_amd  # noqa: E402
from ldpc_amd import _abi  # noqa: E402
from ldpc_amd.codes import Encoder, Graph, get_code  # noqa: E402

NAME, EBN0, F = "wifi1296_23", 2.2, np.float32
BATCHES = (1, 2, 9)     # an empty fp16 half; one full pair; past one 256-thread block (4 pairs) with an odd tail
ITERS = (0, 1, 2, 7)    # stored from the load frame; no hand-over; first last-row -> first-row hand-over; steady state
# (qmax, app_max, beta, qstep): both BETA kernels, a quantizer step, posterior saturation (the last two; with qmax 7
# and beta 2 no posterior of these inputs passes 14, so that case's app_max is 8, not 15)
QUANT = ((15, 127, 0, 1.0), (15, 127, 1, 0.5), (15, 31, 0, 1.0), (7, 8, 2, 1.0))
ES_SWEEPS = 12


def layered_qms_int(H, llr, iters, qmax, app_max, beta, qstep, early_stop=False):
    g = Graph.from_H(H)
    rp, ci = np.asarray(g.row_ptr), np.asarray(g.col_idx)
    q = np.clip(np.rint(np.asarray(llr, F) * (F(1.0) / F(qstep))), -qmax, qmax)   # fp32, as the kernels
    app = -q.astype(np.int64)
    c2v = np.zeros((app.shape[0], g.E), np.int64)
    used = np.full(app.shape[0], iters, np.int32)
    run = np.ones(app.shape[0], bool)               # codewords still decoding; a stopped one stays frozen
    for it in range(iters):
        if not run.any():
            break
        a, m = app[run], c2v[run]
        k = np.arange(a.shape[0])
        for c in range(g.m):
            e = slice(rp[c], rp[c + 1])
            v = ci[e]
            t = a[:, v] - m[:, e]
            mag = np.maximum(np.minimum(np.abs(t), qmax) - beta, 0)
            two = np.partition(mag, 1, axis=1)
            mm = np.repeat(two[:, :1], mag.shape[1], axis=1)
            mm[k, np.argmin(mag, axis=1)] = two[:, 1]
            neg = t < 0
            new = np.where(np.logical_xor.reduce(neg, axis=1)[:, None] ^ neg, -mm, mm)
            m[:, e] = new
            a[:, v] = np.clip(t + new, -app_max, app_max)
        app[run], c2v[run] = a, m
        if early_stop:
            ok = run & ~(np.add.reduceat((app < 0).astype(np.int64)[:, ci], rp[:-1], axis=1) & 1).any(axis=1)
            used[ok] = it + 1
            run &= ~ok
    return dict(bits=(app < 0).astype(np.uint8), z=F(0.5) * app.astype(F), iters_used=used, app=app, unstopped=run)


@functools.lru_cache(None)
def _llr():
    H, _ = get_code(NAME)
    enc = Encoder(H)
    rng = np.random.default_rng(11)
    cw = enc.encode(rng.integers(0, 2, size=(max(BATCHES), enc.k)))
    sigma = np.sqrt(1.0 / (2 * (enc.k / H.shape[1]) * 10 ** (EBN0 / 10)))
    llr = (-2.0 * ((1.0 - 2.0 * cw) + sigma * rng.standard_normal(cw.shape)) / sigma**2).astype(np.float32)
    llr.setflags(write=False)
    return H, llr


def _same(r, ref):
    bits, z, used = (np.asarray(r[k].cpu() if hasattr(r[k], "cpu") else r[k]) for k in ("bits", "soft", "iters_used"))
    assert np.array_equal(used, ref["iters_used"]), (used, ref["iters_used"])
    bad = z != ref["z"]
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4], z[bad][:4], ref["z"][bad][:4])
    assert np.array_equal(bits, ref["bits"])


def _kw(quant, **more):
    qmax, app_max, beta, qstep = quant
    return dict(algo="qms", qmax=qmax, app_max=app_max, beta=float(beta), qstep=qstep, soft="z", want_iters=True,
                schedule="layered", **more)


@pytest.mark.parametrize("quant", QUANT)
@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("B", BATCHES)
def test_fixed_count_equal(B, iters, quant):
    H, llr = _llr()
    ref = layered_qms_int(H, llr[:B], iters, *quant)
    if quant[1] < 127 and iters == 7 and B == max(BATCHES):   # a condition on the inputs: posteriors saturate
        assert (np.abs(ref["app"]) == quant[1]).any()
    r = ldpc_amd.get_decoder(H).decode(torch.from_numpy(llr[:B].copy()).cuda(), iters, **_kw(quant))
    _same(r, ref)


@pytest.mark.parametrize("quant", QUANT[:2])
@pytest.mark.parametrize("how", ["host", "side_stream"])
def test_early_stop_equal(how, quant):
    H, llr = _llr()
    ref = layered_qms_int(H, llr, ES_SWEEPS, *quant, early_stop=True)
    used = ref["iters_used"]
    # conditions on the inputs: codewords stop at different sweeps, one never does, and the two codewords of
    # some fp16 pair stop at different sweeps (the per-half freeze)
    assert len(set(used[~ref["unstopped"]].tolist())) >= 2 and ref["unstopped"].any(), used
    assert (used[0:8:2] != used[1:8:2]).any(), used
    dec = ldpc_amd.get_decoder(H)
    if how == "host":
        r = dec.decode(llr, ES_SWEEPS, **_kw(quant, early_stop=True))
    else:
        side = torch.cuda.Stream()
        r = dec.decode(torch.from_numpy(llr.copy()).cuda(), ES_SWEEPS, stream=side, **_kw(quant, early_stop=True))
        side.synchronize()
    _same(r, ref)


def test_kernel_path():
    dec = ldpc_amd.get_decoder(get_code(NAME)[0])
    assert dec.kernel_path(dec.params(10, "qms", schedule="layered")) == "qc-z54-layered"
    assert dec.kernel_path(dec.params(10, "qms")) == "qc-z54"
    assert dec.kernel_path(dec.params(10, "minsum", schedule="layered")) == "qc-z54-layered"


def test_fp16_bound_is_refused():
    H, llr = _llr()
    with pytest.raises(_abi.LdpcError) as e:
        ldpc_amd.get_decoder(H).decode(llr[:2], 5, algo="qms", qmax=127, app_max=1800, schedule="layered")
    assert e.value.code == _abi.LDPC_EUNSUPPORTED and "LDPC_F_LAYERED" in str(e.value) and "2047" in str(e.value)
