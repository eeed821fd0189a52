"""k_qc_ms_lay (csrc/qc_lay.hip, schedule="layered") against the numpy float32 restatement of its specification
(tests/layered_ref.py): bits, z (as bit patterns) and iters_used are equal bit for bit — the schedule reorders
no sum, so there is nothing to tolerate.  Inputs: encoded codewords over BPSK/AWGN in each code's waterfall."""
import functools

import numpy as np
import pytest

from layered_ref import layered_ms_f32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ldpc_amd  # noqa: E402
from ldpc_amd import _abi  # noqa: E402
from ldpc_amd.codes import Encoder, get_code  # noqa: E402

EBN0 = {"wifi648_12": 1.6, "wifi1296_23": 2.2}   # dB, where 12 sweeps decode some codewords and not others
# B = 1: an empty half-wave (Z = 27); 3: odd; 9: past one 256-thread block at two codewords per wave (Z = 54: at 5)
BATCHES = (1, 3, 9)
# 0: stored straight from the load frame; 1: no hand-over; 2: first last-row -> first-row hand-over; 7: steady state
ITERS = (0, 1, 2, 7)
NORMS = ((1.0, 0.0, 20.0), (0.75, 0.0, 20.0), (1.0, 0.5, 20.0), (0.8125, 0.25, 4.0))  # the four NORM kernels; clamp active


@functools.lru_cache(None)
def _llr(name):
    H, _ = get_code(name)
    enc = Encoder(H)
    rng = np.random.default_rng(11)
    cw = enc.encode(rng.integers(0, 2, size=(max(BATCHES), enc.k)))
    sigma = np.sqrt(1.0 / (2 * (enc.k / H.shape[1]) * 10 ** (EBN0[name] / 10)))
    llr = (-2.0 * ((1.0 - 2.0 * cw) + sigma * rng.standard_normal(cw.shape)) / sigma**2).astype(np.float32)
    llr.setflags(write=False)
    return H, llr


def _same(r, ref):
    bits, z, used = (np.asarray(r[k].cpu() if hasattr(r[k], "cpu") else r[k]) for k in ("bits", "soft", "iters_used"))
    assert np.array_equal(used, ref["iters_used"]), (used, ref["iters_used"])
    bad = z.view(np.uint32) != ref["z"].view(np.uint32)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4], z[bad][:4], ref["z"][bad][:4])
    assert np.array_equal(bits, ref["bits"])


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", sorted(EBN0))
def test_fixed_count_bitwise(name, B, iters, norm):
    H, llr = _llr(name)
    alpha, beta, clamp = norm
    dec = ldpc_amd.get_decoder(H)
    r = dec.decode(torch.from_numpy(llr[:B].copy()).cuda(), iters, algo="minsum", clamp=clamp, alpha=alpha, beta=beta,
                   soft="z", want_iters=True, schedule="layered")
    _same(r, layered_ms_f32(H, llr[:B], iters, clamp, alpha, beta))


@pytest.mark.parametrize("how", ["host", "side_stream"])
@pytest.mark.parametrize("name", sorted(EBN0))
def test_early_stop_bitwise(name, how):
    H, llr = _llr(name)
    ref = layered_ms_f32(H, llr, 12, 20.0, early_stop=True)
    # a condition on the inputs: codewords stop at different sweeps, and one never does
    assert len(set(ref["iters_used"].tolist())) >= 2 and (ref["iters_used"] == 12).any(), ref["iters_used"]
    assert (ref["iters_used"] < 12).any()
    dec = ldpc_amd.get_decoder(H)
    kw = dict(algo="minsum", clamp=20.0, early_stop=True, soft="z", want_iters=True, schedule="layered")
    if how == "host":
        r = dec.decode(llr, 12, **kw)
    else:
        side = torch.cuda.Stream()
        r = dec.decode(torch.from_numpy(llr.copy()).cuda(), 12, stream=side, **kw)
        side.synchronize()
    _same(r, ref)


def test_kernel_path():
    dec = ldpc_amd.get_decoder(get_code("wifi648_12")[0])
    assert dec.kernel_path(dec.params(25, "minsum", 20.0, schedule="layered")) == "qc-z27-layered"
    assert dec.kernel_path(dec.params(25, "minsum", 20.0)) == "qc-z27"


@pytest.mark.parametrize("name,kw", [("wifi648_12", dict(algo="tanh")), ("wifi648_12", dict(algo="qms")),
                                     ("wifi648_12", dict(algo="minsum", precision="f64")),
                                     ("wifi648_12", dict(algo="minsum", force_generic=True)),
                                     ("wifi1944_56", dict(algo="minsum")), ("peg64_32", dict(algo="minsum"))])
def test_unsupported_combinations(name, kw):
    H, _ = get_code(name)
    dec = ldpc_amd.get_decoder(H)
    with pytest.raises(_abi.LdpcError) as e:
        dec.decode(np.ones((2, H.shape[1]), np.float32), 5, schedule="layered", **kw)
    assert e.value.code == _abi.LDPC_EUNSUPPORTED and "LDPC_F_LAYERED" in str(e.value)
