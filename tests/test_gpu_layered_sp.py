"""k_qc_sp_lay (csrc/qc_lay_sp.hip, algo="tanh", schedule="layered" on 802.11n (1944,5/6)) against the float64
restatement of its specification (tests/layered_sp_ref.py), held to softparity.TOL = 1e-5; the early-stop kernel
against the fixed-count kernel's own arithmetic, bit for bit.

Checked on the CPU: the checker decodes 8 of the 9 codewords at 7 and 12 sweeps and none at 1 or 2, and stops the
16 early-stop codewords after [7, 12, 6, 8, 9, 6, 10, 12, 12, 12, 12, 12, 3, 12, 12, 5] sweeps."""
import functools
import itertools

import numpy as np
import pytest

from layered_sp_ref import layered_sp_f64
from softparity import TOL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ldpc_amd  # noqa: E402
from ldpc_amd.codes import Encoder, get_code  # noqa: E402

NAME = "wifi1944_56"
# B = 1: one empty half; 3: odd batch; 9: more than one workgroup.  sweeps 0: stored straight from the load;
# 1: no hand-over; 2: first wrap from the last row to the first; 7, 12: steady state, codewords converged.
# clamp 10: the caller's clamp is active; 20: the log RMAX ceiling is.
CASES = [(B, k, c, "z") for B, k, c in itertools.product((1, 3, 9), (0, 1, 2, 7, 12), (10.0, 20.0))] + [(9, 7, 20.0, "p1")]


@functools.lru_cache(None)
def _llr(ebn0, zeros):
    H, _ = get_code(NAME)
    enc = Encoder(H)
    rng = np.random.default_rng(11)
    cw = enc.encode(rng.integers(0, 2, size=(16, enc.k)))
    sigma = np.sqrt(1.0 / (2 * (enc.k / H.shape[1]) * 10 ** (ebn0 / 10)))
    llr = (-2.0 * ((1.0 - 2.0 * cw) + sigma * rng.standard_normal(cw.shape)) / sigma**2).astype(np.float32)
    if zeros:
        llr[0, ::7] = 0.0   # exact zeros: a == 1 edges, decoded by the plain form
    llr.setflags(write=False)
    return H, llr


@functools.lru_cache(None)
def _ref(sweeps, clamp):
    H, llr = _llr(3.3, True)
    r = layered_sp_f64(H, llr[:9], sweeps, clamp)
    ok = ~((r["bits"].astype(np.int64) @ np.asarray(H).T) & 1).any(axis=1)   # codewords the checker decodes
    for v in (r["z"], r["bits"], ok):
        v.setflags(write=False)
    return r["z"], r["bits"], ok


@pytest.mark.parametrize("B,sweeps,clamp,soft", CASES)
def test_fixed_count_f64(B, sweeps, clamp, soft):
    H, llr = _llr(3.3, True)
    z64, b64, ok = _ref(sweeps, clamp)
    if sweeps == 7:
        assert ok.sum() >= 6, ok   # a condition on the inputs
    dec = ldpc_amd.get_decoder(H)
    r = dec.decode(torch.from_numpy(llr[:B].copy()).cuda(), sweeps, algo="tanh", clamp=clamp, soft=soft,
                   want_iters=True, schedule="layered")
    got, bits = r["soft"].cpu().numpy().astype(np.float64), r["bits"].cpu().numpy()
    assert (r["iters_used"].cpu().numpy() == sweeps).all()
    rows = np.arange(B) if sweeps <= 2 else np.flatnonzero(ok[:B])
    want = z64[rows] if soft == "z" else 1.0 - 1.0 / (1.0 + np.exp(-z64[rows]))
    err = np.abs(got[rows] - want) / (np.maximum(1.0, np.abs(want)) if soft == "z" else 1.0)
    print(f"B={B} sweeps={sweeps} clamp={clamp} {soft}: max err {err.max() if err.size else 0.0:.3e}")
    assert (err <= TOL).all(), (err.max(), np.argwhere(err > TOL)[:4])
    if sweeps > 2:
        assert np.array_equal(bits[rows], b64[rows])


def test_early_stop_against_fixed_count():
    H, llr = _llr(3.0, False)
    Hd = np.asarray(H).astype(np.int64)
    used64 = layered_sp_f64(H, llr, 12, 20.0, early_stop=True)["iters_used"]
    # conditions on the inputs: codewords stop at different sweeps, and some never do
    assert len(set(used64.tolist())) >= 2 and (used64 == 12).any() and (used64 < 12).any(), used64
    dec = ldpc_amd.get_decoder(H)
    kw = dict(algo="tanh", clamp=20.0, soft="z", want_iters=True, schedule="layered")
    x = torch.from_numpy(llr.copy()).cuda()
    fixed = [dec.decode(x, k, **kw) for k in range(1, 13)]
    zk = np.stack([f["soft"].cpu().numpy() for f in fixed])
    sat = np.stack([~((f["bits"].cpu().numpy().astype(np.int64) @ Hd.T) & 1).any(axis=1) for f in fixed])   # [k-1][cw]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side = dec.decode(x, 12, stream=side, early_stop=True, **kw)
    side.synchronize()
    for r in (dec.decode(llr, 12, early_stop=True, **kw), on_side):
        z, used = (np.asarray(r[k].cpu() if hasattr(r[k], "cpu") else r[k]) for k in ("soft", "iters_used"))
        assert used.min() >= 1 and used.max() <= 12 and len(set(used.tolist())) >= 2, used
        for i, u in enumerate(used):
            assert np.array_equal(z[i].view(np.uint32), zk[u - 1, i].view(np.uint32)), (i, u)
            assert not sat[:u - 1, i].any(), (i, u, sat[:, i])       # unsatisfied at every sweep before the stop
            assert sat[u - 1, i] or u == 12, (i, u, sat[:, i])       # satisfied at the stop, or never stopped


def test_kernel_path():
    dec = ldpc_amd.get_decoder(get_code(NAME)[0])
    assert dec.kernel_path(dec.params(25, "tanh", 20.0, schedule="layered")) == "qc-z81-layered"
    assert dec.kernel_path(dec.params(50, "tanh", 20.0)) == "qc-z81"
