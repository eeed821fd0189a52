"""k_ira_lay (csrc/ira_lay.hip, schedule="layered" on an IRA graph) against the numpy float32 restatement of its
specification (tests/ira_layered_ref.py): bits, z (as bit patterns) and iters_used are equal bit for bit.  Small
IRA codes from hand-written tables of (row, shift) per group: "plain" has no repeated group, rows of 3, 2, 2 and 1
slots and shifts whose gather windows wrap; "pairs" has two groups that meet a row twice (shift differences 43 and
77, no divisors of 360); "wide7" / "wide9" have a row of 7 / 9 slots (the 8- and 24-slot kernels) at q = 2."""
import functools

import numpy as np
import pytest

from ira_layered_ref import ira_layered_ms_f32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ldpc_amd  # noqa: E402
from ldpc_amd import _abi  # noqa: E402
from ldpc_amd.codes import IRAEncoder, _ira_code, get_code  # noqa: E402

TABLES = {
    "plain": (4, [[(0, 0), (1, 17), (2, 359)], [(0, 200), (1, 1), (3, 77)], [(0, 359), (2, 100)]]),
    "pairs": (3, [[(0, 5), (0, 48), (1, 7)], [(0, 0), (2, 300), (1, 359)], [(1, 11), (2, 2)], [(0, 123), (2, 0), (2, 77)]]),
    "wide7": (2, [[(0, 37 * i % 360)] + [(1, 11 * i)] * (i % 2) for i in range(7)]),
    "wide9": (2, [[(0, 37 * i % 360)] + [(1, 11 * i)] * (i % 2) for i in range(9)]),
    "triple": (2, [[(0, 1), (0, 50), (0, 200), (1, 3)], [(1, 0)]]),
    "big": (6, [[(i % 6, i)] for i in range(120)]),          # k = 43,200 floats: more than a workgroup's LDS
}
NORMS = ((1.0, 0.0, 20.0), (0.75, 0.0, 20.0), (1.0, 0.5, 20.0), (0.8125, 0.25, 4.0))  # as test_gpu_layered.py
EBN0 = 3.0   # dB: the small codes' waterfall


@functools.lru_cache(None)
def _code(name):
    if name == "dvbs2_12":
        return 90, get_code(name)[0]
    q, t = TABLES[name]
    return q, _ira_code([[a + q * s for a, s in g] for g in t], name, n=(len(t) + q) * 360, k=len(t) * 360, q=q)


@functools.lru_cache(None)
def _llr(name, B=8, ebn0=EBN0):
    q, H = _code(name)
    rng = np.random.default_rng(11)
    cw = IRAEncoder(H).encode(rng.integers(0, 2, size=(B, H.k)))
    sigma = np.sqrt(1.0 / (2 * (H.k / H.n) * 10 ** (ebn0 / 10)))
    llr = (-2.0 * ((1.0 - 2.0 * cw) + sigma * rng.standard_normal(cw.shape)) / sigma**2).astype(np.float32)
    llr.setflags(write=False)
    return llr


def _check(name, x, iters, norm=NORMS[0], early_stop=False, how="device"):
    q, H = _code(name)
    alpha, beta, clamp = norm
    ref = ira_layered_ms_f32(H, q, x, iters, clamp, alpha, beta, early_stop)
    kw = dict(algo="minsum", clamp=clamp, alpha=alpha, beta=beta, early_stop=early_stop, soft="z", want_iters=True,
              schedule="layered")
    dec = ldpc_amd.get_decoder(H)
    if how == "host":
        r = dec.decode(x.copy(), iters, **kw)
    else:
        side = torch.cuda.Stream() if how == "side_stream" else None
        r = dec.decode(torch.from_numpy(x.copy()).cuda(), iters, stream=side, **kw)
        (side or torch.cuda.current_stream()).synchronize()
    bits, z, used = (np.asarray(r[k].cpu() if hasattr(r[k], "cpu") else r[k]) for k in ("bits", "soft", "iters_used"))
    assert np.array_equal(used, ref["iters_used"]), (used, ref["iters_used"])
    bad = z.view(np.uint32) != ref["z"].view(np.uint32)
    assert not bad.any() and np.array_equal(bits, ref["bits"]), (int(bad.sum()), np.argwhere(bad)[:4], z[bad][:4])
    return ref


# 0: stored from the load frame; 1: no hand-over; 2: first row-(q-1) -> row-0 hand-over; 7: steady state
@pytest.mark.parametrize("iters", (0, 1, 2, 7))
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("name", ("plain", "pairs", "wide7", "wide9"))
def test_fixed_count_bitwise(name, B, iters):
    ref = _check(name, _llr(name)[:B], iters)
    if name == "pairs" and iters:
        # conditions on the input: the repeat exists, and the two-edge sum is not the two updates in a row
        q, H = _code(name)
        rows = [(g, x % q) for g, xs in enumerate(H.info_groups) for x in xs if x >= 0]
        assert len(set(rows)) < len(rows) and ref["pair_differs"] > 0


@pytest.mark.parametrize("norm", NORMS)
def test_normalised_offset_clamped(norm):
    _check("pairs", _llr("pairs")[:3], 2, norm)


def test_persistent_loop_and_workspace(monkeypatch):
    # five codewords over two slots: a slot's workspace is reused without a clear, and is per slot, not per codeword
    monkeypatch.setenv("LDPC_IRA_LAY_SLOTS", "2")
    _check("pairs", _llr("pairs")[:5], 2)
    dec = ldpc_amd.get_decoder(_code("pairs")[1])
    p = dec.params(2, "minsum", 20.0, device_ptrs=True, schedule="layered")
    assert 0 < dec.workspace_bytes(2, p) == dec.workspace_bytes(5, p) == dec.workspace_bytes(4096, p)
    assert dec.workspace_bytes(1, p) < dec.workspace_bytes(2, p)


@pytest.mark.parametrize("iters", (1, 2))
def test_signed_zeros_and_saturating_llrs(iters):
    x = _llr("pairs")[:4].copy()
    mask = np.random.default_rng(iters).random(x.shape)
    for lo, hi, val in ((0, 0.02, 0.0), (0.02, 0.04, -0.0), (0.04, 0.045, 1e30), (0.045, 0.05, -1e30)):
        x[(mask >= lo) & (mask < hi)] = val
    _check("pairs", x, iters)


@pytest.mark.parametrize("how", ["host", "side_stream"])
def test_early_stop_bitwise(how):
    used = _check("pairs", _llr("pairs"), 10, early_stop=True, how=how)["iters_used"]
    # conditions on the inputs: codewords stop at different sweeps, and one never does
    assert len(set(used[used < 10].tolist())) >= 2 and (used == 10).any(), used


@pytest.mark.parametrize("iters", (1, 2))
def test_dvbs2_rate_half(iters):
    # the real table at full size: 8 rows with a repeated group, 129,600 bytes of posteriors in LDS
    assert _check("dvbs2_12", _llr("dvbs2_12", 2, 1.0), iters)["pair_differs"] > 0


def test_kernel_path():
    dec = ldpc_amd.get_decoder(_code("plain")[1])
    assert dec.kernel_path(dec.params(25, "minsum", 20.0, schedule="layered")) == "ira-z360-layered"
    assert dec.kernel_path(dec.params(25, "minsum", 20.0)) == "ira-z360"


@pytest.mark.parametrize("name,kw,says", [("big", dict(algo="minsum"), str(160 * 1024)), ("triple", dict(algo="minsum"), "three"),
                                          ("plain", dict(algo="tanh"), "tanh"), ("plain", dict(algo="qms"), "quantized")])
def test_refused(name, kw, says):
    H = _code(name)[1]
    with pytest.raises(_abi.LdpcError) as e:
        ldpc_amd.get_decoder(H).decode(np.ones((2, H.n), np.float32), 5, schedule="layered", **kw)
    assert e.value.code == _abi.LDPC_EUNSUPPORTED and "LDPC_F_LAYERED is not implemented for" in str(e.value)
    assert says in str(e.value), str(e.value)
