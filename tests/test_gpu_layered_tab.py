"""k_qc_ms_lay_tab (csrc/qc_lay_tab.hip: schedule="layered" on a quasi-cyclic graph without a compiled table)
against the numpy float32 restatement of the LDPC_F_LAYERED specification (tests/layered_ref.py): bits, z (as bit
patterns) and iters_used are equal bit for bit.  The all-zero codeword over BPSK/AWGN needs no encoder."""
import functools

import numpy as np
import pytest

from layered_ref import layered_ms_f32
from test_gpu_layered import ITERS, NORMS, _same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ldpc_amd  # noqa: E402
from ldpc_amd import _abi  # noqa: E402
from ldpc_amd.codes import Graph, QCCode, qc_expand  # noqa: E402


def qc_base(mb, nb, Z, seed=5, dv=3):
    rng = np.random.default_rng(seed); base = -np.ones((mb, nb), np.int32); kb = nb - mb
    for j in range(kb):
        rows = rng.choice(mb, size=min(dv, mb), replace=False); base[rows, j] = rng.integers(0, Z, size=len(rows))
    for r in range(mb):
        base[r, kb + r] = 0
        if r + 1 < mb: base[r + 1, kb + r] = 0
    return base
def llr0(n, B, rate, ebn0, seed=11):
    rng = np.random.default_rng(seed); s = np.sqrt(1 / (2 * rate * 10 ** (ebn0 / 10)))
    return (-2 * (1 + s * rng.standard_normal((B, n))) / s**2).astype(np.float32)


# (mb, nb, Z) -> Eb/N0 (dB) at which 12 sweeps decode some of 9 codewords and not others.  Z = 7: 36 codewords per
# workgroup, Z odd, 4 idle lanes; 96: 2 per workgroup; 81: row degrees 16-17 (the largest DMAX bucket), a Z the
# compiled tables also use; 300: Z > 256, the position loop
SHAPES = {(4, 8, 7): 0.0, (6, 12, 96): 2.0, (4, 24, 81): 3.0, (3, 6, 300): 2.0}
# B = 1: an almost empty group; CPG + 1: one codeword past a full group; 9: several groups (Z = 7: not one full)
CASES = [(s, B) for s in sorted(SHAPES) for B in (1, max(1, 256 // s[2]) + 1, 9)]


@functools.lru_cache(None)
def _code(shape, dv=3):   # the code and max(9, CPG + 1) LLR rows (the generator's first 9 rows do not depend on B)
    mb, nb, Z = shape
    qc = QCCode(qc_base(mb, nb, Z, dv=dv), Z)
    llr = llr0(qc.n, max(9, 256 // Z + 1), (nb - mb) / nb, SHAPES.get(shape, 2.0))
    llr.setflags(write=False)
    return qc, llr


@functools.lru_cache(None)
def _ref(shape, iters, norm):   # once per (code, sweeps, norm) at the largest batch; codewords are independent
    qc, llr = _code(shape)
    alpha, beta, clamp = norm
    return layered_ms_f32(qc.H(), llr, iters, clamp, alpha, beta)


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("shape,B", CASES)
def test_fixed_count_bitwise(shape, B, iters, norm):
    qc, llr = _code(shape)
    alpha, beta, clamp = norm
    r = ldpc_amd.get_decoder(qc).decode(torch.from_numpy(llr[:B].copy()).cuda(), iters, algo="minsum", clamp=clamp,
                                        alpha=alpha, beta=beta, soft="z", want_iters=True, schedule="layered")
    _same(r, {k: v[:B] for k, v in _ref(shape, iters, norm).items()})


@pytest.mark.parametrize("how", ["host", "side_stream"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_early_stop_bitwise(shape, how):
    qc, llr = _code(shape)
    llr = llr[:9]
    ref = layered_ms_f32(qc.H(), llr, 12, 20.0, early_stop=True)
    # a condition on the inputs: codewords stop at different sweeps, and one never does
    assert len(set(ref["iters_used"].tolist())) >= 2 and (ref["iters_used"] == 12).any(), ref["iters_used"]
    assert (ref["iters_used"] < 12).any()
    dec = ldpc_amd.get_decoder(qc)
    kw = dict(algo="minsum", clamp=20.0, early_stop=True, soft="z", want_iters=True, schedule="layered")
    if how == "host":
        r = dec.decode(llr, 12, **kw)
    else:
        side = torch.cuda.Stream()
        r = dec.decode(torch.from_numpy(llr.copy()).cuda(), 12, stream=side, **kw)
        side.synchronize()
    _same(r, ref)


def test_punctured_columns():
    qc, llr = _code((6, 12, 96))
    llr = llr[:9].copy()
    llr[:, :2 * qc.Z] = 0.0   # block columns 0 and 1 are not transmitted
    r = ldpc_amd.get_decoder(qc).decode(torch.from_numpy(llr).cuda(), 7, algo="minsum", clamp=20.0, soft="z",
                                        want_iters=True, schedule="layered")
    _same(r, layered_ms_f32(qc.H(), llr, 7, 20.0))


@pytest.mark.parametrize("shape", [(4, 8, 1024),     # 86,016 B: above the 64 KiB a kernel gets unasked; 4 positions per thread
                                   (32, 64, 128)])   # 82,432 B per codeword: 256 / Z = 2 do not fit, one does
def test_lds_limits(shape):
    qc, llr = _code(shape)
    r = ldpc_amd.get_decoder(qc).decode(torch.from_numpy(llr[:3].copy()).cuda(), 2, algo="minsum", clamp=20.0, soft="z",
                                        want_iters=True, schedule="layered")
    _same(r, layered_ms_f32(Graph.from_qc(qc.base, qc.Z), llr[:3], 2, 20.0))


def test_entry_points():
    qc, llr = _code((6, 12, 96))
    x = torch.from_numpy(llr[:9].copy()).cuda()
    zs = []
    for H in (qc.H(), Graph.from_qc(qc.base, qc.Z), qc):
        dec = ldpc_amd.get_decoder(H)
        assert dec.kernel_path(dec.params(25, "minsum", 20.0, schedule="layered")) == "qct-z96-layered"
        assert dec.kernel_path(dec.params(25, "minsum", 20.0)) == "generic-csr"
        assert dec.qc_z == 0
        zs.append(dec.decode(x, 7, algo="minsum", clamp=20.0, soft="z", schedule="layered")["soft"].cpu().numpy())
    assert np.array_equal(zs[0].view(np.uint32), zs[1].view(np.uint32))
    assert np.array_equal(zs[0].view(np.uint32), zs[2].view(np.uint32))


@pytest.mark.parametrize("shape,dv,kw,says", [
    ((6, 12, 96), 3, dict(algo="tanh"), ()), ((6, 12, 96), 3, dict(algo="minsum", precision="f64"), ()),
    ((6, 12, 96), 3, dict(algo="minsum", force_generic=True), ()),
    ((2, 30, 8), 2, dict(algo="minsum"), ("29..30",)),              # every information column meets both rows
    ((20, 40, 1024), 3, dict(algo="minsum"), ("413696", "163840")),  # 4 (40960 + 1024) + 12 * 20480 bytes of 160 KiB
])
def test_refused(shape, dv, kw, says):
    qc = _code(shape, dv)[0]
    fdt = np.float64 if kw.get("precision") == "f64" else np.float32
    with pytest.raises(_abi.LdpcError) as e:
        ldpc_amd.get_decoder(qc).decode(np.ones((2, qc.n), fdt), 5, schedule="layered", **kw)
    assert e.value.code == _abi.LDPC_EUNSUPPORTED and "LDPC_F_LAYERED is not implemented for" in str(e.value)
    assert all(s in str(e.value) for s in says), str(e.value)
