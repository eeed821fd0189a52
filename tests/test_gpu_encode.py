"""k_qc_encode / k_ira_encode (csrc/encode.hip, Decoder.encode) against the numpy encoders codes.Encoder and
codes.IRAEncoder: the parity part of H is invertible, so the codeword is defined bit for bit and every
comparison is array_equal."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ldpc_amd  # noqa: E402
from ldpc_amd import _abi, sweep  # noqa: E402
from ldpc_amd.codes import Encoder, IRAEncoder, get_code  # noqa: E402

QC = {"wifi648_12": 27, "wifi1296_23": 54, "wifi1944_56": 81}
IRA = ("dvbs2_12", "dvbs2s_12")


@functools.lru_cache(None)
def _qc_case(name):
    """identity (a single 1 at every lifting position of every information column: every rotation, its wrap and
    every row membership), all ones, 8 random rows, one row of bytes in {0..3} (only bit 0 counts)"""
    H, _ = get_code(name)
    k = H.shape[1] - H.shape[0]
    rng = np.random.default_rng(5)
    info = np.vstack([np.eye(k, dtype=np.uint8), np.ones((1, k), np.uint8),
                      rng.integers(0, 2, size=(8, k), dtype=np.uint8), rng.integers(0, 4, size=(1, k), dtype=np.uint8)])
    ref = Encoder(H).encode(info & 1)
    for a in (info, ref):
        a.setflags(write=False)
    return H, info, ref


@functools.lru_cache(None)
def _ira_case(name):
    code, _ = get_code(name)
    k = code.k
    rng = np.random.default_rng(6)
    info = np.zeros((8, k), np.uint8)
    for row, pos in enumerate((0, 359, 360, k - 1)):
        info[row, pos] = 1
    info[4] = 1
    info[5:] = rng.integers(0, 2, size=(3, k), dtype=np.uint8)
    ref = IRAEncoder(code).encode(info)
    for a in (info, ref):
        a.setflags(write=False)
    return code, info, ref


# 1: an empty lane half (Z = 27); 2, 3: even and odd; 9: past one workgroup; None: the whole array, tail workgroup
@pytest.mark.parametrize("B", (1, 2, 3, 9, None))
@pytest.mark.parametrize("name", sorted(QC))
def test_qc_encode_bitwise(name, B):
    H, info, ref = _qc_case(name)
    dec = ldpc_amd.get_decoder(H, 0)
    assert dec.encoder_path == f"qc-z{QC[name]}-dualdiag"
    got = dec.encode(torch.from_numpy(info[:B].copy()).cuda()).cpu().numpy()
    assert np.array_equal(got, ref[:B])
    if B is None:
        assert not ((got.astype(np.int64) @ np.asarray(H).T.astype(np.int64)) % 2).any()
        assert np.array_equal(ldpc_amd.encode(H, info), ref)  # numpy in -> numpy out


@pytest.mark.parametrize("B", (1, 3, 8))
@pytest.mark.parametrize("name", IRA)
def test_ira_encode_bitwise(name, B):
    code, info, ref = _ira_case(name)
    dec = ldpc_amd.get_decoder(code, 0)
    assert dec.encoder_path == "ira-staircase"
    got = dec.encode(torch.from_numpy(info[:B].copy()).cuda()).cpu().numpy()
    assert np.array_equal(got, ref[:B])


def test_side_stream_into_preallocated_out():
    H, info, ref = _qc_case("wifi1296_23")
    B, n = 9, H.shape[1]
    dec = ldpc_amd.get_decoder(H, 0)
    buf = torch.full((B + 1, n), 0xA5, dtype=torch.uint8, device="cuda")
    x = torch.from_numpy(info[:B].copy()).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out = dec.encode(x, out=buf[:B], stream=side)
    side.synchronize()
    assert out.data_ptr() == buf.data_ptr()
    assert np.array_equal(buf[:B].cpu().numpy(), ref[:B])
    assert bool((buf[B] == 0xA5).all())


def test_graph_without_encoder():
    H, _ = get_code("peg64_32")
    dec = ldpc_amd.get_decoder(H, 0)
    assert dec.encoder_path == "none"
    with pytest.raises(_abi.LdpcError) as e:
        dec.encode(torch.zeros((2, 32), dtype=torch.uint8, device="cuda"))
    assert e.value.code == _abi.LDPC_EUNSUPPORTED


def test_sweep_counters_do_not_depend_on_the_encoder():
    kw = dict(iters=5, snr_db=(1.0, 3.0), codewords=2048, batch=1024)
    a = sweep.run("wifi648_12", encoder="auto", **kw)
    b = sweep.run("wifi648_12", encoder="torch", **kw)
    for key in ("uncoded_ber", "coded_ber", "coded_bler", "codewords"):
        assert np.array_equal(a[key], b[key]), key
