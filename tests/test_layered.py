"""The layered schedule's Python surface and its numpy reference (no GPU)."""
import numpy as np
import pytest

from layered_ref import layered_ms_f32
from ldpc_amd import _abi
from ldpc_amd.api import Decoder
from ldpc_amd.codes import Encoder, get_code


def test_params_schedule_flag():
    assert _abi.F_LAYERED == 32
    assert Decoder.params(5, "minsum", schedule="layered").flags & 32
    assert not Decoder.params(5, "minsum").flags & 32
    with pytest.raises(ValueError):
        Decoder.params(5, "minsum", schedule="x")


def test_reference_decodes_light_noise():
    """Guards the reference itself: at 6 dB it returns what was sent, and stops within a few sweeps."""
    H, _ = get_code("wifi648_12")
    enc = Encoder(H)
    rng = np.random.default_rng(1)
    cw = enc.encode(rng.integers(0, 2, size=(4, enc.k)))
    sigma = np.sqrt(1.0 / (2 * 0.5 * 10 ** 0.6))
    llr = (-2.0 * ((1.0 - 2.0 * cw) + sigma * rng.standard_normal(cw.shape)) / sigma**2).astype(np.float32)
    r = layered_ms_f32(H, llr, 10, 20.0, early_stop=True)
    assert np.array_equal(r["bits"], cw)
    assert (r["iters_used"] <= 3).all()
    assert np.array_equal(layered_ms_f32(H, llr, 0, 20.0)["z"], np.float32(0.5) * (-llr + np.float32(0.0)))
