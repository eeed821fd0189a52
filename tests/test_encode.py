"""ldpc_encode's C surface and sweep.run's encoder switch, without a GPU."""
import ctypes
import inspect

from ldpc_amd import _abi


def test_library_exports_the_encoder():
    lib = ctypes.CDLL(_abi.LIB_PATH)
    assert hasattr(lib, "ldpc_encode") and hasattr(lib, "ldpc_encoder_path")


def test_null_graph_is_einval_with_a_message():
    lib = _abi.load()
    buf = (ctypes.c_uint8 * 4)()
    rc = lib.ldpc_encode(None, ctypes.addressof(buf), 1, ctypes.addressof(buf), None)
    assert rc == _abi.LDPC_EINVAL and b"null graph" in lib.ldpc_last_error()
    assert lib.ldpc_encoder_path(None) is None


def test_sweep_run_takes_encoder():
    from ldpc_amd import sweep
    assert inspect.signature(sweep.run).parameters["encoder"].default == "auto"
