"""Graph.from_qc builds the CSR of a lifted base matrix without the dense H: the same rows and columns as
Graph.from_H(qc_expand(base, Z)), for the shapes of tests/test_gpu_layered_tab.py."""
import numpy as np
import pytest

from ldpc_amd.codes import Graph, qc_expand


@pytest.mark.parametrize("mb,nb,Z", [(4, 8, 7), (6, 12, 96), (4, 24, 81), (3, 6, 300)])
def test_from_qc_matches_dense(mb, nb, Z):
    rng = np.random.default_rng(5)
    base = np.where(rng.random((mb, nb)) < 0.6, rng.integers(0, Z, size=(mb, nb)), -1).astype(np.int32)
    base[:, 0] = Z - 1   # no empty row; the largest shift
    a, b = Graph.from_qc(base, Z), Graph.from_H(qc_expand(base, Z))
    assert (a.m, a.n) == (b.m, b.n)
    for k in ("row_ptr", "col_idx", "var_ptr", "var_edges"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
