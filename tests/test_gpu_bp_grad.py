"""Training on the GPU: ``Decoder.bp_forward`` / ``bp_backward`` and ``WeightedBP`` against the plain-torch float64
specification (tests/bp_grad_ref.py).  Errors are max|delta| / max|ref| per gradient tensor.

fp64: both sides evaluate the same formula in float64.  Measured maximum over every case below on the first GPU
run: 1.2e-13 (F64_MEASURED); the bound is 100 x that, rounded up to a power of ten.
fp32: the yardstick is the reference evaluated in torch float32 against its own float64 on the same inputs; the
GPU's fp32 error per tensor may be up to 4 x it (measured: at most 3.3 x, and 1.6e-4 absolute-relative)."""
import functools

import numpy as np
import pytest

from bp_grad_ref import Ref
from softparity import _log

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import ldpc_amd  # noqa: E402
from ldpc_amd import _abi  # noqa: E402
from ldpc_amd.api import get_decoder  # noqa: E402
from ldpc_amd.codes import Graph, get_code  # noqa: E402

NAMES = ("vn", "llr_w", "fin", "fin_llr", "llr")
F64_MEASURED = 1.2e-13   # first GPU run, maximum over all 290 (case, tensor) pairs (the llr gradient, gates case)
F64_BOUND = 1e-10        # 100 x measured, rounded up to a power of ten
CHUNK = 512           # k_bp_wgrad's batch chunk (bp_grad.hip kBpChunk)


@functools.lru_cache(None)
def _code(name):
    H, _ = get_code(name)
    g = Graph.from_H(H)
    return H, g, Ref(g)


def _inputs(g, B, iters, seed, mean=1.5, std=2.5):
    rng = np.random.default_rng(seed)
    w = dict(vn=rng.uniform(0.3, 1.7, (iters, int(g.weight_offsets()[-1]))), llr=rng.uniform(0.3, 1.7, (iters, g.n)),
             fin=rng.uniform(0.3, 1.7, g.E), fin_llr=rng.uniform(0.3, 1.7, g.n))
    return w, rng.standard_normal((B, g.n)) * std + mean, rng.standard_normal((B, g.n))


def _gpu(H, llr, w, G, iters, soft, precision, clamp=10.0):
    d = get_decoder(H)
    dt = torch.float64 if precision == "f64" else torch.float32
    sft, tape = d.bp_forward(torch.from_numpy(llr).to("cuda", dt), iters, w, clamp, soft, precision)
    g = d.bp_backward(tape, torch.from_numpy(G).to("cuda", dt))
    return sft, tape, {k: v.double().cpu().numpy() for k, v in g.items()}


def _err(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _check(label, H, ref, llr, w, G, iters, soft, clamp=10.0):
    """Both precisions of one case against the reference; returns the reference record."""
    r64 = ref.grads(llr, w, G, iters, clamp, soft)
    r32 = ref.grads(llr, w, G, iters, clamp, soft, torch.float32)
    g64 = _gpu(H, llr, w, G, iters, soft, "f64", clamp)[2]
    g32 = _gpu(H, llr, w, G, iters, soft, "f32", clamp)[2]
    for k in NAMES:
        if not np.abs(r64[k]).max():   # vn at one iteration: x^0 = 0 is no variable
            assert not g64[k].any() and not g32[k].any(), k
            continue
        e64, e32, yard = _err(g64[k], r64[k]), _err(g32[k], r64[k]), _err(r32[k], r64[k])
        _log({"label": f"bp_grad {label} {k}", "kind": "grad_rel", "f64": e64, "f32": e32, "f32_torch": yard})
        print(f"bp_grad {label} {k}: f64 {e64:.3g} f32 {e32:.3g} torch-f32 {yard:.3g}")
        assert e64 < F64_BOUND, (k, e64)
        assert e32 <= 4 * yard, (k, e32, yard)
    return r64


CASES = [(c, B) for c in ("peg64_32", "wifi648_12", "wifi1944_56") for B in (1, 5, 67)] + [("peg64_32", CHUNK + 3)]


@pytest.mark.parametrize("soft", ["z", "p1"])
@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("code,B", CASES)
def test_gradients_match_reference(code, B, iters, soft):
    H, g, ref = _code(code)
    w, llr, G = _inputs(g, B, iters, seed=B + iters)
    _check(f"{code} B{B} it{iters} {soft}", H, ref, llr, w, G, iters, soft)


def test_gates_strong_llr():
    """Clamp 10 on strong LLRs: a quarter of the last iteration's messages are saturated and pass no gradient; no
    pre-clamp magnitude is within 1e-3 (relative) of the bound, so both precisions agree on every gate."""
    H, g, ref = _code("peg64_32")
    w, llr, G = _inputs(g, 8, 3, seed=0, mean=14.0, std=6.0)
    r = _check("gates", H, ref, llr, w, G, 3, "p1")
    assert 0.05 < (r["y"] > 10.0).mean() < 0.95
    assert np.abs(r["y"] / 10.0 - 1.0).min() > 1e-3


def test_exact_zero_llrs():
    """A few LLRs exactly 0.0 (tanh(0) = 0 at iteration 0, the fp32 kernels' a == 1 codewords): the exclusive
    products give the derivative without dividing by tau."""
    H, g, ref = _code("wifi648_12")
    w, llr, G = _inputs(g, 5, 2, seed=11)
    llr[0, [3, 40, 41]] = 0.0
    llr[3, 600] = 0.0
    _check("zeros", H, ref, llr, w, G, 2, "p1")


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_forward_equals_decode_and_backward_is_reproducible(precision):
    H, g, _ = _code("wifi648_12")
    w, llr, G = _inputs(g, 67, 3, seed=5)
    d = get_decoder(H)
    dt = torch.float64 if precision == "f64" else torch.float32
    x, Gt = torch.from_numpy(llr).to("cuda", dt), torch.from_numpy(G).to("cuda", dt)
    for soft in ("z", "p1"):
        sft, tape = d.bp_forward(x, 3, w, soft=soft, precision=precision)
        assert torch.equal(sft, d.decode(x, 3, weights=w, soft=soft, precision=precision)["soft"])
    a, b = d.bp_backward(tape, Gt), d.bp_backward(tape, Gt)
    assert all(torch.equal(a[k], b[k]) for k in NAMES)
    assert not a["vn"].reshape(3, -1)[0].any()                  # x^0 = 0
    wofs, dv = g.weight_offsets(), g.var_degrees()
    diag = np.concatenate([wofs[v] + np.arange(dv[v]) * (dv[v] + 1) for v in range(g.n)])
    assert not a["vn"][:, torch.from_numpy(diag).cuda()].any()  # u == t is no weight


def test_module_trains_and_round_trips():
    H, g, _ = _code("peg64_32")
    w, llr, G = _inputs(g, 9, 2, seed=2)
    m = ldpc_amd.WeightedBP(H, 2)
    with torch.no_grad():
        for prm, k in ((m.vn, "vn"), (m.llr_weight, "llr"), (m.fin, "fin"), (m.fin_llr, "fin_llr")):
            prm.copy_(torch.from_numpy(w[k]))
    x = torch.from_numpy(llr).float().cuda().requires_grad_()
    Gt = torch.from_numpy(G).float().cuda()
    p1 = m(x)
    (p1 * Gt).sum().backward()
    d = get_decoder(H)
    want = d.bp_backward(d.bp_forward(x, 2, m.weights_dict())[1], Gt)
    for prm, k in ((m.vn, "vn"), (m.llr_weight, "llr_w"), (m.fin, "fin"), (m.fin_llr, "fin_llr"), (x, "llr")):
        assert torch.equal(prm.grad, want[k]), k
    bp = ldpc_amd.BeliefPropagation(H, 2).load_reference_state_dict(m.reference_state_dict())
    assert torch.equal(bp(None, x.detach(), 10.0), p1.detach())
    m2 = ldpc_amd.WeightedBP(H, 2).load_reference_state_dict(m.reference_state_dict())
    assert torch.equal(m2.vn * (m2.vn != 0), m.vn * (m2.vn != 0)) and torch.equal(m2.fin, m.fin)


@pytest.mark.parametrize("kw,reason", [(dict(early_stop=True), "early stop"), (dict(x0=1), "x0"),
                                       (dict(algo="minsum"), "tanh")])
def test_refusals(kw, reason):
    H, g, _ = _code("peg64_32")
    with pytest.raises(_abi.LdpcError, match=reason) as e:
        get_decoder(H).bp_forward(torch.zeros((4, g.n), device="cuda"), 2, **kw)
    assert e.value.code == _abi.LDPC_EUNSUPPORTED
