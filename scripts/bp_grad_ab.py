#!/usr/bin/env python3
"""One training step of weighted BP, the HIP path against what a user could do without it.

    python scripts/bp_grad_ab.py [--out profiles/bp_grad/ab.json] [--pairs 7] [--hip-only N]

Workload: 802.11n (648,1/2), 5 iterations, B = 4096, fp32, LLRs made on the device at Eb/N0 = 2 dB (all-zero
codeword, BPSK/AWGN).  A step is the tape forward plus the backward for all five gradients.  The comparator is the
sparse torch-op statement of the same function (tests/bp_grad_ref.py) on the same GPU in float32 with
torch.autograd.  Both are timed with device events over whole steps, in interleaved pairs in one process; the
engine clock is sampled over the timed loop.  ``--hip-only N`` runs N HIP steps and nothing else (the program a
kernel trace wraps)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ldpc-sims_amd"), os.path.join(ROOT, "tests")]
from bp_grad_ref import Ref  # noqa: E402
from ldpc_amd import get_code, get_decoder  # noqa: E402
from ldpc_amd.codes import Graph  # noqa: E402
from ldpc_amd.gpuclock import ClockSampler  # noqa: E402

CODE, ITERS, B, EBN0 = "wifi648_12", 5, 4096, 2.0


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bp_grad", "ab.json"))
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--hip-only", type=int, default=0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    H, _ = get_code(CODE)
    g = Graph.from_H(H)
    d = get_decoder(H)
    gen = torch.Generator(device="cuda").manual_seed(1)
    sigma = float(np.sqrt(1.0 / (2 * 0.5 * 10 ** (EBN0 / 10))))
    llr = -2.0 * (1.0 + sigma * torch.randn((B, g.n), device="cuda", generator=gen)) / sigma**2
    G = torch.randn((B, g.n), device="cuda", generator=gen)
    shapes = dict(vn=(ITERS, int(g.weight_offsets()[-1])), llr=(ITERS, g.n), fin=(g.E,), fin_llr=(g.n,))
    w = {k: 0.3 + 1.4 * torch.rand(s, device="cuda", generator=gen) for k, s in shapes.items()}
    tape_bytes = []

    def hip_step():
        _, tape = d.bp_forward(llr, ITERS, w)
        tape_bytes[:] = [tape.nbytes]
        return d.bp_backward(tape, G)

    if a.hip_only:
        for _ in range(a.hip_only):
            hip_step()
        torch.cuda.synchronize()
        return
    ref = Ref(g)
    for k in ("tgt", "src", "pos", "vs", "ve", "inv", "idx", "valid"):
        setattr(ref, k, getattr(ref, k).cuda())

    def torch_step():
        t = {k: v.clone().requires_grad_() for k, v in dict(w, x=llr).items()}
        (ref.forward(t["x"], t, ITERS)[0] * G).sum().backward()
        return {"vn": t["vn"].grad, "llr_w": t["llr"].grad, "fin": t["fin"].grad, "fin_llr": t["fin_llr"].grad,
                "llr": t["x"].grad}

    gh, gt = hip_step(), torch_step()   # warm-up of both, and the two agree (fp32 against fp32)
    agree = {k: float((gh[k] - gt[k]).abs().max() / gt[k].abs().max()) for k in gh}
    timed(hip_step, 20), timed(torch_step, 3)
    pairs = []
    with ClockSampler(0) as cs:
        for _ in range(a.pairs):
            pairs.append({"hip_ms": timed(hip_step, 50), "torch_ms": timed(torch_step, 5)})
    ratio = [p["torch_ms"] / p["hip_ms"] for p in pairs]
    rec = dict(workload=dict(code=CODE, iters=ITERS, B=B, precision="f32", ebn0_db=EBN0,
                             step="tape forward + backward, all five gradients"),
               comparator="tests/bp_grad_ref.py on the same GPU, float32, torch.autograd", pairs=pairs,
               hip_ms=dict(median=statistics.median(p["hip_ms"] for p in pairs), min=min(p["hip_ms"] for p in pairs),
                           max=max(p["hip_ms"] for p in pairs)),
               torch_ms=dict(median=statistics.median(p["torch_ms"] for p in pairs),
                             min=min(p["torch_ms"] for p in pairs), max=max(p["torch_ms"] for p in pairs)),
               torch_over_hip=dict(median=statistics.median(ratio), min=min(ratio), max=max(ratio)),
               hip_ahead_in_every_pair=all(r > 1 for r in ratio), tape_bytes=tape_bytes[0],
               max_rel_difference_hip_vs_torch_f32=agree, clock=cs.summary(), device=torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("hip_ms", "torch_ms", "torch_over_hip", "tape_bytes", "clock")}))


if __name__ == "__main__":
    main()
