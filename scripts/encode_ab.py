#!/usr/bin/env python3
"""A/B of the HIP encoders (ldpc_encode: csrc/encode.hip) against synth.DeviceEncoder (torch arithmetic) in one
process on one GPU, on the same device-resident information bits:

  * the three 802.11n codes at B = 65,536 and dvbs2_12 at B = 4,096 (bench.py --full's config [4] batch): the two
    outputs are compared bit for bit at the timed size, then event-timed in interleaved pairs (torch, hip,
    torch, ...) under the engine-clock sampler (ldpc_amd/gpuclock.py): per pair the two times per call and
    their ratio, so the pair-to-pair spread stands next to the difference it qualifies;
  * the share of its compulsory bytes per second (read B k, write B n) the HIP kernel reaches of the
    device-to-device copy rate this GPU measures in the same process (read + write of a buffer of that size);
  * for wifi648_12, the wall time of one sweep point (layered min-sum, 25 sweeps, 65,536 codewords) with
    encoder="torch" against "auto", again in interleaved pairs: the encoder's share of a sweep.

    python scripts/encode_ab.py --out profiles/encode/ab.json [--pairs 10]

Needs a GPU; writes one JSON record.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ldpc-sims_amd"))

CASES = (("wifi648_12", 65536), ("wifi1296_23", 65536), ("wifi1944_56", 65536), ("dvbs2_12", 4096))


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--hip-reps", type=int, default=1000, help="calls per timed window of the HIP leg")
    ap.add_argument("--torch-reps", type=int, default=20, help="calls per timed window of the torch leg")
    ap.add_argument("--sweep-pairs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode", "ab.json"))
    a = ap.parse_args()

    import torch
    import ldpc_amd
    from ldpc_amd import _abi, sweep
    from ldpc_amd.gpuclock import ClockSampler
    from ldpc_amd.synth import DeviceEncoder
    if not torch.cuda.is_available():
        raise SystemExit("encode_ab.py measures on a GPU; none is visible")
    lib = _abi.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        return e0, e1

    out = dict(device=torch.cuda.get_device_name(0), library=_abi.library_digest(), seed=a.seed, pairs=a.pairs,
               hip_reps=a.hip_reps, torch_reps=a.torch_reps, codes={})
    for name, B in CASES:
        H, _ = ldpc_amd.get_code(name)
        m, n = H.shape
        k = n - m
        dec = ldpc_amd.get_decoder(H, 0)
        info = torch.empty((B, k), dtype=torch.uint8, device=dev)
        _abi.check(lib.ldpc_random_bits(info.data_ptr(), B, k, a.seed, 0, stream.cuda_stream))
        tenc = DeviceEncoder(H, dev)
        cw = torch.empty((B, n), dtype=torch.uint8, device=dev)
        legs = dict(torch=lambda: tenc.encode(info), hip=lambda: dec.encode(info, out=cw))
        same = bool(torch.equal(legs["torch"](), legs["hip"]()))  # also the first warm-up of both
        if not same:
            raise SystemExit(f"{name}: the HIP encoder and DeviceEncoder disagree at B = {B}")
        # the copy rate of this GPU on a buffer of the kernel's footprint: B (k + n) / 2 bytes read and written
        src = torch.empty((B * (k + n) // 2,), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        for _ in range(3):
            window(legs["torch"], a.torch_reps)
            window(legs["hip"], a.hip_reps)
            window(lambda: dst.copy_(src), a.hip_reps)
        torch.cuda.synchronize()
        sampler = ClockSampler(0)
        with sampler:
            ev = [(window(legs["torch"], a.torch_reps), window(legs["hip"], a.hip_reps),
                   window(lambda: dst.copy_(src), a.hip_reps)) for _ in range(a.pairs)]
            torch.cuda.synchronize()
        pairs = []
        for (t0, t1), (h0, h1), (c0, c1) in ev:
            t, h, c = t0.elapsed_time(t1) / a.torch_reps, h0.elapsed_time(h1) / a.hip_reps, c0.elapsed_time(c1) / a.hip_reps
            pairs.append(dict(torch_ms=t, hip_ms=h, copy_ms=c, torch_over_hip=t / h))
        byts = B * (k + n)
        hip_ms, copy_ms = (statistics.median(p[key] for p in pairs) for key in ("hip_ms", "copy_ms"))
        rec = dict(batch=B, k=k, n=n, encoder_path=dec.encoder_path, bitwise_equal=same, pairs=pairs,
                   torch_ms=spread([p["torch_ms"] for p in pairs]), hip_ms=spread([p["hip_ms"] for p in pairs]),
                   torch_over_hip=spread([p["torch_over_hip"] for p in pairs]), compulsory_bytes=byts,
                   hip_gbytes_per_s=byts / (hip_ms * 1e6), copy_gbytes_per_s=byts / (copy_ms * 1e6),
                   share_of_copy_rate=copy_ms / hip_ms, clock=sampler.summary())
        out["codes"][name] = rec
        print(f"{name:12s} B={B:6d} {rec['encoder_path']:16s} torch {rec['torch_ms']['median']:9.4f} ms  hip "
              f"{rec['hip_ms']['median']:8.4f} ms  ratio {rec['torch_over_hip']['median']:8.1f} "
              f"[{rec['torch_over_hip']['min']:.1f}, {rec['torch_over_hip']['max']:.1f}]  "
              f"{rec['hip_gbytes_per_s']:.0f} GB/s = {rec['share_of_copy_rate']:.2f} of the copy rate", flush=True)
        del tenc, info, cw, src, dst, legs
        torch.cuda.empty_cache()

    kw = dict(code="wifi648_12", algo="minsum", iters=25, schedule="layered", snr_db=(2.0,), codewords=65536, batch=65536)
    for e in ("torch", "auto"):
        sweep.run(encoder=e, **kw)
    sp = []
    for _ in range(a.sweep_pairs):
        t, h = (sweep.run(encoder=e, **kw)["seconds"] * 1e3 for e in ("torch", "auto"))
        sp.append(dict(torch_ms=t, auto_ms=h, torch_over_auto=t / h))
    out["sweep_point"] = dict(config={kk: (list(v) if isinstance(v, tuple) else v) for kk, v in kw.items()}, pairs=sp,
                              torch_ms=spread([p["torch_ms"] for p in sp]), auto_ms=spread([p["auto_ms"] for p in sp]),
                              torch_over_auto=spread([p["torch_over_auto"] for p in sp]))
    s = out["sweep_point"]
    print(f"sweep point wifi648_12 layered-25, 65,536 cw: torch {s['torch_ms']['median']:.3f} ms  auto "
          f"{s['auto_ms']['median']:.3f} ms  ratio {s['torch_over_auto']['median']:.3f} "
          f"[{s['torch_over_auto']['min']:.3f}, {s['torch_over_auto']['max']:.3f}]")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
