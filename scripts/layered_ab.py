#!/usr/bin/env python3
"""A/B of the layered against the flooding schedule on bench.py's config [1] workload — (648,1/2) min-sum,
B = 65,536, LLRs generated on device at Eb/N0 0:0.5:5 dB, clamp 20 — or, with --algo qms, on config [3]'s:
(1296,2/3), 5-bit LLRs (qmax 15, app_max 127, --qstep), early stop (--early-stop), flooding-20 against layered-10;
--fixed-pair adds the same pair without early stop under "fixed_count"; or, with --code dvbs2_12, on config [4]'s:
DVB-S2 rate 1/2, B = 4,096, Eb/N0 0:0.5:2 dB, the two-stream flooding IRA kernels at 50 iterations against the
LDS-resident layered IRA kernel at 25 sweeps (its record also carries the slot count and the time per layer of one
workgroup); or, with --algo tanh --code wifi1944_56 --mod 16qam-ofdm, on config [2]'s: (1944,5/6) tanh sum-product,
B = 32,768, 16-QAM OFDM LLRs at Eb/N0 4:0.5:9 dB, the flooding k_qc_sp_rs at 50 iterations against the LDS-resident
layered k_qc_sp_lay at 25 sweeps; or, with --code qc:MBxNBxZ[:SEED], on a seeded random quasi-cyclic code (column
weight 3 information part, staircase parity part) that has no compiled table: flooding on the generic CSR kernels
against the table-driven layered k_qc_ms_lay_tab.  In one process on one GPU:

  * block error rate of both legs at every Eb/N0 point (ldpc_count_errors), flooding at --flood-iters (50)
    and layered at --lay-iters (25);
  * event-timed launches in interleaved pairs (flooding, layered, flooding, ...), each leg cycling over the
    points as bench.py's timed loop does, under the engine-clock sampler (ldpc_amd/gpuclock.py): per pair the
    two times and their ratio, so the pair-to-pair spread stands next to the difference it qualifies.

    python scripts/layered_ab.py --out profiles/layered_ab.json [--pairs 12] [--launches 11]
    python scripts/layered_ab.py --algo qms --code wifi1296_23 --flood-iters 20 --lay-iters 10 --early-stop \
        --fixed-pair --out profiles/layered/ab_q5.json
    python scripts/layered_ab.py --code dvbs2_12 --batch 4096 --ebn0 0:0.5:2 --pairs 10 --launches 5 --warmup 10 \
        --out profiles/layered/ab_ira.json
    python scripts/layered_ab.py --algo tanh --code wifi1944_56 --mod 16qam-ofdm --batch 32768 --ebn0 4:0.5:9 \
        --out profiles/layered/ab_sp.json
    python scripts/layered_ab.py --code qc:12x24x81 --batch 16384 --ebn0 1:0.5:3.5 --pairs 8 --launches 6 --warmup 12 \
        --out profiles/layered/ab_tab.json

Needs a GPU; writes one JSON record.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ldpc-sims_amd"))


def qc_random_base(mb, nb, Z, seed, dv=3):
    """Base matrix of a random QC code: dv shifts per information column, a staircase (dual-diagonal) parity part."""
    rng = np.random.default_rng(seed)
    base = -np.ones((mb, nb), np.int32)
    kb = nb - mb
    for j in range(kb):
        rows = rng.choice(mb, size=min(dv, mb), replace=False)
        base[rows, j] = rng.integers(0, Z, size=len(rows))
    for r in range(mb):
        base[r, kb + r] = 0
        if r + 1 < mb:
            base[r + 1, kb + r] = 0
    return base


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--code", default="wifi648_12")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--ebn0", default="0:0.5:5")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--clamp", type=float, default=20.0)
    ap.add_argument("--algo", default="minsum", choices=["minsum", "qms", "tanh"])
    ap.add_argument("--mod", default="bpsk", choices=["bpsk", "16qam-ofdm"], help="LLR generator, as bench.py's --mod")
    ap.add_argument("--qstep", type=float, default=1.0, help="qms: LLR quantizer step (qmax 15, app_max 127)")
    ap.add_argument("--early-stop", action="store_true")
    ap.add_argument("--fixed-pair", action="store_true", help="with --early-stop: time the fixed-count pair too")
    ap.add_argument("--flood-iters", type=int, default=50)
    ap.add_argument("--lay-iters", type=int, default=25)
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--launches", type=int, default=11, help="launches per leg of a pair (one cycle over the points)")
    ap.add_argument("--warmup", type=int, default=22)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layered_ab.json"))
    a = ap.parse_args()

    import torch
    import ldpc_amd
    from ldpc_amd import _abi
    from ldpc_amd.gpuclock import ClockSampler
    from ldpc_amd.synth import DeviceEncoder
    if not torch.cuda.is_available():
        raise SystemExit("layered_ab.py measures on a GPU; none is visible")
    lib = _abi.load()
    base = None
    if a.code.startswith("qc:"):
        dims, *rest = a.code[3:].split(":")
        mb, nb, Z = (int(v) for v in dims.split("x"))
        base = qc_random_base(mb, nb, Z, int(rest[0]) if rest else 5)
        qc = ldpc_amd.codes.QCCode(base, Z, name=a.code)
        H = qc.H()
        dec = ldpc_amd.get_decoder(qc, 0)
    else:
        H, _ = ldpc_amd.get_code(a.code)
        dec = ldpc_amd.get_decoder(H, 0)
    m, n = H.shape
    k, B = n - m, a.batch
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    lo, step, hi = (float(x) for x in a.ebn0.split(":"))
    ebn0 = np.round(np.arange(lo, hi + 1e-9, step), 6)
    info = torch.empty((B, k), dtype=torch.uint8, device="cuda")
    _abi.check(lib.ldpc_random_bits(info.data_ptr(), B, k, a.seed, 0, st))
    cw = DeviceEncoder(H, torch.device("cuda", 0)).encode(info)
    llrs = []
    for i, e in enumerate(ebn0):  # bench.py's generation: same seeds, same points
        x = torch.empty((B, n), dtype=torch.float32, device="cuda")
        if a.mod == "bpsk":
            sigma = float(np.sqrt(1.0 / (2.0 * (k / n) * 10.0 ** (e / 10.0))))
            _abi.check(lib.ldpc_awgn_llr(cw.data_ptr(), x.data_ptr(), B, n, sigma, a.seed * 1000 + i, 0, st))
        else:  # the OFDM front end, 32 subcarriers, 4 bits per symbol
            from ldpc_amd.channel import ofdm_demod, ofdm_tx
            esn0 = float(10.0 ** (e / 10.0) * (k / n) * 4)
            s_ = cw.view(-1)
            if (-s_.numel()) % 128:
                s_ = torch.cat([s_, torch.zeros((-s_.numel()) % 128, dtype=torch.uint8, device="cuda")])
            x.copy_(ofdm_demod(ofdm_tx(s_, 32, 4, esn0, a.seed * 1000 + i, 0), 32, 4, esn0)[:B * n].view(B, n))
        llrs.append(x)
    bits = torch.empty((B, n), dtype=torch.uint8, device="cuda")

    def measure(a, early_stop):
        legs = {}
        for name, iters, sched in (("flooding", a.flood_iters, "flooding"), ("layered", a.lay_iters, "layered")):
            p = dec.params(iters, a.algo, a.clamp, early_stop=early_stop, qstep=a.qstep, device_ptrs=True, schedule=sched)
            wsb = dec.workspace_bytes(B, p)
            legs[name] = dict(p=p, wsb=wsb, ws=torch.empty((max(wsb, 1),), dtype=torch.uint8, device="cuda"),
                              iters=iters, kernel_path=dec.kernel_path(p))

        def launch(leg, x):
            _abi.check(lib.ldpc_decode_ex(dec._h, x.data_ptr(), B, leg["p"], bits.data_ptr(), None, None,
                                          leg["ws"].data_ptr(), leg["wsb"], st))

        bler = {}
        for name, leg in legs.items():
            counts = torch.zeros((len(ebn0), 3), dtype=torch.int64, device="cuda")
            for i, x in enumerate(llrs):
                launch(leg, x)
                _abi.check(lib.ldpc_count_errors(bits.data_ptr(), cw.data_ptr(), B, n, k, counts[i].data_ptr(), st))
            c = counts.cpu().numpy().astype(np.float64)
            bler[name] = dict(coded_bler=(c[:, 1] / c[:, 2]).tolist(), coded_ber_info=(c[:, 0] / (c[:, 2] * k)).tolist())

        def timed(leg):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for s in range(a.launches):
                launch(leg, llrs[s % len(llrs)])
            e1.record(stream)
            return e0, e1

        for w in range(a.warmup):
            launch(legs["flooding" if w % 2 == 0 else "layered"], llrs[w % len(llrs)])
        sampler = ClockSampler(0)
        with sampler:
            events = [(timed(legs["flooding"]), timed(legs["layered"])) for _ in range(a.pairs)]  # no gap between legs
            torch.cuda.synchronize()
        pairs = []
        for (f0, f1), (l0, l1) in events:
            f, l = f0.elapsed_time(f1) / a.launches, l0.elapsed_time(l1) / a.launches
            pairs.append(dict(flooding_ms=f, layered_ms=l, layered_over_flooding_cw_per_s=f / l))
        ratios = [q["layered_over_flooding_cw_per_s"] for q in pairs]
        out = dict(code=a.code, algo=a.algo, mod=a.mod, early_stop=early_stop, qstep=a.qstep, batch=B, ebn0_db=ebn0.tolist(), seed=a.seed, clamp=a.clamp, launches_per_leg=a.launches,
                   library=_abi.library_digest(), device=torch.cuda.get_device_name(0),
                   legs={nm: dict(iters=lg["iters"], kernel_path=lg["kernel_path"], **bler[nm]) for nm, lg in legs.items()},
                   pairs=pairs, clock=sampler.summary())
        for nm, key in (("flooding", "flooding_ms"), ("layered", "layered_ms")):
            ms = [q[key] for q in pairs]
            out["legs"][nm].update(launch_ms_median=statistics.median(ms), launch_ms_min=min(ms), launch_ms_max=max(ms),
                                   ms_per_sweep=statistics.median(ms) / legs[nm]["iters"],
                                   cw_per_s=B / (statistics.median(ms) * 1e-3))
        lay = legs["layered"]
        if lay["kernel_path"] == "ira-z360-layered":  # one workgroup per slot decodes ceil(B / slots) codewords in turn
            a256 = lambda v: (v + 255) // 256 * 256
            slots = lay["wsb"] // (a256(12 * m) + a256(4 * m))
            trips = -(-B // slots)
            out["legs"]["layered"].update(slots=slots, codewords_per_slot=trips, us_per_layer=out["legs"]["layered"][
                "launch_ms_median"] * 1e3 / (trips * lay["iters"] * (m // 360)))
        if base is not None:
            out["base_matrix"] = dict(Z=Z, shifts=base.tolist())
        out["ratio_median"] = statistics.median(ratios)
        out["ratio_min"], out["ratio_max"] = min(ratios), max(ratios)
        return out, legs

    out, legs = measure(a, a.early_stop)
    if a.early_stop and a.fixed_pair:
        out["fixed_count"] = measure(a, False)[0]
        print("fixed count:", json.dumps({kk: out["fixed_count"][kk] for kk in ("ratio_median", "ratio_min", "ratio_max")}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({kk: out[kk] for kk in ("ratio_median", "ratio_min", "ratio_max")}))
    for nm in legs:
        lg = out["legs"][nm]
        print(nm, lg["kernel_path"], f"{lg['iters']} it  {lg['launch_ms_median']:.4f} ms/launch  {lg['ms_per_sweep'] * 1e3:.2f} us/sweep  "
              f"{lg['cw_per_s'] / 1e6:.2f} M cw/s")
    print("Eb/N0  BLER flooding  BLER layered")
    for i, e in enumerate(ebn0):
        print(f"{e:5.2f}  {out['legs']['flooding']['coded_bler'][i]:.5f}       {out['legs']['layered']['coded_bler'][i]:.5f}")


if __name__ == "__main__":
    main()
