#!/usr/bin/env python3
"""Mempool transactions of known signers: hsv_committee_verify_transactions_device
against hsv_verify_transactions_device on the same bytes.

Workload: n (default 2^20) device-resident transactions of `--tx-size` bytes
(default 512, the reference benchmark's), signed on the GPU by
Signer.sign_transactions with K keys drawn uniformly per item, for K = 4, 100
and 1000 -- the reference's benchmark has one key per client and a handful of
clients (node/src/client.rs, benchmark/fabfile.py).  Legs, per K, in one
process, alternating call by call after a warm-up, each call timed by device
events:

  a  the committee call, every signer a member
  b  hsv_verify_transactions_device on the same buffer
  c  hsv_committee_verify_device over the transactions' precomputed 128-byte
     records and member indices: the floor, without message hash and lookup
  d  the committee call with an empty committee (every transaction a miss)
  e  the committee call with keys [0, K / 2) as members (about half hits)

Every leg writes flag bytes only.  Before any timing, the flags of a, c, d and
e must equal those of b byte for byte, every transaction must be STRICT_OK,
and the split each committee call reports (hsv_test_committee_tx_counts) must
be the one the key indices give; a mismatch ends the run.  The tool runs on
libhsv_test.so (the product's objects plus the hooks it needs for c and for
the split).  Writes one JSON record (--out).

    python tools/committee_tx_bench.py --out profiles/committee_tx_bench_2p20.json

`--only a` (or another leg) runs that leg alone at the first K and writes no
record: for a kernel trace of its launches in a run of its own.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hotstuff-digital-signature-benchmarking_amd"))


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ms, n):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "calls": len(ms),
            "per_s_median": round(n / med * 1e3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--tx-size", type=int, default=512)
    ap.add_argument("--keys", type=int, nargs="+", default=[4, 100, 1000])
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices="abcde", help="one leg alone at the first K, no record (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "committee_tx_bench.json"))
    args = ap.parse_args()

    import torch
    from hsverify import STRICT_OK, Signer, _lib, _testing, mempool
    from hsverify.committee import Committee

    if _lib.device_count() <= 0:
        raise SystemExit("committee_tx_bench: no HIP device visible")
    n, size = args.n, args.tx_size
    dev = torch.device("cuda:0")
    rnd = np.random.default_rng(4700)
    gen = torch.Generator(device="cpu").manual_seed(4700)
    d_txs = torch.randint(0, 256, (n, size), generator=gen, dtype=torch.uint8).to(dev)
    rec = {
        "what": "tools/committee_tx_bench.py: hsv_committee_verify_transactions_device against "
                "hsv_verify_transactions_device on the same device-resident transactions",
        "n": n, "tx_size": size, "reps": args.reps, "warmup": args.warmup, "outputs": "flag bytes only",
        "timing": "device events around each call, legs alternating call by call in one process, after the warm-up",
        "checked": "flags of legs a, c, d, e equal leg b's byte for byte; every transaction STRICT_OK; the split "
                   "reported by hsv_test_committee_tx_counts equals the one the key indices give",
        "by_keys": {},
    }
    with _testing.test_library() as lib:
        rec["library"], rec["device"] = _lib.version(), torch.cuda.get_device_name(0)
        for K in args.keys:
            seeds = rnd.integers(0, 256, (K, 32), dtype=np.uint8)
            key_idx = torch.randint(0, K, (n,), generator=gen, dtype=torch.int32).to(dev)
            with Signer(seeds) as signer:
                signer.sign_transactions_device(d_txs, key_idx=key_idx)
                pks = signer.public_keys()
            torch.cuda.synchronize()
            full, empty, half = Committee(pks), Committee(np.zeros((0, 32), np.uint8)), Committee(pks[:K // 2])
            records = torch.zeros((n, 128), dtype=torch.uint8, device=dev)
            _lib.check(lib.hsv_test_tx_records(ctypes.c_void_p(d_txs.data_ptr()), None, size, n,
                                               ctypes.c_void_p(records.data_ptr()),
                                               ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                       "hsv_test_tx_records")
            flags = {leg: torch.full((n,), 0xff, dtype=torch.uint8, device=dev) for leg in "abcde"}
            fault = torch.zeros(2, dtype=torch.int32, device=dev)

            def committee_leg(c, leg):
                return lambda: c.verify_transactions_device(d_txs, None, tx_size=size, n=n, flags=flags[leg], fault=fault)

            legs = {
                "a": committee_leg(full, "a"),
                "b": lambda: mempool.verify_transactions_device(d_txs, None, tx_size=size, n=n, flags=flags["b"],
                                                                fault=fault),
                "c": lambda: full.verify_device(key_idx, records[:, 32:96], records[:, 96:128], flags["c"], fault=fault),
                "d": committee_leg(empty, "d"),
                "e": committee_leg(half, "e"),
            }
            if args.only:
                legs = {args.only: legs[args.only]}
            n_half = int((key_idx < K // 2).sum())
            split = {"a": (n, 0), "d": (0, n), "e": (n_half, n - n_half)}
            counts = {}
            for leg, fn in legs.items():          # correctness first
                fn()
                torch.cuda.synchronize()
                if fault.cpu().tolist() != [0, 0]:
                    raise SystemExit(f"committee_tx_bench: K = {K}, leg {leg}: a device self-check failed")
                if leg in split:
                    counts[leg] = _testing.committee_tx_counts()
                    if counts[leg][:2] != split[leg]:
                        raise SystemExit(f"committee_tx_bench: K = {K}, leg {leg}: split {counts[leg]}, expected {split[leg]}")
            for leg in legs:
                if not bool((flags[leg] & STRICT_OK).all()):
                    raise SystemExit(f"committee_tx_bench: K = {K}, leg {leg}: a signed transaction is rejected")
                if "b" in legs and not torch.equal(flags[leg], flags["b"]):
                    raise SystemExit(f"committee_tx_bench: K = {K}: leg {leg} differs from hsv_verify_transactions_device")
            for _ in range(args.warmup):
                for fn in legs.values():
                    fn()
            torch.cuda.synchronize()
            ms = {leg: [] for leg in legs}
            for _ in range(args.reps):
                for leg, fn in legs.items():
                    ms[leg].append(timed(torch, fn))
            out = {leg: summary(v, n) for leg, v in ms.items()}
            for leg, cnt in counts.items():
                out[leg]["hits_misses_fallback"] = list(cnt)
            if not args.only:
                b = out["b"]["ms_median"]
                out["ratios"] = {
                    "a_speedup_over_b": round(b / out["a"]["ms_median"], 3),
                    "a_faster_than_b": out["a"]["ms_median"] < b,
                    "a_time_over_floor_c": round(out["a"]["ms_median"] / out["c"]["ms_median"], 3),
                    "d_time_over_b": round(out["d"]["ms_median"] / b, 3),
                    "e_time_over_b": round(out["e"]["ms_median"] / b, 3),
                }
            rec["by_keys"][str(K)] = out
            print(json.dumps({"K": K, **{leg: out[leg]["ms_median"] for leg in legs}, **out.get("ratios", {})}), flush=True)
            for c in (full, empty, half):
                c.close()
            del records, flags
            if args.only:
                return
    rec["legs"] = {
        "a": "hsv_committee_verify_transactions_device, every signer a member",
        "b": "hsv_verify_transactions_device",
        "c": "hsv_committee_verify_device over precomputed records and member indices (no hash, no lookup)",
        "d": "hsv_committee_verify_transactions_device, empty committee (all misses)",
        "e": "hsv_committee_verify_transactions_device, keys [0, K / 2) members",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
