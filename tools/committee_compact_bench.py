#!/usr/bin/env python3
"""Compact committees (48 KiB of comb table per key, hsv_committee_create_ex
with 4-bit digits) against the generic calls and against a full committee
(384 KiB per key) on the same bytes.

Workload: n (default 2^20) device-resident items signed on the GPU by a Signer
with K keys, a uniformly random member per item, in two shapes: whole messages
of 32 bytes (hsv_committee_verify_msgs_device against hsv_verify_msgs_device)
and transactions of 512 bytes (hsv_committee_verify_transactions_device against
hsv_verify_transactions_device).  K = 1000, 2^14 and 2^17; at 2^17 the compact
tables take 6 GiB, far beyond the 256 MiB Infinity Cache.  Legs, per shape and
K, in one process, alternating call by call after a warm-up, each call timed by
device events:

  g  the generic call
  f  a full committee, every signer a member (K <= --full-max-keys only: 2^14
     full tables would already be 6 GiB)
  c  a compact committee, every signer a member
  h  a compact committee of keys [0, K / 2) (about half hits)

Every leg writes flag bytes only.  Before any timing, the flags of f, c and h
must equal those of g byte for byte, every item must be STRICT_OK, and the
split each committee call reports (hsv_test_committee_*_counts) must be the one
the key indices give; a mismatch ends the run.  The build of each compact
committee is timed on the host clock around hsv_committee_create_ex (it ends in
a stream synchronise; allocation, key copy and lookup table included).  The
tool runs on libhsv_test.so (the product's objects plus the count hooks).
Writes one JSON record (--out).

    python tools/committee_compact_bench.py --out profiles/committee_compact_bench_2p20.json

`--only c --shapes tx512 --keys 131072` (or another leg, shape and K) runs that
leg alone and writes no record: for a kernel trace of its launches in a run of
its own.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hotstuff-digital-signature-benchmarking_amd"))

SHAPES = ("msgs32", "tx512")
TX_SIZE = 512


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
    ap.add_argument("--keys", type=int, nargs="+", default=[1000, 1 << 14, 1 << 17])
    ap.add_argument("--full-max-keys", type=int, default=1000, help="largest K that also gets a full committee")
    ap.add_argument("--shapes", nargs="+", choices=SHAPES, default=list(SHAPES))
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices="gfch", help="one leg alone at the first shape and K, no record")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "committee_compact_bench.json"))
    args = ap.parse_args()

    import torch
    from hsverify import STRICT_OK, Signer, _lib, _testing, mempool, verifier
    from hsverify.committee import Committee

    if _lib.device_count() <= 0:
        raise SystemExit("committee_compact_bench: no HIP device visible")
    n = args.n
    dev = torch.device("cuda:0")
    rnd = np.random.default_rng(4900)
    gen = torch.Generator(device="cpu").manual_seed(4900)
    rec = {
        "what": "tools/committee_compact_bench.py: compact committees (48 KiB per key) against the generic calls and "
                "a full committee (384 KiB per key) on the same device-resident items",
        "n": n, "reps": args.reps, "warmup": args.warmup, "outputs": "flag bytes only",
        "timing": "device events around each call, legs alternating call by call in one process, after the warm-up; "
                  "builds on the host clock around hsv_committee_create_ex",
        "checked": "flags of legs f, c, h equal leg g's byte for byte; every item STRICT_OK in every leg; the split "
                   "reported by the count hooks equals the one the key indices give",
        "by_shape": {},
    }

    def built(pks, compact):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c = Committee(pks, compact=compact)
        return c, time.perf_counter() - t0

    with _testing.test_library():
        rec["library"], rec["device"] = _lib.version(), torch.cuda.get_device_name(0)
        for shape in args.shapes:
            rec["by_shape"][shape] = {}
            for K in args.keys:
                seeds = rnd.integers(0, 256, (K, 32), dtype=np.uint8)
                key_idx = torch.randint(0, K, (n,), generator=gen, dtype=torch.int32).to(dev)
                with Signer(seeds) as signer:
                    pks = signer.public_keys()
                    if shape == "msgs32":
                        d_msgs = torch.randint(0, 256, (n, 32), generator=gen, dtype=torch.uint8).to(dev)
                        d_sig = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
                        signer.sign_device(d_msgs, d_sig, key_idx=key_idx, msg_len=32)
                        d_pk = torch.from_numpy(pks).to(dev)[key_idx.to(torch.int64)].contiguous()
                    else:
                        d_txs = torch.randint(0, 256, (n, TX_SIZE), generator=gen, dtype=torch.uint8).to(dev)
                        signer.sign_transactions_device(d_txs, key_idx=key_idx)
                torch.cuda.synchronize()
                flags = {leg: torch.full((n,), 0xff, dtype=torch.uint8, device=dev) for leg in "gfch"}
                fault = torch.zeros(2, dtype=torch.int32, device=dev)
                if shape == "msgs32":
                    generic = lambda: verifier.verify_msgs_device(d_pk, d_sig, d_msgs.view(-1), flags=flags["g"],
                                                                  fault=fault, msg_len=32)
                    call = lambda c, leg: (lambda: c.verify_msgs_device(d_pk, d_sig, d_msgs.view(-1), flags=flags[leg],
                                                                        fault=fault, msg_len=32))
                    read_counts = _testing.committee_msgs_counts
                else:
                    generic = lambda: mempool.verify_transactions_device(d_txs, None, tx_size=TX_SIZE, n=n,
                                                                         flags=flags["g"], fault=fault)
                    call = lambda c, leg: (lambda: c.verify_transactions_device(d_txs, None, tx_size=TX_SIZE, n=n,
                                                                                flags=flags[leg], fault=fault))
                    read_counts = _testing.committee_tx_counts
                committees, builds = {}, {}
                want = [leg for leg in "fch" if (leg != "f" or K <= args.full_max_keys)
                        and (not args.only or leg == args.only)]
                for leg in want:
                    committees[leg], builds[leg] = built(pks[:K // 2] if leg == "h" else pks, compact=leg != "f")
                legs = {leg: call(c, leg) for leg, c in committees.items()}
                if not args.only or args.only == "g":
                    legs = {"g": generic, **legs}
                n_half = int((key_idx < K // 2).sum())
                split = {"f": (n, 0), "c": (n, 0), "h": (n_half, n - n_half)}
                counts = {}
                for leg, fn in legs.items():          # correctness first
                    fn()
                    torch.cuda.synchronize()
                    if fault.cpu().tolist() != [0, 0]:
                        raise SystemExit(f"committee_compact_bench: {shape}, K = {K}, leg {leg}: a device self-check failed")
                    if leg in split:
                        counts[leg] = read_counts()
                        if counts[leg][:2] != split[leg]:
                            raise SystemExit(f"committee_compact_bench: {shape}, K = {K}, leg {leg}: split "
                                             f"{counts[leg]}, expected {split[leg]}")
                for leg in legs:
                    if not bool((flags[leg] & STRICT_OK).all()):
                        raise SystemExit(f"committee_compact_bench: {shape}, K = {K}, leg {leg}: a signed item is rejected")
                    if "g" in legs and not torch.equal(flags[leg], flags["g"]):
                        raise SystemExit(f"committee_compact_bench: {shape}, K = {K}: leg {leg} differs from the "
                                         "generic call")
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
                for leg, c in committees.items():
                    out[leg].update({"keys": len(c), "digit_bits": c.digit_bits, "table_bytes": c.table_bytes,
                                     "build_s": round(builds[leg], 4),
                                     "build_us_per_key": round(builds[leg] / max(1, len(c)) * 1e6, 3)})
                if not args.only:
                    g = out["g"]["ms_median"]
                    out["ratios"] = {"c_rate_over_g": round(g / out["c"]["ms_median"], 3),
                                     "h_time_over_g": round(out["h"]["ms_median"] / g, 3)}
                    if "f" in out:
                        out["ratios"]["f_rate_over_g"] = round(g / out["f"]["ms_median"], 3)
                        out["ratios"]["c_rate_over_f"] = round(out["f"]["ms_median"] / out["c"]["ms_median"], 3)
                rec["by_shape"][shape][str(K)] = out
                print(json.dumps({"shape": shape, "K": K, **{leg: out[leg]["ms_median"] for leg in legs},
                                  **{f"build_us_per_key_{leg}": out[leg]["build_us_per_key"] for leg in committees},
                                  **out.get("ratios", {})}), flush=True)
                for c in committees.values():
                    c.close()
                del flags, legs, generic, call
                if shape == "msgs32":
                    del d_msgs, d_sig, d_pk
                else:
                    del d_txs
                if args.only:
                    return
            ks = rec["by_shape"][shape]
            lo, hi = str(min(args.keys)), str(max(args.keys))
            if lo != hi:                              # whether the gathered table reads become the limit
                ks["c_rate_at_%s_over_%s_keys" % (hi, lo)] = round(ks[lo]["c"]["ms_median"] / ks[hi]["c"]["ms_median"], 3)
    rec["legs"] = {
        "g": "the generic call: hsv_verify_msgs_device (msgs32), hsv_verify_transactions_device (tx512)",
        "f": "the committee call, full tables (8-bit digits, 384 KiB per key), every signer a member",
        "c": "the committee call, compact tables (4-bit digits, 48 KiB per key), every signer a member",
        "h": "the committee call, compact tables, keys [0, K / 2) members",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
