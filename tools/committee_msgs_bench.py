#!/usr/bin/env python3
"""Whole messages of known signers: hsv_committee_verify_msgs_device against
hsv_verify_msgs_device on the same bytes.

Workload: n (default 2^20) device-resident items, signed on the GPU by
Signer.sign_device (the ragged shape: by one Signer.sign_msgs_device call over
the packed buffer) with K keys drawn uniformly per item, for K = 4, 100 and
1000, in three shapes: msg_len 32, msg_len 416 (the message part of the
reference benchmark's 512-byte transaction) and ragged lengths uniform in
0 .. 1024 packed back to back in random order.  The reference measures this
workload itself (off-chain-benchmarking/production/src/main.rs: EdDSA over
whole messages under one fixed key and under a fixed key set).  Legs, per
shape and K, in one process, alternating call by call after a warm-up, each
call timed by device events:

  a  the committee call, every signer a member
  b  hsv_verify_msgs_device on the same bytes
  c  hsv_committee_verify_device over the member indices (msg_len 32 only: the
     floor, without the lookup and with the 32-byte hash in the comb kernel)
  d  the committee call with an empty committee (every item a miss)
  e  the committee call with keys [0, K / 2) as members (about half hits)

Every leg writes flag bytes only.  Before any timing, the flags of a, d and e
must equal those of b byte for byte, every item must be STRICT_OK (c too), and
the split each committee call reports (hsv_test_committee_msgs_counts) must be
the one the key indices give; a mismatch ends the run.  The tool runs on
libhsv_test.so (the product's objects plus that hook).  Writes one JSON record
(--out).

    python tools/committee_msgs_bench.py --out profiles/committee_msgs_bench_2p20.json

`--only d --shapes len32` (or another leg and shape) runs that leg alone at the
first K and writes no record: for a kernel trace of its launches in a run of
its own.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hotstuff-digital-signature-benchmarking_amd"))

SHAPES = ("len32", "len416", "ragged_0_1024")


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


def signed_items(torch, signer, shape, n, key_idx, rnd, gen, dev):
    """(d_sig, d_msgs, call keywords, key_idx in item order) of n signed items of `shape`."""
    d_sig = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    if shape != "ragged_0_1024":
        length = 32 if shape == "len32" else 416
        d_msgs = torch.randint(0, 256, (n, length), generator=gen, dtype=torch.uint8).to(dev)
        signer.sign_device(d_msgs, d_sig, key_idx=key_idx, msg_len=length)
        return d_sig, d_msgs.view(-1), {"msg_len": length}, key_idx
    # the messages back to back in random order, signed in one sign_msgs_device call
    lens = np.sort(rnd.integers(0, 1025, n))
    perm = torch.from_numpy(rnd.permutation(n)).to(dev)
    d_lens = torch.from_numpy(lens).to(dev)[perm]
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_off[1:] = torch.cumsum(d_lens, 0)
    d_buf = torch.randint(0, 256, (int(d_off[-1]),), generator=gen, dtype=torch.uint8).to(dev)
    key_idx = key_idx[perm].contiguous()
    signer.sign_msgs_device(d_buf, d_sig, offsets=d_off, key_idx=key_idx)
    return d_sig, d_buf, {"offsets": d_off}, key_idx


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--keys", type=int, nargs="+", default=[4, 100, 1000])
    ap.add_argument("--shapes", nargs="+", choices=SHAPES, default=list(SHAPES))
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices="abcde", help="one leg alone at the first K, no record (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "committee_msgs_bench.json"))
    args = ap.parse_args()

    import torch
    from hsverify import STRICT_OK, Signer, _lib, _testing, verifier
    from hsverify.committee import Committee

    if _lib.device_count() <= 0:
        raise SystemExit("committee_msgs_bench: no HIP device visible")
    n = args.n
    dev = torch.device("cuda:0")
    rnd = np.random.default_rng(4800)
    gen = torch.Generator(device="cpu").manual_seed(4800)
    rec = {
        "what": "tools/committee_msgs_bench.py: hsv_committee_verify_msgs_device against hsv_verify_msgs_device on "
                "the same device-resident items",
        "n": n, "reps": args.reps, "warmup": args.warmup, "outputs": "flag bytes only",
        "timing": "device events around each call, legs alternating call by call in one process, after the warm-up",
        "checked": "flags of legs a, d, e equal leg b's byte for byte; every item STRICT_OK in every leg; the split "
                   "reported by hsv_test_committee_msgs_counts equals the one the key indices give",
        "by_shape": {},
    }
    with _testing.test_library():
        rec["library"], rec["device"] = _lib.version(), torch.cuda.get_device_name(0)
        for shape in args.shapes:
            rec["by_shape"][shape] = {}
            for K in args.keys:
                seeds = rnd.integers(0, 256, (K, 32), dtype=np.uint8)
                drawn = torch.randint(0, K, (n,), generator=gen, dtype=torch.int32).to(dev)
                with Signer(seeds) as signer:
                    d_sig, d_msgs, kw, key_idx = signed_items(torch, signer, shape, n, drawn, rnd, gen, dev)
                    pks = signer.public_keys()
                d_pk = torch.from_numpy(pks).to(dev)[key_idx.to(torch.int64)].contiguous()
                torch.cuda.synchronize()
                full, empty, half = Committee(pks), Committee(np.zeros((0, 32), np.uint8)), Committee(pks[:K // 2])
                flags = {leg: torch.full((n,), 0xff, dtype=torch.uint8, device=dev) for leg in "abcde"}
                fault = torch.zeros(2, dtype=torch.int32, device=dev)

                def committee_leg(c, leg):
                    return lambda: c.verify_msgs_device(d_pk, d_sig, d_msgs, flags=flags[leg], fault=fault, **kw)

                legs = {
                    "a": committee_leg(full, "a"),
                    "b": lambda: verifier.verify_msgs_device(d_pk, d_sig, d_msgs, flags=flags["b"], fault=fault, **kw),
                    "d": committee_leg(empty, "d"),
                    "e": committee_leg(half, "e"),
                }
                if shape == "len32":
                    legs["c"] = lambda: full.verify_device(key_idx, d_sig, d_msgs.view(n, 32), flags["c"], fault=fault)
                if args.only:
                    legs = {args.only: legs[args.only]}
                n_half = int((key_idx < K // 2).sum())
                split = {"a": (n, 0), "d": (0, n), "e": (n_half, n - n_half)}
                counts = {}
                for leg, fn in legs.items():          # correctness first
                    fn()
                    torch.cuda.synchronize()
                    if fault.cpu().tolist() != [0, 0]:
                        raise SystemExit(f"committee_msgs_bench: {shape}, K = {K}, leg {leg}: a device self-check failed")
                    if leg in split:
                        counts[leg] = _testing.committee_msgs_counts()
                        if counts[leg][:2] != split[leg]:
                            raise SystemExit(f"committee_msgs_bench: {shape}, K = {K}, leg {leg}: split {counts[leg]}, "
                                             f"expected {split[leg]}")
                for leg in legs:
                    if not bool((flags[leg] & STRICT_OK).all()):
                        raise SystemExit(f"committee_msgs_bench: {shape}, K = {K}, leg {leg}: a signed item is rejected")
                    if "b" in legs and not torch.equal(flags[leg], flags["b"]):
                        raise SystemExit(f"committee_msgs_bench: {shape}, K = {K}: leg {leg} differs from "
                                         "hsv_verify_msgs_device")
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
                        "d_time_over_b": round(out["d"]["ms_median"] / b, 3),
                        "e_time_over_b": round(out["e"]["ms_median"] / b, 3),
                    }
                    if "c" in out:
                        out["ratios"]["a_time_over_floor_c"] = round(out["a"]["ms_median"] / out["c"]["ms_median"], 3)
                if shape == "ragged_0_1024":
                    out["message_bytes"] = int(d_msgs.numel())
                rec["by_shape"][shape][str(K)] = out
                print(json.dumps({"shape": shape, "K": K, **{leg: out[leg]["ms_median"] for leg in legs},
                                  **out.get("ratios", {})}), flush=True)
                for c in (full, empty, half):
                    c.close()
                del flags, d_sig, d_msgs, d_pk
                if args.only:
                    return
    rec["legs"] = {
        "a": "hsv_committee_verify_msgs_device, every signer a member",
        "b": "hsv_verify_msgs_device",
        "c": "hsv_committee_verify_device over the member indices, msg_len 32 only (no lookup)",
        "d": "hsv_committee_verify_msgs_device, empty committee (all misses)",
        "e": "hsv_committee_verify_msgs_device, keys [0, K / 2) members",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
