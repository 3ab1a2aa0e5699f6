#!/usr/bin/env python3
"""hsv_committee_verify_msgs_indexed_device against the calls a committee
holder had before it.

One process, K = 1000 keys, every item device-resident and signed on the GPU by
Signer.sign_msgs_device, every signature valid.  Before anything is timed the
new call's flags must equal those of hsv_committee_verify_msgs_device and of
hsv_verify_msgs_device on the same bytes, and every item must be STRICT_OK.

Latency: m = 3, 67, 667, 4096 at message lengths 32, 100, 416 and ragged
0 .. 1024.  Legs, alternating call by call, --calls timed calls each, host clock
around the call and a synchronise of its stream:
  a  hsv_committee_verify_msgs_indexed_device   (the product's route, by m)
  b  hsv_committee_verify_msgs_device           (pk-addressed: three launches)
  c  hsv_verify_msgs_device                     (no committee: a small form)
  d  hsv_committee_verify_device                (32-byte digests; at 32 bytes only: the floor)
The quad route ships for a size only where a's p50 is below b's and c's.

Throughput: 2^20 items at 32 and 416 bytes, legs a and b alternating, 3 warm-up
and 12 timed calls each, device events, two passes; a must not exceed b by more
than b's spread between the passes.

--attach NAME=FILE copies other JSON results of the same run (bench.py against
the parent's library, tools/msgs_small_bench.py) into the output.

    python tools/committee_msgs_indexed_bench.py --out profiles/committee_msgs_indexed_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hotstuff-digital-signature-benchmarking_amd"))

SIZES = (3, 67, 667, 4096)
KINDS = ("len32", "len100", "len416", "ragged_0_1024")
NKEYS = 1000


def pct(ms, q):
    return round(float(np.percentile(np.asarray(ms), q)), 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=300, help="timed calls per leg and point")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=9100)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--kinds", nargs="*", default=list(KINDS))
    ap.add_argument("--throughput-items", type=int, default=1 << 20, help="0 skips the throughput part")
    ap.add_argument("--attach", action="append", default=[], metavar="NAME=FILE")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "committee_msgs_indexed_bench.json"))
    args = ap.parse_args()

    import torch
    from hsverify import Signer, _lib, _testing
    from hsverify.committee import Committee
    from hsverify import verifier

    if _lib.device_count() <= 0:
        raise SystemExit("committee_msgs_indexed_bench: no HIP device visible (there is no CPU form of the verifier)")
    dev = torch.device("cuda:0")
    rnd = np.random.default_rng(args.seed)
    seeds = rnd.integers(0, 256, (NKEYS, 32), dtype=np.uint8)

    with _testing.test_library() as lib:
        lib.hsv_set_auto_committee(0)
        lib.hsv_set_resident_service(0)
        _testing.cmsg_indexed_form(-1)
        stream = torch.cuda.current_stream(dev)
        signer = Signer(seeds)
        keys = signer.public_keys()
        committee = Committee(keys)
        d_keys = torch.from_numpy(keys).to(dev)

        def batch(n, kind):
            """n valid items of `kind`: (key_idx, pk, sig, message bytes 3 bytes off a 16-byte boundary,
            offsets or None, msg_len)"""
            idx = torch.from_numpy(rnd.integers(0, NKEYS, n).astype(np.int32)).to(dev)
            if kind == "ragged_0_1024":
                lens = rnd.integers(0, 1025, n)
                off = np.zeros(n + 1, np.int64)
                off[1:] = np.cumsum(lens)
                length, total = 0, int(off[-1])
                d_off = torch.from_numpy(off).to(dev)
            else:
                length = int(kind[3:])
                total, d_off = n * length, None
            raw = torch.zeros(total + 19, dtype=torch.uint8, device=dev)
            raw[3:3 + total].copy_(torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev))
            sig = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
            fault = torch.zeros(2, dtype=torch.int32, device=dev)
            signer.sign_msgs_device(raw[3:], sig, offsets=d_off, msg_len=length, key_idx=idx, fault=fault)
            torch.cuda.synchronize()
            if fault.cpu().tolist() != [0, 0]:
                raise SystemExit(f"committee_msgs_indexed_bench: signing {kind}: self-check words {fault.cpu().tolist()}")
            return idx, d_keys[idx.long()].contiguous(), sig, raw[3:], d_off, length

        def legs(n, b):
            idx, pk, sig, msgs, off, length = b
            o = off[:n + 1] if off is not None else None
            out = {k: torch.zeros(n, dtype=torch.uint8, device=dev) for k in "abc"}
            fn = {"a": lambda fault=None: committee.verify_msgs_indexed_device(idx[:n], sig[:n], msgs, o, msg_len=length,
                                                                               flags=out["a"], fault=fault),
                  "b": lambda fault=None: committee.verify_msgs_device(pk[:n], sig[:n], msgs, o, msg_len=length,
                                                                       flags=out["b"], fault=fault),
                  "c": lambda fault=None: verifier.verify_msgs_device(pk[:n], sig[:n], msgs, o, msg_len=length,
                                                                      flags=out["c"], fault=fault)}
            return fn, out

        def checked(n, fn, out, what):
            for k, f in fn.items():
                fault = torch.ones(2, dtype=torch.int32, device=dev)
                out[k].fill_(0xee)
                f(fault)
                torch.cuda.synchronize()
                if fault.cpu().tolist() != [0, 0]:
                    raise SystemExit(f"committee_msgs_indexed_bench: {what} leg {k}: self-check words {fault.cpu().tolist()}")
            if not (torch.equal(out["a"], out["b"]) and torch.equal(out["a"], out["c"])):
                raise SystemExit(f"committee_msgs_indexed_bench: {what}: the legs' flags differ")
            bad = int((out["a"] & 1).eq(0).sum())
            if bad:
                raise SystemExit(f"committee_msgs_indexed_bench: {what}: {bad} valid signatures rejected")

        def one(f):
            t0 = time.perf_counter()
            f()
            stream.synchronize()
            return (time.perf_counter() - t0) * 1e3

        rec = {"what": "tools/committee_msgs_indexed_bench.py: hsv_committee_verify_msgs_indexed_device (a) against "
                       "hsv_committee_verify_msgs_device (b), hsv_verify_msgs_device (c) and, at 32 bytes, "
                       "hsv_committee_verify_device on digests (d); one process, legs alternating call by call",
               "library": _lib.version(), "device": torch.cuda.get_device_name(0), "keys": NKEYS,
               "calls_per_leg": args.calls, "warmup": args.warmup,
               "timing": "latency: host clock around the call and a synchronise of its stream, ms; throughput: "
                         "device events around each call, ms",
               "checked": "flags of a equal to b's and c's, all STRICT_OK, fault words zero, before timing",
               "latency": [], "throughput": []}
        nmax = max(args.sizes) if args.sizes else 0
        for kind in args.kinds:
            if not nmax:
                break
            b = batch(nmax, kind)
            for n in args.sizes:
                fn, out = legs(n, b)
                before = _testing.cmsg_indexed_counts()
                checked(n, fn, out, f"{kind} m={n}")
                after = _testing.cmsg_indexed_counts()
                route = "quad" if after[0] > before[0] else "bulk"
                if kind == "len32":   # the floor: the same triples as 32-byte digests
                    ref = torch.zeros(n, dtype=torch.uint8, device=dev)
                    d_msg = b[3][:n * 32].clone().reshape(n, 32)
                    fn["d"] = lambda fault=None: committee.verify_device(b[0][:n], b[2][:n], d_msg, ref, fault=fault)
                    fn["d"]()
                    torch.cuda.synchronize()
                    if not torch.equal(ref, out["a"]):
                        raise SystemExit(f"committee_msgs_indexed_bench: {kind} m={n}: the floor's flags differ")
                order = sorted(fn)
                ms = {k: [] for k in order}
                for _ in range(args.warmup):
                    for k in order:
                        one(fn[k])
                for _ in range(args.calls):
                    for k in order:
                        ms[k].append(one(fn[k]))
                p = {"kind": kind, "m": n, "route_of_a": route}
                for k in order:
                    p[k] = {"p50": pct(ms[k], 50), "p99": pct(ms[k], 99)}
                p["a_over_b"] = round(p["a"]["p50"] / p["b"]["p50"], 4)
                p["a_over_c"] = round(p["a"]["p50"] / p["c"]["p50"], 4)
                p["a_below_b_and_c"] = p["a"]["p50"] < p["b"]["p50"] and p["a"]["p50"] < p["c"]["p50"]
                if "d" in p:
                    p["a_over_d"] = round(p["a"]["p50"] / p["d"]["p50"], 4)
                rec["latency"].append(p)
                print(json.dumps(p), flush=True)
        rec["condition_a_below_b_and_c_everywhere"] = all(p["a_below_b_and_c"] for p in rec["latency"])

        n = args.throughput_items
        for kind in ("len32", "len416") if n else ():
            b = batch(n, kind)
            fn, out = legs(n, b)
            checked(n, {k: fn[k] for k in "abc"}, out, f"throughput {kind}")
            passes = []
            for _ in range(2):
                ms = {"a": [], "b": []}
                for it in range(3 + 12):
                    for k in ("a", "b"):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        fn[k]()
                        e1.record(stream)
                        e1.synchronize()
                        if it >= 3:
                            ms[k].append(e0.elapsed_time(e1))
                passes.append({k: round(float(np.median(v)), 4) for k, v in ms.items()})
            spread_b = round(abs(passes[0]["b"] - passes[1]["b"]), 4)
            a, bb = min(p["a"] for p in passes), min(p["b"] for p in passes)
            t = {"kind": kind, "items": n, "passes_median_ms": passes, "spread_of_b_between_passes_ms": spread_b,
                 "a_items_per_s": round(n / a * 1e3), "b_items_per_s": round(n / bb * 1e3),
                 "a_over_b": round(a / bb, 4),
                 "a_not_slower_beyond_spread": all(p["a"] <= p["b"] + spread_b for p in passes)}
            rec["throughput"].append(t)
            print(json.dumps(t), flush=True)
        committee.close()
        signer.close()

    rec["existing_paths"] = {}
    for spec in args.attach:
        name, path = spec.split("=", 1)
        with open(path) as f:
            text = f.read()
        try:
            rec["existing_paths"][name] = json.loads(text)
        except ValueError:   # one JSON object per line (bench.py's result lines)
            rec["existing_paths"][name] = [json.loads(l) for l in text.splitlines() if l.strip().startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "condition": rec["condition_a_below_b_and_c_everywhere"]}))


if __name__ == "__main__":
    main()
