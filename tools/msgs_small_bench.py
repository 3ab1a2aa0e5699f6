#!/usr/bin/env python3
"""Latency of hsv_verify_msgs_device at small batch sizes: the small forms'
message instantiations (one launch, the default at <= 2^13 items) against the
message prepass + point pass (two launches, the route of larger batches), and
against hsv_verify_device over the same triples at 32 bytes.

One process, inputs resident in HBM, every signature valid and checked so under
both routes before anything is timed.  Per point (n, length): 3 warm-up calls
and --calls timed calls per route, each call followed by a synchronise of its
stream and timed with the host clock around both; the two routes alternate in
blocks of --block calls (the test library's hsv_test_msgs_small moves the
route: -1 by n, 0 two launches).  Reports p50 and p99 in ms, the form the
default route took (hsv_test_msgs_form_counts), and whether the default's p50
is no higher than the two-launch route's.  The floor runs with the automatic
committee cache and the resident latency service off.

    python tools/msgs_small_bench.py --out profiles/msgs_small_latency.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hotstuff-digital-signature-benchmarking_amd"))

SIZES = (1, 67, 256, 257, 667, 768, 769, 3072, 3073, 8192)
FORMS = ("two_launch", "quad", "joint", "row", "pair")


def pct(ms, q):
    return round(float(np.percentile(np.asarray(ms), q)), 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=300, help="timed calls per route and point (>= 300)")
    ap.add_argument("--block", type=int, default=50, help="calls of one route before the other takes its turn")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=8100)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--kinds", nargs="*", default=None, help="a subset of len32 len100 len416 ragged_0_1024 "
                    "(a kernel trace of one length, say)")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "msgs_small_latency.json"))
    args = ap.parse_args()

    import torch
    from hsverify import Signer, _lib, _testing, verifier

    if _lib.device_count() <= 0:
        raise SystemExit("msgs_small_bench: no HIP device visible (there is no CPU form of the verifier)")
    dev = torch.device("cuda:0")
    rnd = np.random.default_rng(args.seed)
    nmax = max(args.sizes)
    seeds = rnd.integers(0, 256, (nmax, 32), dtype=np.uint8)

    with _testing.test_library() as lib:
        lib.hsv_set_auto_committee(0)
        lib.hsv_set_resident_service(0)
        stream = torch.cuda.current_stream(dev)

        def counts():
            out = (ctypes.c_uint64 * 5)()
            lib.hsv_test_msgs_form_counts(out)
            return np.array(list(out), np.int64)

        def one(fn):
            t0 = time.perf_counter()
            fn()
            stream.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def all_valid(flags, fault, what):
            torch.cuda.synchronize()
            if fault.cpu().tolist() != [0, 0]:
                raise SystemExit(f"msgs_small_bench: {what}: device self-check words {fault.cpu().tolist()}")
            bad = int((flags & 1).eq(0).sum())
            if bad:
                raise SystemExit(f"msgs_small_bench: {what}: {bad} valid signatures rejected")

        def alternate(fns):
            """ms per call of each (route, fn), the routes alternating in blocks"""
            out = [[] for _ in fns]
            for mode, fn in fns:
                lib.hsv_test_msgs_small(mode)
                for _ in range(args.warmup):
                    one(fn)
            done = 0
            while done < args.calls:
                m = min(args.block, args.calls - done)
                for k, (mode, fn) in enumerate(fns):
                    lib.hsv_test_msgs_small(mode)
                    out[k] += [one(fn) for _ in range(m)]
                done += m
            lib.hsv_test_msgs_small(-1)
            return out

        # the batches of nmax items, signed once on the host; smaller sizes are prefixes
        kinds = {}
        for length in (32, 100, 416):
            msgs = rnd.integers(0, 256, (nmax, length), dtype=np.uint8)
            pk, sig = verifier.sign_many(seeds, msgs)
            kinds[f"len{length}"] = (pk, sig, msgs.reshape(-1), None, length)
        # ragged: the packed buffer signed on the GPU in one call (Signer.sign_msgs_device)
        lens = rnd.integers(0, 1025, nmax)
        off = np.zeros(nmax + 1, np.int64)
        off[1:] = np.cumsum(lens)
        buf = rnd.integers(0, 256, int(off[-1]), dtype=np.uint8)
        with Signer(seeds) as signer:
            d_sig = torch.zeros((nmax, 64), dtype=torch.uint8, device=dev)
            fault = torch.zeros(2, dtype=torch.int32, device=dev)
            signer.sign_msgs_device(torch.from_numpy(buf).to(dev), d_sig, offsets=torch.from_numpy(off).to(dev),
                                    fault=fault)
            torch.cuda.synchronize()
            if fault.cpu().tolist() != [0, 0]:
                raise SystemExit(f"msgs_small_bench: signing the ragged batch: self-check words {fault.cpu().tolist()}")
            kinds["ragged_0_1024"] = (signer.public_keys(), d_sig.cpu().numpy(), buf, off, 0)

        rec = {"what": "tools/msgs_small_bench.py: hsv_verify_msgs_device, default route (a small form, one launch) "
                       "against two launches (hsv_test_msgs_small 0), one process, alternating blocks",
               "library": _lib.version(), "device": torch.cuda.get_device_name(0), "calls_per_route": args.calls,
               "block": args.block, "warmup": args.warmup,
               "timing": "host clock around the call and a synchronise of its stream, ms",
               "checked": "every signature valid; flags all STRICT_OK and fault words zero under both routes "
                          "before timing", "points": []}
        worst = 0.0
        for kind, (pk, sig, buf, off, length) in kinds.items():
            if args.kinds and kind not in args.kinds:
                continue
            d_pk, d_sig = torch.from_numpy(pk).to(dev), torch.from_numpy(sig).to(dev)
            # the messages 3 bytes off a 16-byte boundary, as a caller's buffer usually is
            raw = torch.zeros(buf.size + 19, dtype=torch.uint8, device=dev)
            raw[3:3 + buf.size].copy_(torch.from_numpy(np.ascontiguousarray(buf)))
            d_off = torch.from_numpy(off).to(dev) if off is not None else None
            for n in args.sizes:
                flags = torch.zeros(n, dtype=torch.uint8, device=dev)
                fault = torch.zeros(2, dtype=torch.int32, device=dev)
                call = lambda fault=None: verifier.verify_msgs_device(
                    d_pk[:n], d_sig[:n], raw[3:], d_off[:n + 1] if d_off is not None else None, msg_len=length,
                    flags=flags, fault=fault)
                form = None
                for mode in (-1, 0):
                    lib.hsv_test_msgs_small(mode)
                    before = counts()
                    flags.zero_()
                    call(fault)
                    all_valid(flags, fault, f"{kind} n={n} route {mode}")
                    moved = counts() - before
                    if mode == -1:
                        form = FORMS[int(np.argmax(moved))]
                a, b = alternate([(-1, call), (0, call)])
                p = {"kind": kind, "n": n, "default_form": form,
                     "default": {"p50": pct(a, 50), "p99": pct(a, 99)},
                     "two_launch": {"p50": pct(b, 50), "p99": pct(b, 99)}}
                p["p50_ratio"] = round(p["default"]["p50"] / p["two_launch"]["p50"], 4)
                p["default_no_slower"] = p["default"]["p50"] <= p["two_launch"]["p50"]
                worst = max(worst, p["p50_ratio"])
                if kind == "len32":
                    d_msg = torch.from_numpy(np.ascontiguousarray(buf[:n * 32]).reshape(n, 32)).to(dev)
                    ref = torch.zeros(n, dtype=torch.uint8, device=dev)
                    verifier.verify_device(d_pk[:n], d_sig[:n], d_msg, flags=ref, fault=fault)
                    all_valid(ref, fault, f"hsv_verify_device n={n}")
                    (f,) = alternate([(-1, lambda: verifier.verify_device(d_pk[:n], d_sig[:n], d_msg, flags=ref))])
                    p["floor_hsv_verify_device"] = {"p50": pct(f, 50), "p99": pct(f, 99)}
                    p["default_over_floor"] = round(p["default"]["p50"] / p["floor_hsv_verify_device"]["p50"], 4)
                rec["points"].append(p)
                print(json.dumps(p), flush=True)
        rec["worst_p50_ratio_default_over_two_launch"] = worst
        rec["condition_default_no_slower_everywhere"] = all(p["default_no_slower"] for p in rec["points"])

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "worst_p50_ratio": worst,
                      "condition": rec["condition_default_no_slower_everywhere"]}))


if __name__ == "__main__":
    main()
