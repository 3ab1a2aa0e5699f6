#!/usr/bin/env python3
"""Signing mempool transactions on the GPU against the host route.

Workload: n transactions (default 2^20) of `--tx-size` bytes (default 512), one
key per item, seeded.  In one process:

  host route  hashlib SHA-512 per message plus hsv_sign_many on 16 host
              threads -- what hsverify.synth.transactions does -- timed on
              `--host-n` items (default 2^16; the rate is that run's, not an
              extrapolation) and kept as the reference bytes
  device      Signer.sign_transactions_device in place on a device tensor,
              device events, per call
  floor       Signer.sign_device over n 32-byte digests with the same keys, the
              same way: transaction signing does that work plus one message
              hash per item
  host form   Signer.sign_transactions over a host array, wall time (copies
              both ways included)
  ragged      the device form over lengths drawn from 96 ... 1120

Before any timing is taken from it, the GPU output of each form is compared
byte for byte with the host route on the first `--host-n` items, and ALL items
must pass the mempool verifier (hsv_verify_transactions_device, STRICT_OK); a
mismatch ends the run.  Writes one JSON record (--out).

    python tools/tx_sign_bench.py --out profiles/tx_sign_bench_2p20.json
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hotstuff-digital-signature-benchmarking_amd"))


def device_times(torch, fn, warmup, reps):
    """ms per call of fn() by device events on the current stream."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def summary(ms, n):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "calls": len(ms),
            "per_s_median": round(n / med * 1e3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--tx-size", type=int, default=512)
    ap.add_argument("--host-n", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--device-only", action="store_true",
                    help="only the device form (for a kernel trace of the two launches); writes no record")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "tx_sign_bench.json"))
    args = ap.parse_args()

    import torch
    from hsverify import STRICT_OK, Signer, _lib, mempool
    from hsverify.verifier import sign_many

    if _lib.device_count() <= 0:
        raise SystemExit("tx_sign_bench: no HIP device visible (there is no CPU form of the signer)")
    n, size, hn = args.n, args.tx_size, min(args.host_n, args.n)
    mlen = size - 96
    dev = torch.device("cuda:0")
    rnd = np.random.default_rng(9000)
    seeds = rnd.integers(0, 256, (n, 32), dtype=np.uint8)
    txs = np.zeros((n, size), np.uint8)
    txs[:, :mlen] = rnd.integers(0, 256, (n, mlen), dtype=np.uint8)

    # the host route, on the first hn items
    t = time.perf_counter()
    dig = np.empty((hn, 32), np.uint8)
    for i in range(hn):
        dig[i] = np.frombuffer(hashlib.sha512(txs[i, :mlen].tobytes()).digest()[:32], np.uint8)
    t_hash = time.perf_counter() - t
    pk_ref, sig_ref = sign_many(seeds[:hn], dig, nthreads=args.threads)
    host_route_ms = (time.perf_counter() - t) * 1e3
    want = txs[:hn].copy()
    want[:, mlen:mlen + 32], want[:, mlen + 32:] = pk_ref, sig_ref

    def check(d_txs, d_offsets, count, what, tx_size):
        flags = torch.zeros(count, dtype=torch.uint8, device=dev)
        fault = torch.ones(2, dtype=torch.int32, device=dev)
        mempool.verify_transactions_device(d_txs, offsets=d_offsets, tx_size=tx_size, n=count, flags=flags, fault=fault)
        torch.cuda.synchronize()
        if fault.cpu().tolist() != [0, 0] or not bool((flags & STRICT_OK).all()):
            raise SystemExit(f"tx_sign_bench: {what}: the mempool verifier rejects a signed transaction")

    signer = Signer(seeds)
    d_txs = torch.from_numpy(txs).to(dev)
    fault = torch.ones(2, dtype=torch.int32, device=dev)
    signer.sign_transactions_device(d_txs, fault=fault)
    torch.cuda.synchronize()
    if fault.cpu().tolist() != [0, 0] or not (d_txs[:hn].cpu().numpy() == want).all():
        raise SystemExit("tx_sign_bench: device form differs from the host route")
    check(d_txs, None, n, "device form", size)
    dev_ms = device_times(torch, lambda: signer.sign_transactions_device(d_txs), args.warmup, args.reps)
    if args.device_only:
        print(json.dumps({"device_form": summary(dev_ms, n)}))
        return

    # the floor: the same keys over 32-byte digests
    d_dig = torch.from_numpy(rnd.integers(0, 256, (n, 32), dtype=np.uint8)).to(dev)
    d_sig = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    floor_ms = device_times(torch, lambda: signer.sign_device(d_dig, d_sig), args.warmup, args.reps)
    del d_dig, d_sig

    # the host-buffer form
    host_ms = []
    for k in range(args.host_reps + 1):
        t = time.perf_counter()
        got = signer.sign_transactions(txs)
        if k:
            host_ms.append((time.perf_counter() - t) * 1e3)
        elif not (got[:hn] == want).all() or not (got == d_txs.cpu().numpy()).all():
            raise SystemExit("tx_sign_bench: host form differs from the host route or the device form")
    del got, d_txs

    # ragged: lengths 96 ... 1120
    lens = rnd.integers(96, 1121, n).astype(np.int64)
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    rag = rnd.integers(0, 256, int(offsets[-1]), dtype=np.uint8)
    d_rag, d_off = torch.from_numpy(rag).to(dev), torch.from_numpy(offsets).to(dev)
    signer.sign_transactions_device(d_rag, offsets=d_off, fault=fault)
    torch.cuda.synchronize()
    head = d_rag[:int(offsets[256])].cpu().numpy()
    for i in range(256):
        a, b = int(offsets[i]), int(offsets[i + 1])
        d = np.frombuffer(hashlib.sha512(rag[a:b - 96].tobytes()).digest()[:32], np.uint8)[None]
        pk, sg = sign_many(seeds[i:i + 1], d, nthreads=1)
        if bytes(head[a:b]) != rag[a:b - 96].tobytes() + bytes(pk[0]) + bytes(sg[0]):
            raise SystemExit(f"tx_sign_bench: ragged item {i} differs from the host route")
    check(d_rag, d_off, n, "ragged device form", 0)
    rag_ms = device_times(torch, lambda: signer.sign_transactions_device(d_rag, offsets=d_off), args.warmup, args.reps)
    signer.close()

    rec = {
        "what": "tools/tx_sign_bench.py: mempool transactions signed on the GPU against the host route",
        "library": _lib.version(),
        "device": torch.cuda.get_device_name(0),
        "n": n, "tx_size": size, "reps": args.reps, "warmup": args.warmup,
        "checked": f"device, host and ragged form byte for byte against hashlib + hsv_sign_many on the first "
                   f"{hn} (ragged: 256) items; every item of every form STRICT_OK from hsv_verify_transactions_device",
        "device_form": dict(summary(dev_ms, n), note="hsv_signer_sign_transactions_device, device events, in place"),
        "floor_sign_device_32B": dict(summary(floor_ms, n),
                                      note="hsv_signer_sign_device over n 32-byte digests, same keys, device events"),
        "host_form": dict(summary(host_ms, n), note="hsv_signer_sign_transactions wall time, copies both ways included"),
        "ragged_device_form": dict(summary(rag_ms, n), lengths="uniform 96 ... 1120", bytes=int(offsets[-1])),
        "host_route": {"items": hn, "threads": args.threads, "ms": round(host_route_ms, 2),
                       "hashlib_ms": round(t_hash * 1e3, 2), "per_s": round(hn / host_route_ms * 1e3),
                       "note": f"hashlib loop + hsv_sign_many, timed on {hn} items (not extrapolated to n)"},
    }
    d = rec["device_form"]["ms_median"]
    rec["ratios"] = {
        "device_form_vs_floor": round(d / rec["floor_sign_device_32B"]["ms_median"], 3),
        "ragged_vs_device_form": round(rec["ragged_device_form"]["ms_median"] / d, 3),
        "device_form_rate_vs_host_route_rate": round(rec["device_form"]["per_s_median"] / rec["host_route"]["per_s"], 1),
        "host_form_rate_vs_host_route_rate": round(rec["host_form"]["per_s_median"] / rec["host_route"]["per_s"], 1),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["ratios"] | {"device_form_tx_per_s": rec["device_form"]["per_s_median"],
                                      "host_route_tx_per_s": rec["host_route"]["per_s"], "out": args.out}))


if __name__ == "__main__":
    main()
