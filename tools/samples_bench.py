#!/usr/bin/env python3
"""The benchmark's sample transactions on the device: what the sample index and
the client's bursts cost beside the calls they stand next to.

Workload, device-resident, in one process: n (default 2^20) transactions of 512
bytes from synth.client_bursts_gpu with burst 1000, signed on the GPU, verified,
and sealed at batch_size 500,000 with flush.
Legs, alternating call by call after a warm-up, each call between device events:
  index    hsv_batches_samples_bincode_device on the seal's (d_out, d_batch_offsets),
           n_batches = batches_cap, tx_cap = n
  seal     hsv_seal_transactions_device on the same transactions (no digests)
  verify   hsv_batches_verify_bincode_device on the same batches
  bursts   hsv_client_bursts_device (trailer 96) into a second buffer
  memset   hipMemsetAsync of the bytes the bursts write, n * (tx_size - 96)
  sign     hsv_signer_sign_transactions_device on that buffer
Before any timing the transactions must equal the client loop's (a numpy
restatement), every flag must say HSV_STRICT_OK, and the index must equal the
one computed from the burst arithmetic and the greedy cut.  Writes one JSON
record.

    python tools/samples_bench.py --out profiles/samples_bench.json
"""
import argparse
import ctypes
import json
import os
import platform
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


def stats(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "calls": len(ms)}


def hip_runtime():
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
        try:
            lib = ctypes.CDLL(name)
            lib.hipMemsetAsync.restype = ctypes.c_int
            lib.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
            return lib
        except OSError:
            continue
    raise SystemExit("samples_bench: the HIP runtime library is not loadable")


def client_preambles(n, burst, counter0, r0):
    """client.rs:121-133 for transactions 0..n-1 -> (is_sample, the u64 behind the tag)"""
    i = np.arange(n, dtype=np.uint64)
    c = np.uint64(counter0) + i // np.uint64(burst)
    is_sample = i % np.uint64(burst) == c % np.uint64(burst)
    r = np.uint64(r0) + np.cumsum(~is_sample, dtype=np.uint64)
    return is_sample, np.where(is_sample, c, r)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--tx-size", type=int, default=512)
    ap.add_argument("--burst", type=int, default=1000)
    ap.add_argument("--batch-size", type=int, default=500_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "samples_bench.json"))
    args = ap.parse_args()

    import torch
    from hsverify import Signer, _lib, mempool, synth, wire

    if _lib.device_count() <= 0:
        raise SystemExit("samples_bench: no HIP device visible")
    n, size, burst, counter0, r0 = args.n, args.tx_size, args.burst, 7, 1 << 40
    dev = torch.device("cuda:0")
    hip = hip_runtime()
    rnd = np.random.default_rng(2718)
    seeds = rnd.integers(0, 256, (64, 32), dtype=np.uint8)
    key_idx = torch.from_numpy(rnd.integers(0, 64, n).astype(np.int32)).to(dev)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    with Signer(seeds) as signer:
        d_txs, _ = synth.client_bursts_gpu(n, size, burst, counter0, r0, signer=signer, key_idx=key_idx)
        d_flags = torch.zeros(n, dtype=torch.uint8, device=dev)
        mempool.verify_transactions_device(d_txs, None, tx_size=size, n=n, flags=d_flags)
        cap, bcap = mempool.seal_bound(n * size, n, args.batch_size)
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        boff = torch.empty(bcap + 1, dtype=torch.int64, device=dev)
        summ = torch.empty(8, dtype=torch.int64, device=dev)
        seal = lambda: mempool.seal_device(d_txs, None, size, n, d_flags, args.batch_size, True, out=out,
                                           batch_offsets=boff, summary_out=summ)
        seal()
        index = torch.empty((bcap, 5), dtype=torch.int64, device=dev)
        ids = torch.empty(n, dtype=torch.int64, device=dev)
        do_index = lambda: mempool.batches_samples_device(out, boff, n, bcap, index=index, ids=ids)
        do_index()
        torch.cuda.synchronize()

        # correctness first
        is_sample, value = client_preambles(n, burst, counter0, r0)
        head = d_txs[:, :9].cpu().numpy()
        want_head = np.concatenate([(~is_sample).astype(np.uint8)[:, None],
                                    value.astype(">u8").view(np.uint8).reshape(n, 8)], axis=1)
        if not (head == want_head).all() or int(d_txs[:, 9:size - 96].max()) != 0:
            raise SystemExit("samples_bench: the transactions are not the client loop's")
        if not (d_flags.cpu().numpy() & 1).all():
            raise SystemExit("samples_bench: a signed transaction does not verify")
        per = -(-args.batch_size // size)  # transactions per full batch
        k = -(-n // per)
        s = mempool.SealSummary.from_words(summ.cpu().numpy()).as_dict()
        if s["status"] != 0 or s["n_batches"] != k or s["sealed"] != n:
            raise SystemExit(f"samples_bench: seal summary {s}, expected {k} batches of {n} transactions")
        rows = index.cpu().numpy().view(np.uint64)
        got_ids = ids.cpu().numpy().view(np.uint64)
        before = np.concatenate([[0], np.cumsum(is_sample)])
        for b in range(bcap):
            lo, hi = min(b * per, n), min((b + 1) * per, n)
            want = ([0, hi - lo, (hi - lo) * size, before[hi] - before[lo], before[lo]] if b < k else [2, 0, 0, 0, 0])
            if rows[b].tolist() != [int(x) for x in want]:
                raise SystemExit(f"samples_bench: index row {b} is {rows[b].tolist()}, expected {want}")
        total = int(before[n])
        if not (got_ids[:total] == value[is_sample]).all():
            raise SystemExit("samples_bench: the ids are not the sample counters in order")

        results = torch.empty(3 * bcap, dtype=torch.int64, device=dev)
        vflags = torch.empty(n, dtype=torch.uint8, device=dev)
        fault = torch.zeros(2, dtype=torch.int32, device=dev)
        d_fill = torch.zeros((n, size), dtype=torch.uint8, device=dev)
        body = n * (size - 96)
        legs = {
            "index": do_index,
            "seal": seal,
            "verify": lambda: wire.batches_verify_device(out, boff, bcap, n, results, flags=vflags, fault=fault),
            "bursts": lambda: synth.client_bursts_gpu(n, size, burst, counter0, r0, out=d_fill),
            "memset": lambda: hip.hipMemsetAsync(d_fill.data_ptr(), 0, body, stream()),
            "sign": lambda: signer.sign_transactions_device(d_fill, key_idx=key_idx),
        }
        for _ in range(args.warmup):
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        ms = {leg: [] for leg in legs}
        for _ in range(args.reps):
            for leg, fn in legs.items():
                ms[leg].append(timed(torch, fn))
        good = [r[0] for r in wire.batch_results(results.cpu().numpy())[:k]]
        if fault.cpu().tolist() != [0, 0] or any(g != 0 for g in good):
            raise SystemExit("samples_bench: the verify leg does not pass the sealed batches")

    rec = {"what": "tools/samples_bench.py: hsv_batches_samples_bincode_device beside hsv_seal_transactions_device and "
                   "hsv_batches_verify_bincode_device on the same batches; hsv_client_bursts_device beside a "
                   "hipMemsetAsync of the bytes it writes and hsv_signer_sign_transactions_device on its result",
           "n": n, "tx_size": size, "burst": burst, "batch_size": args.batch_size, "n_batches": k, "batches_cap": bcap,
           "samples": total, "bytes_sealed": s["bytes"], "bytes_written_by_bursts": body,
           "reps": args.reps, "warmup": args.warmup,
           "timing": "device events around each call, legs alternating call by call in one process, after the warm-up",
           "checked": "transactions equal the client loop; every flag HSV_STRICT_OK; index rows and ids from the burst "
                      "arithmetic and the greedy cut; the verify leg passes every sealed batch",
           "library": _lib.version(), "device": torch.cuda.get_device_name(0),
           "box": {"host_cpu": platform.processor() or platform.machine(), "cpus_visible": os.cpu_count(),
                   "torch": torch.__version__, "hip": getattr(torch.version, "hip", None),
                   "devices_visible": torch.cuda.device_count()},
           **{leg: stats(v) for leg, v in ms.items()}}
    med = lambda leg: rec[leg]["ms_median"]
    rec["ratios"] = {"index_over_seal": round(med("index") / med("seal"), 3),
                     "index_over_verify": round(med("index") / med("verify"), 4),
                     "bursts_over_memset": round(med("bursts") / med("memset"), 3),
                     "bursts_over_sign": round(med("bursts") / med("sign"), 5),
                     "bursts_GBps_written": round(body / med("bursts") / 1e6, 1),
                     "memset_GBps_written": round(body / med("memset") / 1e6, 1)}
    print(json.dumps({**{leg: med(leg) for leg in legs}, **rec["ratios"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
