#!/usr/bin/env python3
"""Serialized mempool batches: hsv_batches_verify_bincode* against the
transaction calls they replace.

Workload: transactions of `--tx-size` bytes (default 512, the reference
benchmark's), signed on the GPU by Signer.sign_transactions with 4 keys, in
bincode MempoolMessage::Batch messages of 15,000 B and 500,000 B (the local
benchmark's and the default batch_size: 30 and 977 transactions; a batch is
sealed by the transaction that reaches the size, mempool/src/batch_maker.rs).
Both sides of every comparison run in this process, alternating call by call
after a warm-up; the figure is the median (p50).

  host    one batch in host memory, wall clock around the call:
          a  hsv_batches_verify_bincode on the serialized bytes
          b  hsv_verify_transactions on the same transactions already packed
             (contiguous bytes + offsets)
          r  the repacking b needs and a does not, alone: hsv_batch_parse_bincode
             for the spans, then one copy of every transaction into a packed
             buffer and the offsets (numpy)
  device  1, 64 and 1024 batches of 500,000 B in HBM, device events around the call:
          a  hsv_batches_verify_bincode_device, tx_cap = the exact count
          b  hsv_verify_transactions_device on the same transactions packed
             contiguously, with precomputed offsets
          and the stages of a, each between two events (hsv_test_batch_stages,
          libhsv_test.so): parse (count, index, spans), record kernel,
          verification launch + mask, verdict kernel

Before any timing every batch must be HSV_BATCH_OK, a's flags must equal b's
byte for byte and every transaction must be STRICT_OK; a mismatch ends the run.
Writes one JSON record (--out).

    python tools/batch_wire_probe.py --out profiles/batch_wire_bench.json
"""
import argparse
import ctypes
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hotstuff-digital-signature-benchmarking_amd"))


def p50(ms, n):
    med = statistics.median(ms)
    return {"ms_p50": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "calls": len(ms),
            "tx_per_s_p50": round(n / med * 1e3)}


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def serialize_on_device(torch, txs):
    """(nb, n, size) uint8 transactions -> (nb, 12 + n * (8 + size)) bincode batches"""
    nb, n, size = txs.shape
    enc = torch.zeros((nb, 12 + n * (8 + size)), dtype=torch.uint8, device=txs.device)
    enc[:, 4:12] = torch.tensor(list(struct.pack("<Q", n)), dtype=torch.uint8, device=txs.device)
    body = enc[:, 12:].view(nb, n, 8 + size)
    body[:, :, :8] = torch.tensor(list(struct.pack("<Q", size)), dtype=torch.uint8, device=txs.device)
    body[:, :, 8:] = txs
    return enc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tx-size", type=int, default=512)
    ap.add_argument("--batch-bytes", type=int, nargs="+", default=[15000, 500000])
    ap.add_argument("--device-batches", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "batch_wire_bench.json"))
    args = ap.parse_args()

    import torch
    from hsverify import STRICT_OK, Signer, _lib, _testing, mempool, wire

    if _lib.device_count() <= 0:
        raise SystemExit("batch_wire_probe: no HIP device visible")
    size = args.tx_size
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(4711)
    per_batch = {b: -(-b // size) for b in args.batch_bytes}   # the transaction that reaches the size seals the batch
    big = max(args.batch_bytes)
    n_big = per_batch[big]
    total = max(args.device_batches) * n_big
    seeds = np.random.default_rng(4711).integers(0, 256, (4, 32), dtype=np.uint8)
    d_txs = torch.randint(0, 256, (total, size), generator=gen, dtype=torch.uint8).to(dev)
    key_idx = torch.randint(0, 4, (total,), generator=gen, dtype=torch.int32).to(dev)
    rec = {
        "what": "tools/batch_wire_probe.py: hsv_batches_verify_bincode* on serialized MempoolMessage::Batch bytes "
                "against the transaction calls on the same transactions already packed",
        "tx_size": size, "reps": args.reps, "warmup": args.warmup, "figure": "median (p50) of the timed calls",
        "checked": "every batch HSV_BATCH_OK, flags equal to the baseline's byte for byte, every transaction STRICT_OK",
        "host": {}, "device": {},
    }
    with _testing.test_library() as lib:
        rec["library"], rec["device_name"] = _lib.version(), torch.cuda.get_device_name(0)
        with Signer(seeds) as signer:
            signer.sign_transactions_device(d_txs, key_idx=key_idx)
        torch.cuda.synchronize()

        # ---- host form: one batch --------------------------------------------------------------
        for bb in args.batch_bytes:
            n = per_batch[bb]
            txs = d_txs[:n].cpu().numpy()
            tx_list = [t.tobytes() for t in txs]
            enc = np.frombuffer(wire.encode_batch(tx_list), np.uint8).copy()
            off2 = np.array([0, enc.size], np.uint64)
            res = (wire.BatchResult * 1)()
            flags_a, flags_b = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
            packed, offsets = mempool.pack(tx_list)
            p = lambda a: ctypes.c_void_p(a.ctypes.data)

            def leg_a():
                _lib.check(lib.hsv_batches_verify_bincode(None, p(enc), p(off2), 1, ctypes.cast(res, ctypes.c_void_p),
                                                          p(flags_a), n), "hsv_batches_verify_bincode")

            def leg_b():
                _lib.check(lib.hsv_verify_transactions(p(packed), p(offsets), n, p(flags_b)), "hsv_verify_transactions")

            def leg_r():
                cnt = ctypes.c_size_t(0)
                spans = np.empty(2 * n, np.uint64)
                _lib.check(lib.hsv_batch_parse_bincode(p(enc), enc.size, ctypes.byref(cnt), p(spans), spans.size),
                           "hsv_batch_parse_bincode")
                lo, hi = spans[0::2].astype(np.int64), spans[1::2].astype(np.int64)
                out = np.empty(int((hi - lo).sum()), np.uint8)
                offs = np.zeros(n + 1, np.uint64)
                np.cumsum(hi - lo, out=offs[1:].view(np.int64))
                for i in range(n):
                    out[int(offs[i]):int(offs[i + 1])] = enc[lo[i]:hi[i]]
                return out, offs

            leg_a(), leg_b()
            if res[0].as_tuple() != (wire.BATCH_OK, 0, n, 0) or not (flags_a == flags_b).all() or \
                    not (flags_a & STRICT_OK).all():
                raise SystemExit(f"batch_wire_probe: host form, {bb} B: wrong result {res[0].as_tuple()}")
            out, offs = leg_r()
            if not (out == packed).all() or not (offs == offsets).all():
                raise SystemExit("batch_wire_probe: the repack leg does not reproduce the packed layout")
            legs = {"a": leg_a, "b": leg_b, "r": leg_r}
            for _ in range(args.warmup):
                for fn in legs.values():
                    fn()
            ms = {k: [] for k in legs}
            for _ in range(args.reps):
                for k, fn in legs.items():
                    ms[k].append(wall(fn))
            o = {k: p50(v, n) for k, v in ms.items()}
            o["n_tx"], o["batch_bytes_encoded"] = n, int(enc.size)
            o["a_time_over_b"] = round(o["a"]["ms_p50"] / o["b"]["ms_p50"], 3)
            o["a_time_over_b_plus_r"] = round(o["a"]["ms_p50"] / (o["b"]["ms_p50"] + o["r"]["ms_p50"]), 3)
            rec["host"][str(bb)] = o
            print(json.dumps({"host": bb, **{k: o[k]["ms_p50"] for k in legs}, "a_over_b": o["a_time_over_b"]}), flush=True)

        # ---- device form: batches of the largest size in HBM -----------------------------------
        for nb in args.device_batches:
            n = nb * n_big
            txs = d_txs[:n]
            enc = serialize_on_device(torch, txs.view(nb, n_big, size))
            blen = enc.shape[1]
            d_off = (torch.arange(nb + 1, dtype=torch.int64) * blen).to(dev)
            d_txoff = (torch.arange(n + 1, dtype=torch.int64) * size).to(dev)
            results = torch.zeros(3 * nb, dtype=torch.int64, device=dev)
            flags_a = torch.full((n,), 0xff, dtype=torch.uint8, device=dev)
            flags_b = torch.full((n,), 0xff, dtype=torch.uint8, device=dev)
            fault = torch.zeros(2, dtype=torch.int32, device=dev)
            stage_ms = (ctypes.c_float * 4)()

            def leg_a():
                wire.batches_verify_device(enc, d_off, nb, n, results, flags=flags_a, fault=fault)

            def leg_b():
                mempool.verify_transactions_device(txs, d_txoff, n=n, flags=flags_b, fault=fault)

            def stages():
                _lib.check(lib.hsv_test_batch_stages(ctypes.c_void_p(enc.data_ptr()), ctypes.c_void_p(d_off.data_ptr()),
                                                     nb, n, ctypes.c_void_p(results.data_ptr()), stage_ms),
                           "hsv_test_batch_stages")
                return list(stage_ms)

            leg_a(), leg_b()
            torch.cuda.synchronize()
            got = wire.batch_results(results.cpu().numpy())
            if fault.cpu().tolist() != [0, 0]:
                raise SystemExit(f"batch_wire_probe: {nb} batches: a device self-check failed")
            if got != [(wire.BATCH_OK, 0, n_big, b * n_big) for b in range(nb)]:
                raise SystemExit(f"batch_wire_probe: {nb} batches: wrong verdicts {got[:3]}")
            if not torch.equal(flags_a, flags_b) or not bool((flags_a & STRICT_OK).all()):
                raise SystemExit(f"batch_wire_probe: {nb} batches: flags differ from hsv_verify_transactions_device")
            for _ in range(args.warmup):
                leg_a(), leg_b(), stages()
            torch.cuda.synchronize()
            ms = {"a": [], "b": []}
            st = []
            for _ in range(args.reps):
                ms["a"].append(timed(torch, leg_a))
                ms["b"].append(timed(torch, leg_b))
                st.append(stages())
            o = {k: p50(v, n) for k, v in ms.items()}
            o["n_tx"], o["batch_bytes_encoded"], o["n_batches"] = n, int(blen), nb
            o["a_time_over_b"] = round(o["a"]["ms_p50"] / o["b"]["ms_p50"], 3)
            o["stages_ms_p50"] = {name: round(statistics.median(s[i] for s in st), 4)
                                  for i, name in enumerate(("parse", "records", "verify_and_mask", "verdicts"))}
            rec["device"][str(nb)] = o
            print(json.dumps({"device_batches": nb, "a": o["a"]["ms_p50"], "b": o["b"]["ms_p50"],
                              "a_over_b": o["a_time_over_b"], **o["stages_ms_p50"]}), flush=True)
            del enc, flags_a, flags_b, results, d_txoff
    rec["legs"] = {
        "host.a": "hsv_batches_verify_bincode, one serialized batch (the host parses, one staged round)",
        "host.b": "hsv_verify_transactions on the same transactions packed contiguously with offsets",
        "host.r": "the repacking b needs: hsv_batch_parse_bincode + one copy per transaction into a packed buffer (numpy)",
        "device.a": "hsv_batches_verify_bincode_device, tx_cap = the exact count, flags written",
        "device.b": "hsv_verify_transactions_device on the same transactions packed contiguously, precomputed offsets",
        "device.stages_ms_p50": "hsv_test_batch_stages: parse (count, index, span kernels), span-mode record kernel, "
                                "verification launch over the records + mask, verdict kernel",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
