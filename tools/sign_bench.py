#!/usr/bin/env python3
"""Batch signing on the GPU against the host signer.

Workload: n keys (default 2^20), n 32-byte digests, `--inputs` seeded input
sets.  For every input set, in one process and alternating:

  baseline   hsv_sign_many on 16 host threads (seed -> pk and signature): the
             only way to sign before the GPU signer, and the reference bytes
  keygen     Signer(seeds): key expansion on the GPU, wall time of the call
             (seed upload, kernel, public keys read back)
  host       Signer.sign over host arrays, wall time (copies included)
  device     Signer.sign_device over device tensors, device events, per call
  groups     the device form at every built G (items per lane sharing one
             field inversion; G = 1 is the unbatched form)

Every GPU public key and signature of every input set is compared byte for
byte with the baseline's before any timing is taken from it; a mismatch ends
the run.  Writes one JSON record (--out).

    python tools/sign_bench.py --out profiles/sign_bench.json
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

GROUPS = (1, 2, 4, 8, 16)


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
    ap.add_argument("--inputs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "sign_bench.json"))
    args = ap.parse_args()

    import torch
    from hsverify import Signer, _lib, _testing
    from hsverify.verifier import sign_many

    n = args.n
    with _testing.test_library() as lib:
        if lib.hsv_device_count() <= 0:
            raise SystemExit("sign_bench: no HIP device visible (there is no CPU form of the signer)")
        product_group = lib.hsv_test_signer_group(0)
        dev = torch.device("cuda:0")
        base_ms, keygen_ms, host_ms, dev_ms = [], [], [], []
        group_ms = {g: [] for g in GROUPS}
        Signer(np.zeros((64, 32), np.uint8)).close()  # context, B table and code objects before the first timed call
        for k in range(args.inputs):
            rnd = np.random.default_rng(7000 + k)
            seeds = rnd.integers(0, 256, (n, 32), dtype=np.uint8)
            msgs = rnd.integers(0, 256, (n, 32), dtype=np.uint8)
            t = time.perf_counter()
            pk_ref, sig_ref = sign_many(seeds, msgs, nthreads=args.threads)
            base_ms.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            signer = Signer(seeds)
            keygen_ms.append((time.perf_counter() - t) * 1e3)
            if not (signer.public_keys() == pk_ref).all():
                raise SystemExit(f"sign_bench: input set {k}: GPU public keys differ from hsv_sign_many")
            t = time.perf_counter()
            sig = signer.sign(msgs)
            host_ms.append((time.perf_counter() - t) * 1e3)
            if not (sig == sig_ref).all():
                raise SystemExit(f"sign_bench: input set {k}: GPU signatures (host form) differ from hsv_sign_many")
            d_msg = torch.from_numpy(msgs).to(dev)
            d_sig = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
            fault = torch.zeros(2, dtype=torch.int32, device=dev)
            # the product's G as "the device form", then every built G (the product's again among them)
            for sink, g in [(dev_ms, product_group)] + [(group_ms[g], g) for g in GROUPS]:
                if lib.hsv_test_signer_group(g) < 0:
                    raise SystemExit(f"sign_bench: G = {g} is not built")
                d_sig.zero_()
                signer.sign_device(d_msg, d_sig, fault=fault)
                torch.cuda.synchronize()
                if fault.cpu().tolist() != [0, 0] or not (d_sig.cpu().numpy() == sig_ref).all():
                    raise SystemExit(f"sign_bench: input set {k}, G = {g}: device-form signatures differ")
                sink.extend(device_times(torch, lambda: signer.sign_device(d_msg, d_sig), args.warmup, args.reps))
            lib.hsv_test_signer_group(0)
            signer.close()
            del d_msg, d_sig
        base = statistics.median(base_ms)
        rec = {
            "what": "tools/sign_bench.py: GPU batch signing against hsv_sign_many",
            "library": _lib.version(),
            "device": torch.cuda.get_device_name(0),
            "n": n, "msg_len": 32, "input_sets": args.inputs, "reps_per_input_set": args.reps,
            "checked": "all public keys and signatures of every input set, host form, device form and every G, "
                       "byte for byte against hsv_sign_many",
            "product_group": product_group,
            "baseline_sign_many": dict(summary(base_ms, n), threads=args.threads,
                                       note="seed -> pk and signature per item, host wall time"),
            "gpu_keygen_create": dict(summary(keygen_ms, n), note="hsv_signer_create wall time: upload, kernel, pk read-back"),
            "gpu_sign_host_form": dict(summary(host_ms, n), note="hsv_signer_sign wall time: copies both ways included"),
            "gpu_sign_device_form": dict(summary(dev_ms, n), note="hsv_signer_sign_device, device events"),
            "gpu_sign_device_form_by_group": {str(g): summary(group_ms[g], n) for g in GROUPS},
        }
        dev_med = rec["gpu_sign_device_form"]["ms_median"]
        g1 = rec["gpu_sign_device_form_by_group"]["1"]["ms_median"]
        gp = rec["gpu_sign_device_form_by_group"][str(product_group)]["ms_median"]
        rec["ratios"] = {
            "device_form_vs_baseline": round(base / dev_med, 1),
            "host_form_vs_baseline": round(base / statistics.median(host_ms), 1),
            "keygen_plus_host_form_vs_baseline": round(base / (statistics.median(keygen_ms) + statistics.median(host_ms)), 1),
            "product_group_vs_group_1": round(g1 / gp, 2),
        }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["ratios"] | {"device_form_per_s": rec["gpu_sign_device_form"]["per_s_median"],
                                      "baseline_per_s": rec["baseline_sign_many"]["per_s_median"], "out": args.out}))


if __name__ == "__main__":
    main()
