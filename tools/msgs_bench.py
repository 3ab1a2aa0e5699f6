#!/usr/bin/env python3
"""Verification over messages of any length against the 32-byte path and the
mempool path.

n items (default 2^20), inputs resident in HBM, keys and signatures from the
GPU signer.  In one process, alternating per repetition and timed with device
events:

  len32    hsv_verify_msgs_device at msg_len 32 against hsv_verify_device on
           the same triples (flags compared before any timing);
  len416   hsv_verify_msgs_device at msg_len 416 against
           hsv_verify_transactions_device on 512-byte transactions holding the
           same message bytes (there the signature is over
           SHA-512(message)[..32]); the same transactions with HSV_TX_FUSED=0,
           the two-launch form of that shape, in a second process;
  ragged   lengths uniform in 0..1024, packed back to back in random order.

Every signature is valid, and every call's flags must say so (and its fault
words stay zero) before it is timed.  Writes one JSON record (--out).

    python tools/msgs_bench.py --out profiles/msgs_bench_2p20.json
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hotstuff-digital-signature-benchmarking_amd"))


def timed(torch, fns, warmup, reps):
    """ms per call of each fn, the fns alternating inside every repetition."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return out


def summary(ms, n):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "calls": len(ms),
            "per_s_median": round(n / med * 1e3)}


def all_strict_ok(torch, flags, fault, what):
    torch.cuda.synchronize()
    if fault.cpu().tolist() != [0, 0]:
        raise SystemExit(f"msgs_bench: {what}: device self-check words {fault.cpu().tolist()}")
    bad = int((flags & 1).eq(0).sum())
    if bad:
        raise SystemExit(f"msgs_bench: {what}: {bad} valid signatures rejected")


def transactions(torch, signer, msgs, d_pk, dev):
    """(n, L + 96) device tensor: message || pk || signature over SHA-512(message)[..32]."""
    n = msgs.shape[0]
    dig = np.stack([np.frombuffer(hashlib.sha512(msgs[i].tobytes()).digest()[:32], np.uint8) for i in range(n)])
    d_sig = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    signer.sign_device(torch.from_numpy(dig).to(dev), d_sig)
    return torch.cat([torch.from_numpy(msgs).to(dev), d_pk, d_sig], dim=1).contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=8000)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "msgs_bench.json"))
    ap.add_argument("--tx-only", action="store_true", help="the transaction leg alone; prints its times (the "
                    "HSV_TX_FUSED=0 child)")
    args = ap.parse_args()

    import torch
    from hsverify import Signer, _lib, mempool, verifier

    if _lib.device_count() <= 0:
        raise SystemExit("msgs_bench: no HIP device visible (there is no CPU form of the verifier)")
    n = args.n
    dev = torch.device("cuda:0")
    rnd = np.random.default_rng(args.seed)
    seeds = rnd.integers(0, 256, (n, 32), dtype=np.uint8)
    msgs416 = rnd.integers(0, 256, (n, 416), dtype=np.uint8)
    signer = Signer(seeds)
    d_pk = torch.from_numpy(signer.public_keys()).to(dev)
    flags = torch.zeros(n, dtype=torch.uint8, device=dev)
    fault = torch.zeros(2, dtype=torch.int32, device=dev)

    d_tx = transactions(torch, signer, msgs416, d_pk, dev)
    tx = lambda: mempool.verify_transactions_device(d_tx, None, tx_size=512, n=n, flags=flags)
    mempool.verify_transactions_device(d_tx, None, tx_size=512, n=n, flags=flags, fault=fault)
    all_strict_ok(torch, flags, fault, "transactions")
    if args.tx_only:
        (ms,) = timed(torch, [tx], args.warmup, args.reps)
        print(json.dumps(ms))
        return

    def msgs_call(d_sig, d_msgs, **kw):
        return lambda: verifier.verify_msgs_device(d_pk, d_sig, d_msgs, flags=flags, **kw)

    rec = {"what": "tools/msgs_bench.py: hsv_verify_msgs_device against hsv_verify_device and the mempool path",
           "library": _lib.version(), "device": torch.cuda.get_device_name(0), "n": n, "reps": args.reps,
           "checked": "every signature valid; every call's flags all STRICT_OK and fault words zero before timing"}

    # ---- msg_len 32 against hsv_verify_device ------------------------------
    d_m32 = torch.from_numpy(rnd.integers(0, 256, (n, 32), dtype=np.uint8)).to(dev)
    d_s32 = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    signer.sign_device(d_m32, d_s32)
    ref = torch.zeros(n, dtype=torch.uint8, device=dev)
    verifier.verify_device(d_pk, d_s32, d_m32, flags=ref, fault=fault)
    all_strict_ok(torch, ref, fault, "hsv_verify_device")
    verifier.verify_msgs_device(d_pk, d_s32, d_m32.view(-1), msg_len=32, flags=flags, fault=fault)
    all_strict_ok(torch, flags, fault, "msg_len 32")
    a, b = timed(torch, [lambda: verifier.verify_device(d_pk, d_s32, d_m32, flags=ref),
                         msgs_call(d_s32, d_m32.view(-1), msg_len=32)], args.warmup, args.reps)
    rec["len32"] = {"hsv_verify_device": summary(a, n), "hsv_verify_msgs_device": summary(b, n)}

    # ---- msg_len 416 against 512-byte transactions ---------------------------
    d_m416 = torch.from_numpy(msgs416).to(dev)
    d_s416 = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    signer.sign_device(d_m416, d_s416)
    verifier.verify_msgs_device(d_pk, d_s416, d_m416.view(-1), msg_len=416, flags=flags, fault=fault)
    all_strict_ok(torch, flags, fault, "msg_len 416")
    a, b = timed(torch, [tx, msgs_call(d_s416, d_m416.view(-1), msg_len=416)], args.warmup, args.reps)
    rec["len416"] = {"hsv_verify_transactions_device_fused": summary(a, n), "hsv_verify_msgs_device": summary(b, n)}
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--tx-only", "--n", str(n), "--reps",
                            str(args.reps), "--warmup", str(args.warmup), "--seed", str(args.seed)],
                           env=dict(os.environ, HSV_TX_FUSED="0"), capture_output=True, text=True, timeout=900)
    if child.returncode != 0:
        raise SystemExit("msgs_bench: HSV_TX_FUSED=0 child failed:\n" + child.stderr[-2000:])
    rec["len416"]["hsv_verify_transactions_device_two_launch"] = summary(json.loads(child.stdout.strip().split("\n")[-1]), n)
    del d_m416, d_tx

    # ---- ragged: lengths uniform in 0..1024, random order ---------------------
    # item j is signed by key perm[j]: one sign_msgs_device call over the packed buffer
    lens = np.sort(rnd.integers(0, 1025, n))
    perm = torch.from_numpy(rnd.permutation(n)).to(dev)
    d_lens = torch.from_numpy(lens).to(dev)[perm]
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_off[1:] = torch.cumsum(d_lens, 0)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    d_buf = torch.randint(0, 256, (int(d_off[-1]),), dtype=torch.uint8, device=dev, generator=gen)
    d_sr = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    signer.sign_msgs_device(d_buf, d_sr, offsets=d_off, key_idx=perm.to(torch.int32), fault=fault)
    torch.cuda.synchronize()
    if fault.cpu().tolist() != [0, 0]:
        raise SystemExit(f"msgs_bench: signing the ragged batch: device self-check words {fault.cpu().tolist()}")
    d_pkr = d_pk[perm].contiguous()
    ragged = lambda: verifier.verify_msgs_device(d_pkr, d_sr, d_buf, d_off, flags=flags)
    verifier.verify_msgs_device(d_pkr, d_sr, d_buf, d_off, flags=flags, fault=fault)
    all_strict_ok(torch, flags, fault, "ragged")
    (a,) = timed(torch, [ragged], args.warmup, args.reps)
    rec["ragged_0_1024"] = {"message_bytes": int(d_buf.numel()), "hsv_verify_msgs_device": summary(a, n)}
    signer.close()

    med = lambda leg, key: rec[leg][key]["ms_median"]
    rec["ratios"] = {
        "len32_msgs_over_verify_device": round(med("len32", "hsv_verify_msgs_device") / med("len32", "hsv_verify_device"), 4),
        "len416_msgs_over_tx_fused": round(med("len416", "hsv_verify_msgs_device") /
                                           med("len416", "hsv_verify_transactions_device_fused"), 4),
        "len416_msgs_over_tx_two_launch": round(med("len416", "hsv_verify_msgs_device") /
                                                med("len416", "hsv_verify_transactions_device_two_launch"), 4),
        "ragged_over_len32_verify_device": round(med("ragged_0_1024", "hsv_verify_msgs_device") /
                                                 med("len32", "hsv_verify_device"), 4),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["ratios"] | {"out": args.out}))


if __name__ == "__main__":
    main()
