#!/usr/bin/env python3
"""The staged host forms bench.py does not time, two generic calls and their
committee twins, which run one walk each:

  tx_fixed        hsv_verify_transactions_fixed
  committee_tx    hsv_committee_verify_transactions (fixed size)
  msgs            hsv_verify_msgs (fixed length)
  committee_msgs  hsv_committee_verify_msgs (fixed length)

Workload: n (default 2^20) transactions of 512 bytes and n messages of 416
bytes in host memory, signed on the GPU with K = 1000 keys drawn uniformly per
item; the committee is those K keys.  Each call is timed on the host clock
around the C ABI call (it returns with the flags in host memory); a figure is
the median of `--reps` calls after `--warmup`.  Before any timing every item
must be STRICT_OK in all four calls and each committee call's flags must equal
its generic twin's.  The library is the one HSV_LIB names (default libhsv.so),
so two builds are compared by alternating processes.  Prints one JSON line.

    python tools/host_forms_bench.py
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hotstuff-digital-signature-benchmarking_amd"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--tx-size", type=int, default=512)
    ap.add_argument("--msg-len", type=int, default=416)
    ap.add_argument("--keys", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    from hsverify import STRICT_OK, Signer, _lib
    from hsverify.committee import Committee

    if _lib.device_count() <= 0:
        raise SystemExit("host_forms_bench: no HIP device visible")
    lib = _lib.load(require=True)
    n, size, length, K = args.n, args.tx_size, args.msg_len, args.keys
    dev = torch.device("cuda:0")
    rnd = np.random.default_rng(4900)
    gen = torch.Generator(device="cpu").manual_seed(4900)
    seeds = rnd.integers(0, 256, (K, 32), dtype=np.uint8)
    key_idx = torch.randint(0, K, (n,), generator=gen, dtype=torch.int32).to(dev)
    d_txs = torch.randint(0, 256, (n, size), generator=gen, dtype=torch.uint8).to(dev)
    d_msgs = torch.randint(0, 256, (n, length), generator=gen, dtype=torch.uint8).to(dev)
    d_sig = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    with Signer(seeds) as signer:
        signer.sign_transactions_device(d_txs, key_idx=key_idx)
        signer.sign_device(d_msgs, d_sig, key_idx=key_idx, msg_len=length)
        pks = np.ascontiguousarray(signer.public_keys(), np.uint8).reshape(K, 32)
    torch.cuda.synchronize()
    txs, msgs, sig = d_txs.cpu().numpy(), d_msgs.cpu().numpy(), d_sig.cpu().numpy()
    pk = np.ascontiguousarray(pks[key_idx.cpu().numpy()])
    del d_txs, d_msgs, d_sig
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    flags = {leg: np.full(n, 0xff, np.uint8) for leg in ("tx_fixed", "committee_tx", "msgs", "committee_msgs")}
    with Committee(pks) as c:
        legs = {
            "tx_fixed": lambda: lib.hsv_verify_transactions_fixed(p(txs), size, n, p(flags["tx_fixed"])),
            "committee_tx": lambda: lib.hsv_committee_verify_transactions(c._h, p(txs), None, size, n,
                                                                          p(flags["committee_tx"])),
            "msgs": lambda: lib.hsv_verify_msgs(p(pk), p(sig), p(msgs), None, length, length, n, p(flags["msgs"])),
            "committee_msgs": lambda: lib.hsv_committee_verify_msgs(c._h, p(pk), p(sig), p(msgs), None, length, length,
                                                                    n, p(flags["committee_msgs"])),
        }
        for leg, fn in legs.items():              # correctness first
            _lib.check(fn(), leg)
            if not (flags[leg] & STRICT_OK).all():
                raise SystemExit(f"host_forms_bench: {leg}: a signed item is rejected")
        for twin, generic in (("committee_tx", "tx_fixed"), ("committee_msgs", "msgs")):
            if not (flags[twin] == flags[generic]).all():
                raise SystemExit(f"host_forms_bench: {twin} differs from {generic}")
        for _ in range(args.warmup):
            for fn in legs.values():
                fn()
        ms = {leg: [] for leg in legs}
        for _ in range(args.reps):                # legs alternating call by call
            for leg, fn in legs.items():
                t0 = time.perf_counter()
                rc = fn()
                ms[leg].append((time.perf_counter() - t0) * 1e3)
                _lib.check(rc, leg)
    out = {"tool": "host_forms_bench", "library": _lib.version(), "lib_file": os.path.basename(_lib.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "n": n, "tx_size": size, "msg_len": length, "keys": K,
           "reps": args.reps, "warmup": args.warmup,
           "ms_median": {leg: round(statistics.median(v), 3) for leg, v in ms.items()},
           "ms_min": {leg: round(min(v), 3) for leg, v in ms.items()},
           "ms_max": {leg: round(max(v), 3) for leg, v in ms.items()}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
