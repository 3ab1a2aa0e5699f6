#!/usr/bin/env python3
"""Block::verify in one call against the three calls it replaces.

One process, the product library, host buffers, every signature valid, the
automatic committee cache warm (every key recurs, as a committee's do).  For a
block of n = 3, 67 and 667 votes (C1, C2, C3) with a QC and a TC of n votes
each, on the same bytes, legs alternating call by call:
  one      hsv_block_verify_bincode                    (1 + n + n items, one call)
  strict   hsv_verify_strict of the author's signature \
  qc       hsv_qc_verify_bincode of the embedded QC     > what a shim assembles
  tc       hsv_tc_verify_bincode of the embedded TC    /
  member   hsv_block_verify_bincode with an explicit committee (for reference)
The condition: the p50 of `one` does not exceed the sum of the p50s of
`strict`, `qc` and `tc` at any of the three sizes.  For `one` the call's host
timeline (hsv_host_call_marks: cache lookup done, slot, staged, launched,
synchronised, done; ms from the call's entry, so parse and assembly lie before
the first mark) is recorded beside it.

Chain: 256 blocks of C2 (1 + 67 + 67 items each, 34 560 items) through
hsv_blocks_verify_bincode without and with an explicit committee, and block by
block through hsv_block_verify_bincode.

Before anything is timed every leg must answer Ok.  Times are host wall clock
around the call (the calls are synchronous), in ms.

    python tools/proposal_bench.py --out profiles/proposal_bench.json
"""
import argparse
import ctypes
import hashlib
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hotstuff-digital-signature-benchmarking_amd"))

SIZES = (3, 67, 667)
CHAIN_BLOCKS, CHAIN_VOTES = 256, 67


def pct(ms, q):
    return round(float(np.percentile(np.asarray(ms), q)), 4)


def le(x):
    return struct.pack("<Q", x)


def h32(b):
    return hashlib.sha512(b).digest()[:32]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=400, help="timed calls per leg and size")
    ap.add_argument("--chain-calls", type=int, default=20, help="timed calls per chain leg")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=9200)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "proposal_bench.json"))
    args = ap.parse_args()

    from hsverify import _lib, verifier, wire
    from hsverify.committee import Committee

    lib = _lib.load()
    if _lib.device_count() <= 0:
        raise SystemExit("proposal_bench: no HIP device visible (there is no CPU form of the verifier)")
    rnd = np.random.default_rng(args.seed)
    nkeys = max(SIZES) + CHAIN_BLOCKS  # the voters, then one author per chain block
    seeds = rnd.integers(0, 256, (nkeys, 32), dtype=np.uint8)
    pk_arr, _ = verifier.sign_many(seeds, np.zeros((nkeys, 32), np.uint8))
    pks = [bytes(p) for p in pk_arr]

    def sign(idx, digests):
        msgs = np.frombuffer(b"".join(digests), np.uint8).reshape(len(idx), 32)
        return [bytes(s) for s in verifier.sign_many(seeds[np.asarray(idx)], msgs)[1]]

    def block(n, author, round_, tc=True):
        """-> (block bytes, author digest, author signature, QC bytes, TC bytes)"""
        qc_hash = bytes(rnd.integers(0, 256, 32, dtype=np.uint8))
        payload = [bytes(rnd.integers(0, 256, 32, dtype=np.uint8)) for _ in range(3)]
        sq = sign(range(n), [h32(qc_hash + le(round_ - 1))] * n)
        qc = wire.encode_qc(qc_hash, round_ - 1, [(pks[i], sq[i]) for i in range(n)])
        hqc = [round_ - 2 - i % 3 for i in range(n)]
        st = sign(range(n), [h32(le(round_ - 1) + le(r)) for r in hqc])
        tcb = wire.encode_tc(round_ - 1, [(pks[i], st[i], hqc[i]) for i in range(n)]) if tc else None
        digest = wire.block_digest(pks[author], round_, payload, qc_hash)
        sig = sign([author], [digest])[0]
        return wire.encode_block(qc, tcb, pks[author], round_, payload, sig), digest, sig, qc, tcb

    # every key in the automatic cache, and an explicit committee over the same keys
    lib.hsv_set_auto_committee(1)
    packed = b"".join(p + bytes(64) for p in pks)
    for _ in range(3):
        lib.hsv_verify_batch_packed(bytes(32), packed, nkeys)
    if lib.hsv_auto_committee_wait(120000) != 1 or lib.hsv_auto_committee_size() < nkeys:
        raise SystemExit("proposal_bench: the automatic committee cache did not learn the keys")
    committee = Committee(pk_arr)
    ch = committee._h
    res = (ctypes.c_uint32 * 2)()

    def timed(f):
        t0 = time.perf_counter()
        rc = f()
        return (time.perf_counter() - t0) * 1e3, rc

    def run(legs, calls, what):
        for k, f in legs.items():
            if f() != legs_ok[k]:
                raise SystemExit(f"proposal_bench: {what}: leg {k} did not answer Ok: {_lib.last_error()}")
        order = list(legs)
        for _ in range(args.warmup):
            for k in order:
                legs[k]()
        ms = {k: [] for k in order}
        for _ in range(calls):
            for k in order:
                t, rc = timed(legs[k])
                if rc != legs_ok[k]:
                    raise SystemExit(f"proposal_bench: {what}: leg {k} answered {rc}")
                ms[k].append(t)
        return {k: {"p50": pct(v, 50), "p99": pct(v, 99)} for k, v in ms.items()}

    import torch  # the device's name only
    rec = {"what": "tools/proposal_bench.py: one hsv_block_verify_bincode call against hsv_verify_strict + "
                   "hsv_qc_verify_bincode + hsv_tc_verify_bincode on the same bytes; one process, legs alternating "
                   "call by call, automatic committee cache warm",
           "library": _lib.version(), "device": torch.cuda.get_device_name(0), "keys": nkeys,
           "calls_per_leg": args.calls, "warmup": args.warmup,
           "timing": "host wall clock around each synchronous call, ms",
           "checked": "every leg answers Ok before and while it is timed",
           "blocks": [], "chain": None}
    legs_ok = {"one": 1, "strict": 1, "qc": 1, "tc": 1, "member": 1}
    for n in SIZES:
        buf, digest, sig, qc, tc = block(n, max(SIZES), 9)
        author = pks[max(SIZES)]
        legs = {"one": lambda: lib.hsv_block_verify_bincode(None, buf, len(buf), res, None, None, None),
                "strict": lambda: lib.hsv_verify_strict(digest, author, sig),
                "qc": lambda: lib.hsv_qc_verify_bincode(qc, len(qc), None, None),
                "tc": lambda: lib.hsv_tc_verify_bincode(tc, len(tc), None, None),
                "member": lambda: lib.hsv_block_verify_bincode(ch, buf, len(buf), res, None, None, None)}
        p = {"votes": n, "items": 1 + 2 * n, "bytes": len(buf)}
        p.update(run(legs, args.calls, f"block of {n} votes"))
        p["three_calls_p50_sum"] = round(p["strict"]["p50"] + p["qc"]["p50"] + p["tc"]["p50"], 4)
        p["one_over_three"] = round(p["one"]["p50"] / p["three_calls_p50_sum"], 4)
        p["one_not_above_three"] = p["one"]["p50"] <= p["three_calls_p50_sum"]
        # where one call's time goes: the host timeline of a `one` call from its entry (parse, digests and
        # assembly come before the cache lookup), median over 50 calls
        marks = []
        for _ in range(50):
            legs["one"]()
            buf6 = (ctypes.c_double * 6)()
            lib.hsv_host_call_marks(buf6, 6)
            marks.append(list(buf6))
        p["one_marks_ms"] = dict(zip(("lookup", "slot", "staged", "launch", "sync", "done"),
                                     [round(float(x), 4) for x in np.median(np.asarray(marks), axis=0)]))
        rec["blocks"].append(p)
        print(json.dumps(p), flush=True)
    rec["condition_one_not_above_three_everywhere"] = all(p["one_not_above_three"] for p in rec["blocks"])

    # a chain: 256 blocks of C2
    blocks = [block(CHAIN_VOTES, max(SIZES) + b, 100 + b)[0] for b in range(CHAIN_BLOCKS)]
    offsets = np.zeros(CHAIN_BLOCKS + 1, np.uint64)
    offsets[1:] = np.cumsum([len(b) for b in blocks], dtype=np.uint64)
    bufs = b"".join(blocks)
    op = ctypes.c_void_p(offsets.ctypes.data)
    results = (ctypes.c_uint32 * (2 * CHAIN_BLOCKS))()

    def each():
        return sum(lib.hsv_block_verify_bincode(None, b, len(b), res, None, None, None) for b in blocks)

    legs_ok = {"chain": CHAIN_BLOCKS, "chain_member": CHAIN_BLOCKS, "block_by_block": CHAIN_BLOCKS}
    legs = {"chain": lambda: lib.hsv_blocks_verify_bincode(None, bufs, op, CHAIN_BLOCKS, results),
            "chain_member": lambda: lib.hsv_blocks_verify_bincode(ch, bufs, op, CHAIN_BLOCKS, results),
            "block_by_block": each}
    args.warmup = min(args.warmup, 3)
    c = {"blocks": CHAIN_BLOCKS, "votes": CHAIN_VOTES, "items": CHAIN_BLOCKS * (1 + 2 * CHAIN_VOTES), "bytes": len(bufs),
         "calls_per_leg": args.chain_calls}
    c.update(run(legs, args.chain_calls, "chain"))
    for k in ("chain", "chain_member", "block_by_block"):
        c[k]["items_per_s"] = round(c["items"] / c[k]["p50"] * 1e3)
    rec["chain"] = c
    print(json.dumps(c), flush=True)
    committee.close()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "condition": rec["condition_one_not_above_three_everywhere"]}))


if __name__ == "__main__":
    main()
