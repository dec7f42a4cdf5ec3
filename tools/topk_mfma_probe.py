#!/usr/bin/env python3
"""What the matrix-core Hamming top-k costs for k = 4 and k = 8 against the vector-ALU kernel, on the bench's match shape (35 312 queries x
983 616 rows, descriptors from synth): apds_dev_hamming_topk_backend with backend 1 (xor + popcount) and backend 3 (hamming_mfma_topk_kernel),
and k = 2 on backend 2 for scale. All variants alternate in one process, `--rounds` times over; per round and variant one warm-up call, then
HIP-event time of the whole call (expansion, threshold launch, main launch, merge) for `--reps` calls, median. The keys of the two backends
are compared on that very run.

    python tools/topk_mfma_probe.py [--rounds 2] [--reps 5] [--out profiles/topk_mfma/topk_mfma_probe.json]

The last line is a JSON summary; `kmax` is what the figures say APDS_MATCH_MFMA_KMAX should default to: 8 if backend 3 beats backend 1 at both
k by more than the spread between the rounds' medians, 4 if at k = 4 only, else 2."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", type=int, default=35312)
    ap.add_argument("--rows", type=int, default=983616)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import __graft_entry__ as graft
    pkg = graft.load_package()
    L, check, synth = pkg.lib(), pkg._lib.check, pkg.synth
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    check(L.apds_set_device(0))
    nq, nt = args.queries, args.rows

    db_np = synth.make_descriptor_db(nt)
    q_np, _ = synth.make_queries(db_np, nq)
    pad = lambda a: torch.from_numpy(np.concatenate([a, np.zeros((len(a), 3), np.uint8)], 1)).to(dev)   # noqa: E731
    db, q = pad(db_np), pad(q_np)
    stream = torch.cuda.Stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    variants = [(1, 4), (3, 4), (1, 8), (3, 8), (2, 2)]          # (backend, k)
    outs = {v: torch.empty((nq, v[1]), dtype=torch.int64, device=dev) for v in variants}
    torch.cuda.synchronize()

    def call(v):
        check(L.apds_dev_hamming_topk_backend(q.data_ptr(), nq, db.data_ptr(), nt, 0, v[1], outs[v].data_ptr(), v[0], sp))

    medians = {v: [] for v in variants}
    for r in range(args.rounds):
        for v in variants:
            call(v)                                              # warm-up
            stream.synchronize()
            ms = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                call(v)
                b.record(stream)
                b.synchronize()
                ms.append(a.elapsed_time(b))
            medians[v].append(float(np.median(ms)))
            print(f"round {r} backend {v[0]} k {v[1]}: median {medians[v][-1]:.3f} ms of {[round(x, 3) for x in ms]}", flush=True)
    torch.cuda.synchronize()
    equal = {k: bool(torch.equal(outs[(1, k)], outs[(3, k)])) for k in (4, 8)}
    equal[2] = bool(torch.equal(outs[(2, 2)], outs[(1, 4)][:, :2]))

    spread = max(max(m) - min(m) for m in medians.values())
    faster = {k: equal[k] and min(medians[(1, k)]) - max(medians[(3, k)]) > spread for k in (4, 8)}
    kmax = 8 if faster[4] and faster[8] else (4 if faster[4] else 2)
    med = lambda v: float(np.median(medians[v]))   # noqa: E731
    summary = dict(queries=nq, rows=nt, rounds=args.rounds, reps=args.reps,
                   ms={f"backend{b}_k{k}": [round(x, 3) for x in medians[(b, k)]] for b, k in variants},
                   spread_between_rounds_ms=round(spread, 3), keys_equal=equal,
                   speedup_k4=round(med((1, 4)) / med((3, 4)), 2), speedup_k8=round(med((1, 8)) / med((3, 8)), 2),
                   pairs_per_s_backend3_k4=round(nq * nt / (med((3, 4)) * 1e-3), -9), pairs_per_s_backend3_k8=round(nq * nt / (med((3, 8)) * 1e-3), -9),
                   pairs_per_s_backend2_k2=round(nq * nt / (med((2, 2)) * 1e-3), -9), kmax=kmax, device=torch.cuda.get_device_name(0))
    line = json.dumps(summary)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    if not all(equal.values()):
        raise SystemExit("keys differ between the backends")


if __name__ == "__main__":
    main()
