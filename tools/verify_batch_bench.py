"""Batched Machine::verify on one MI355X against the host verifier, over distinct C2 proofs (fib with loop bounds FIB_N[20] - r, the
segments bench.py's segment mode proves).  Prints one JSON line:
  host_ms_per_proof_1t / _16t   vgpu_verify per C2 proof, on one host thread and on 16 (throughput: wall time / proofs)
  batch[n]                      vgpu_verify_batch of n distinct proofs: wall ms around the synchronised call (median of --reps after a
                                warm-up), per proof, and the call's own split into host stages (plans, packing, verdicts, constraints)
                                and the device stage (upload, kernels, flags back)
  speedup_vs_16t / _vs_1t       at the largest batch
    python tools/verify_batch_bench.py [--device 0] [--sizes 1,8,32] [--reps 5]"""
import argparse
import concurrent.futures
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIB_N_2_20 = 149794  # bench.py FIB_N[20]: 2^20 cpu rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sizes", default="1,8,32")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args(argv)
    sizes = [int(x) for x in args.sizes.split(",")]

    import valida_amd as va

    rc = va.poseidon_round_constants()
    machine = va.Machine.basic()
    prover = va.Prover(machine, rc, device=args.device)
    proofs, commits = [], []
    for r in range(max(sizes)):
        w = va.Workload.fib(FIB_N_2_20 - r)
        mt, prep = w.main_traces(), w.preprocessed()
        proofs.append(prover.prove([prover.upload(m) for m in mt], [(c, prover.upload(m)) for c, m in prep]).words)
        commits.append(va.host_commit_root([m for _, m in prep], rc))
    del prover

    def host_one(i):
        assert va.verify(machine, rc, proofs[i], commits[i]) is None

    host_one(0)  # warm-up
    n1 = min(8, len(proofs))
    t0 = time.perf_counter()
    for i in range(n1):
        host_one(i)
    host_1t = (time.perf_counter() - t0) * 1e3 / n1
    with concurrent.futures.ThreadPoolExecutor(16) as ex:  # ctypes releases the GIL inside vgpu_verify
        list(ex.map(host_one, range(len(proofs))))
        t0 = time.perf_counter()
        list(ex.map(host_one, range(len(proofs))))
        host_16t = (time.perf_counter() - t0) * 1e3 / len(proofs)

    v = va.Verifier(machine, rc, device=args.device)
    batch = {}
    for n in sizes:
        assert v.verify_batch(proofs[:n], commits[:n]) == [None] * n  # warm-up (and the check)
        walls, splits = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            v.verify_batch(proofs[:n], commits[:n])
            walls.append((time.perf_counter() - t0) * 1e3)
            splits.append(v.timing())
        k = walls.index(statistics.median(walls)) if args.reps % 2 else 0
        batch[str(n)] = {"wall_ms": round(statistics.median(walls), 3), "ms_per_proof": round(statistics.median(walls) / n, 4),
                         "host_ms": round(splits[k][0], 3), "device_ms": round(splits[k][1], 3), "walls_ms": [round(x, 3) for x in walls]}
    big = batch[str(max(sizes))]["ms_per_proof"]
    print(json.dumps({"metric": "verify_batch_c2", "proof_words": int(proofs[0].size), "host_ms_per_proof_1t": round(host_1t, 3),
                      "host_ms_per_proof_16t": round(host_16t, 3), "batch": batch, "speedup_vs_16t": round(host_16t / big, 2),
                      "speedup_vs_1t": round(host_1t / big, 2)}))


if __name__ == "__main__":
    main()
