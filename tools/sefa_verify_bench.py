"""Times the batched verification of non-expression directions (fervit.sefa) against the reference's procedure
driven through the same native model, interleaved on one GPU, and the bandwidth of fer_latent_shift
(DESIGN.md section 2.10).

    python tools/sefa_verify_bench.py [--rounds 5] [--samples 2000] [--out profiles/sefa_verify_bench.txt]

Model: LatentViT (depth 6, the default constructor) with seeded random weights, in the precision it is built
with; latents: a synthetic packed shard of `--samples` x 18 x 512 standard-normal latents; directions: the 10
leading SeFa directions of a seeded 512 x 512 matrix (fervit.sefa.factorize_weight). Host wall clock around
work that ends with the result on the host:
  batched 50:   verify_non_expression_directions(max_samples=50): one base forward, one latent_shift, one
                forward of the 10 x 4 x 50 rows in chunks of batch_size, one label_change per chunk, one read
  loop 50:      the reference's procedure (`sefa/verify_directions.py:38-69`): per direction and sample one
                batch-1 forward and a host read of its argmax, then per non-zero step a shifted copy, a batch-1
                forward and a host read, stopping at the first change. The reference never takes more than
                50 samples
  batched all:  verify_non_expression_directions(max_samples=None) over the whole shard. The loop is not run
                at this size (its time per sample is the 50-sample figure's; the reference cannot do it at all)
fer_latent_shift at (samples, 18, 512), HIP events around a block of calls, GB/s = bytes the call must move
(below) / time:
  choice, in place:  one read and one write of the batch (2 x n x L x D x 4 bytes)
  grid 2 x 2:        one read of the batch and four batches written (5 x n x L x D x 4 bytes)
Per case: 2 untimed runs per arm, then `rounds` alternating blocks; one JSON line per arm with the median and
the fastest block. There is no pass threshold: the lines report what was measured.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fer-vit_amd"))

STEPS = [-3.0, -1.5, 0.0, 1.5, 3.0]


def one_by_one(directions, latents, model, steps=STEPS, max_samples=50):
    """The reference's procedure on the native model: batch-1 forwards, a host read after each."""
    model.eval()
    rates = []
    with torch.no_grad():
        for d in directions:
            d = torch.as_tensor(d, dtype=torch.float32, device="cuda")
            changed = []
            for w in latents[:max_samples]:
                w = w.cuda()
                before = model(w[None]).argmax(1).item()
                hit = False
                for s in steps:
                    if s == 0.0:
                        continue
                    if model((w + s * d[None])[None]).argmax(1).item() != before:
                        hit = True
                        break
                changed.append(hit)
            rates.append(float(np.mean(changed)))
    return rates


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def event_block(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def measure(label, arms, rounds, emit, extra=None):
    for f in arms.values():
        for _ in range(2):
            f()
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            ms[k].append(wall(f))
    for k, v in ms.items():
        emit({"case": label, "arm": k, "blocks": len(v), "median_ms": round(statistics.median(v), 3),
              "min_ms": round(min(v), 3), **(extra or {})})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--batch_size", type=int, default=1024)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sefa_verify_bench: needs a ROCm device (timings on a CPU say nothing)")
    from fervit import ops
    from fervit.data import PackedLatentDataset, write_shard
    from fervit.sefa import factorize_weight, verify_non_expression_directions
    from models_fer_vit.latent_vit import LatentViT

    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    model = LatentViT(dropout=0.0).cuda()
    n, L, D, K = args.samples, 18, 512, 10
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.fwps")
        write_shard(path, rng.standard_normal((n, L, D), dtype=np.float32), rng.integers(0, 7, n))
        ds = PackedLatentDataset(path)
        latents = torch.empty(n, L, D)
        ds.gather(np.arange(n), latents)
        ds.close()
    dirs = factorize_weight(rng.standard_normal((D, D)), num_semantics=K)["directions"]
    # unit eigenvectors barely move a standard-normal latent: scale them so that some labels do change and
    # the loop's early exit is exercised as it would be on real directions
    dirs = dirs * 8.0

    def batched(max_samples):
        return [r["label_change_rate"] for r in verify_non_expression_directions(
            dirs, latents, model, None, STEPS, max_samples=max_samples, batch_size=args.batch_size, verbose=False)]

    a, b = batched(50), one_by_one(dirs, latents, model)
    emit({"case": "agreement at 50 samples", "batched_rates": a, "loop_rates": b,
          "max_abs_rate_difference": max(abs(x - y) for x, y in zip(a, b)),
          "note": "batch-1 and batched forwards may pick different GEMM tiles: a near-tie can flip"})
    measure(f"verify K={K}, 50 samples, ms per run (host wall clock)",
            {"batched": lambda: batched(50), "loop": lambda: one_by_one(dirs, latents, model)}, args.rounds, emit,
            {"precision": str(model.compute_dtype()), "batch_size": args.batch_size})
    measure(f"verify K={K}, all {n} samples, ms per run (host wall clock)", {"batched": lambda: batched(None)},
            args.rounds, emit, {"precision": str(model.compute_dtype()), "batch_size": args.batch_size})

    x = latents.cuda()
    d2 = torch.as_tensor(dirs[:2]).cuda().contiguous()
    s2 = torch.tensor([-1.0, 1.0], device="cuda")
    choice = ops.latent_dir_draw(n, 4, 0.2, 1)
    grid_out = torch.empty(4 * n, L, D, device="cuda")
    nbytes = n * L * D * 4
    for label, fn, moved in (("choice, in place", lambda: ops.latent_shift(x, d2, s2, choice=choice, out=x), 2 * nbytes),
                             ("grid 2 x 2", lambda: ops.latent_shift(x, d2, s2, out=grid_out), 5 * nbytes)):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ms = [event_block(fn, 50) for _ in range(args.rounds)]
        med = statistics.median(ms)
        emit({"case": f"latent_shift ({n}, {L}, {D}) {label} (HIP events)", "reps_per_block": 50, "blocks": len(ms),
              "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "bytes": moved,
              "median_GBps": round(moved / med / 1e6, 1), "max_GBps": round(moved / min(ms) / 1e6, 1)})


if __name__ == "__main__":
    main()
