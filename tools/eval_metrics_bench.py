"""Times the device evaluation metrics against what the trainers and the reference's evaluation script do
today, interleaved on one GPU.

    python tools/eval_metrics_bench.py [--rounds 7] [--out profiles/eval_metrics_bench.txt]

epoch metrics, 100 batches of 256 x 7 logits already on the device (host wall clock around work that ends
with the result on the host):
  meter:  ClassificationMeter.update per batch (one fer_cls_stats launch) + compute() (one fer_cls_report
          launch, one transfer)
  host:   train.common.EpochStats' path: argmax per batch, cat, two transfers, sklearn accuracy_score and
          f1_score (macro, weighted) on the host
token similarity at (1, 19, 512) and (1, 197, 768), bf16 and fp32 tokens already on the device (HIP events
around a block of calls):
  native: fervit.ops.token_cosine (one fer_token_cosine launch, both outputs)
  torch:  the reference's two torch.cosine_similarity calls (`eval/evaluate_model.py:262-280`)
Per case: 3 untimed runs per arm, then `rounds` alternating blocks; one JSON line per arm with the median
and the fastest block. No ratio is a goal here: the lines report what was measured, also where torch is
faster.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fer-vit_amd"))


def epoch_arms(batches=100, B=256, C=7):
    from sklearn.metrics import accuracy_score, f1_score

    from fervit.metrics import ClassificationMeter

    g = torch.Generator(device="cuda").manual_seed(0)
    data = [(torch.randn(B, C, device="cuda", generator=g), torch.randint(0, C, (B,), device="cuda", generator=g))
            for _ in range(batches)]
    meter = ClassificationMeter(C, "cuda")

    def native():
        meter.reset()
        for z, y in data:
            meter.update(z, y)
        r = meter.compute()
        return r["accuracy"], r["f1_macro"], r["f1_weighted"]

    def host():
        preds, labels = [], []
        for z, y in data:
            preds.append(z.argmax(dim=1))
            labels.append(y)
        p, l = torch.cat(preds).cpu().numpy(), torch.cat(labels).cpu().numpy()
        return accuracy_score(l, p), f1_score(l, p, average="macro"), f1_score(l, p, average="weighted")

    a, b = native(), host()
    assert np.allclose(a, b, rtol=0, atol=1e-12), (a, b)
    return {"meter": native, "host": host}


def wall_block(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps


def event_block(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def cosine_arms(B, N, D, dtype):
    from fervit import ops

    g = torch.Generator(device="cuda").manual_seed(N)
    x = torch.randn(B, N, D, device="cuda", generator=g).to(dtype)

    def native():
        return ops.token_cosine(x)

    def torch_():
        cls = torch.cosine_similarity(x[:, :1], x[:, 1:], dim=2)
        tok = torch.cosine_similarity(x[:, 1:].unsqueeze(2), x[:, 1:].unsqueeze(1), dim=3)
        return cls, tok

    return {"native": native, "torch": torch_}


def measure(label, arms, block, reps, rounds, emit):
    for f in arms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            ms[k].append(block(f, reps))
    for k, v in ms.items():
        emit({"case": label, "arm": k, "reps_per_block": reps, "blocks": len(v),
              "median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_metrics_bench: needs a ROCm device (timings on a CPU say nothing)")
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    measure("epoch metrics 100 x (256, 7), ms per epoch (host wall clock)", epoch_arms(), wall_block, 5, args.rounds, emit)
    for B, N, D in ((1, 19, 512), (1, 197, 768)):
        for dtype in (torch.bfloat16, torch.float32):
            name = "bf16" if dtype == torch.bfloat16 else "fp32"
            measure(f"token similarity ({B}, {N}, {D}) {name}, ms per call (HIP events)", cosine_arms(B, N, D, dtype),
                    event_block, 200, args.rounds, emit)


if __name__ == "__main__":
    main()
