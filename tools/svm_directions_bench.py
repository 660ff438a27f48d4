"""Times the linear-SVM passes and the full direction fit at the FER2013 shape.

    python tools/svm_directions_bench.py [--rows 28709] [--features 9216] [--rounds 7] [--sklearn-seconds 600]
                                         [--out profiles/svm_directions_bench.txt]

passes: fer_svm_forward (hinge and scale epilogues) and fer_svm_xtr on synthetic latents made here (7 Gaussian
  class means, unit noise, FER2013's class shares), HIP events around blocks of calls, 3 untimed runs first, then
  `rounds` alternating blocks; median and fastest per call, and the achieved GB/s of the N F 4 bytes of X against
  the 6.29 TB/s a float4 copy reaches on this chip (the measured HBM figure; 8.0 TB/s is the datasheet's).
fit: fit_linear_svm, both methods: host wall clock, passes over X, outer iterations, convergence flags.
sklearn: LinearSVC(max_iter=10000, C=0.1, class_weight='balanced') on the same data where sklearn imports, in a
  child process that is ended after --sklearn-seconds (reported as capped then); a CPU baseline from the same
  run, single-threaded as liblinear is. No ratio is a goal here: the lines report what was measured.
"""
import argparse
import json
import multiprocessing as mp
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fer-vit_amd"))

HBM_COPY_GBS = 6290.0
FER2013_SHARES = np.array([3995, 436, 4097, 7215, 4965, 4830, 3171], dtype=np.float64)  # train split, per class


def synthetic(N, F, seed=0, spread=2.0):
    g = np.random.default_rng(seed)
    y = g.choice(7, size=N, p=FER2013_SHARES / FER2013_SHARES.sum())
    y[:7] = np.arange(7)
    means = g.standard_normal((7, F)).astype(np.float32) * np.float32(spread / np.sqrt(F))
    X = g.standard_normal((N, F), dtype=np.float32)
    X += means[y]
    return X, y.astype(np.int64)


def event_block(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def sklearn_child(X, y, method, q):
    from sklearn.svm import LinearSVC

    t = time.perf_counter()
    if method == "multiclass":
        LinearSVC(max_iter=10000, C=0.1, class_weight="balanced").fit(X, y)
    else:
        for k in range(7):
            LinearSVC(max_iter=10000, C=0.1, class_weight="balanced").fit(X, (y == k).astype(int))
    q.put(time.perf_counter() - t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=28709)
    ap.add_argument("--features", type=int, default=9216)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sklearn-seconds", type=float, default=600.0, help="0 skips the sklearn baseline")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("svm_directions_bench: needs a ROCm device (timings on a CPU say nothing)")
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    from fervit import ops
    from fervit.directions import class_weights, fit_linear_svm

    N, F = args.rows, args.features
    Xh, yh = synthetic(N, F)
    X, y = torch.from_numpy(Xh).cuda(), torch.from_numpy(yh).cuda()
    g = torch.Generator(device="cuda").manual_seed(1)
    W = torch.randn(7, F, device="cuda", generator=g) / F ** 0.5
    b = torch.zeros(7, device="cuda")
    classes = torch.arange(7, device="cuda")
    Cp, Cn = (t.float().cuda() for t in class_weights(np.bincount(yh, minlength=7), "binary", 0.1))
    R, Dw, _, _ = ops.svm_hinge(X, W, b, y, classes, Cp, Cn)
    arms = {"forward hinge": lambda: ops.svm_hinge(X, W, b, y, classes, Cp, Cn),
            "forward scale": lambda: ops.svm_scale(X, W, b, Dw),
            "xtr": lambda: ops.svm_xtr(X, R)}
    for f in arms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, f in arms.items():
            ms[k].append(event_block(f, args.reps))
    gb = N * F * 4 / 1e9
    for k, v in ms.items():
        med = statistics.median(v)
        emit({"case": f"pass over X ({N}, {F}), 7 columns", "arm": k, "reps_per_block": args.reps, "blocks": len(v),
              "median_ms": round(med, 4), "min_ms": round(min(v), 4), "x_gbytes": round(gb, 4),
              "gbytes_per_s": round(gb / (med * 1e-3), 1), "of_hbm_copy_rate": round(gb / (med * 1e-3) / HBM_COPY_GBS, 3)})

    for method in ("binary", "multiclass"):
        torch.cuda.synchronize()
        t = time.perf_counter()
        coef, intercept, info = fit_linear_svm(X, y, 7, method=method)
        torch.cuda.synchronize()
        emit({"case": f"fit ({N}, {F}), 7 classes", "arm": f"fit_linear_svm {method}", "seconds": round(time.perf_counter() - t, 3),
              "total_passes": info["total_passes"], "outer_iterations": info["outer_iterations"],
              "converged": info["converged"], "relative_gradient": [float(f"{v:.3e}") for v in info["relative_gradient"]]})

    if args.sklearn_seconds > 0:
        try:
            import sklearn  # noqa: F401
        except ImportError:
            emit({"case": f"fit ({N}, {F}), 7 classes", "arm": "sklearn LinearSVC", "skipped": "sklearn does not import"})
            return
        for method in ("multiclass", "binary"):
            q = mp.get_context("spawn").Queue()
            p = mp.get_context("spawn").Process(target=sklearn_child, args=(Xh, yh, method, q))
            t = time.perf_counter()
            p.start()
            p.join(args.sklearn_seconds)
            rec = {"case": f"fit ({N}, {F}), 7 classes", "arm": f"sklearn LinearSVC {method} (host, one thread)"}
            if p.is_alive():
                p.terminate()
                p.join()
                rec.update(capped_at_seconds=args.sklearn_seconds, finished=False)
            else:
                rec.update(seconds=round(q.get() if not q.empty() else time.perf_counter() - t, 3), finished=True)
            emit(rec)


if __name__ == "__main__":
    main()
