#!/usr/bin/env python3
"""Single-sample inference latency: the counterpart of the reference's `scripts/measure_full_pipeline.py`
(SURVEY.md section 2.1 row 19), which compares LatentViT(depth=2) against an image ViT at batch size 1 with
20 warm-up and 100 timed forwards under no_grad. Prints one JSON line.

Models (the reference script's settings, bf16):
  latent_d2   LatentViT(depth=2, embed_dim=512, heads=8, seq_len=18)
  latent_d6   LatentViT at its default depth 6
  image_d2    ImageViT(img_size=224, patch_size=16, embed_dim=512, depth=2, heads=8, mlp_dim=2048)
--family prenorm measures the pre-norm family instead (prenorm_models below: the tiny and the config-4 base
HybridLatentViT with adapters at B = 1, 2, 3 and the tiny concat ExpressionAwareViT at B = 1), same arms.
Arms, per model and batch size (the latent models at B = 1, 2, 3 and 8, the image model at B = 1):
  eager    model.eval() forward under torch.no_grad() -- the path before InferenceSession existed
  graph    InferenceSession(skinny="off"): the same forward replayed as a HIP graph
  skinny   InferenceSession(skinny="on"), where B * tokens <= 64 (the latent models up to B = 3)
The arms are interleaved and the whole round is repeated (--repeats, default 3) in one process on one device;
each visit of an arm is --warmup forwards, then --iters forwards timed one by one with HIP events. Per arm:
mean / std / median / p10 / p90 over all timed forwards (microseconds), the median of each repeat, and
`spread`, the largest difference between two repeats' medians -- the arm's own repeat-to-repeat noise, which
a difference between two arms has to exceed to count. `launches` is the number of libfervit launch calls one
forward of the arm makes (counted on one eager pass of the same launch sequence; the input copy and the graph
launch itself are not counted; a call is one kernel except fer_gemm's split-K and column-sum forms, which
add a reduction).

Left out: the reference script's pSp encoder stage and its timm model; neither package is available here.
The tool reads nothing outside the repository.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fer-vit_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

NOT_LAUNCHES = ("_ws", "fer_last_error", "fer_version", "fer_attention_saved_floats", "fer_svm_slab",
                "fer_svm_max_groups", "fer_set_", "fer_gemm_set_config", "fer_reduce_defer", "fer_stream_")


class _Counting:
    """Proxy of the loaded library that counts the calls that enqueue kernels."""

    def __init__(self, real):
        self._real = real
        self.n = 0

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("fer_") or any(s in name for s in NOT_LAUNCHES):
            return fn

        def counted(*a):
            self.n += 1
            return fn(*a)

        return counted


def count_launches(fn):
    from fervit import _lib

    real = _lib.lib()
    proxy = _Counting(real)
    _lib._LIB = proxy
    try:
        with torch.no_grad():
            fn()
        torch.cuda.synchronize()
    finally:
        _lib._LIB = real
    return proxy.n


def time_arm(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [1e3 * a.elapsed_time(b) for a, b in ev]


def prenorm_models():
    """The pre-norm family (--family prenorm), 12 blocks each, w+ 18 x 512 inputs:
      hybrid_tiny   HybridLatentViT, timm tiny geometry (D 192), adapters of width 64, B = 1, 2, 3
      hybrid_base   BASELINE config 4: base geometry (D 768), adapters of width 64, B = 1, 2, 3
      concat_tiny   ExpressionAwareViT(output_mode="concat") on the tiny hybrid: 37 token rows, B = 1
    The adapters' alpha is set to 0.37 and their weights to N(0, 0.05^2) so that no launch works on zeros; the
    decomposer's directions are seeded random unit vectors."""
    from models_fer_vit.expression_aware_vit import ExpressionAwareViT
    from models_fer_vit.hybrid_latent_vit import create_hybrid_latent_vit
    from models_fer_vit.latent_decomposer import LatentDecomposer

    def hybrid(size, seq_len=18):
        m = create_hybrid_latent_vit(latent_dim=512, seq_len=seq_len, model_size=size, use_pretrained=False,
                                     use_adapter=True, adapter_dim=64)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("alpha"):
                    p.fill_(0.37)
                elif n.startswith("adapters") and p.dim() == 2:
                    p.normal_(0.0, 0.05)
        return m

    dec = LatentDecomposer({i: torch.randn(18, 512) for i in range(7)})
    return {
        "hybrid_tiny": (hybrid("tiny"), (18, 512), 19, (1, 2, 3)),
        "hybrid_base": (hybrid("base"), (18, 512), 19, (1, 2, 3)),
        "concat_tiny": (ExpressionAwareViT(dec, hybrid("tiny", 36), output_mode="concat"), (18, 512), 37, (1,)),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--family", choices=("postnorm", "prenorm"), default="postnorm",
                    help="postnorm: the models above; prenorm: the HybridLatentViT / ExpressionAwareViT set")
    args = ap.parse_args()

    from fervit.infer import SKINNY_MAX_ROWS, InferenceSession

    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    if args.family == "postnorm":
        from models_fer_vit.image_vit import ImageViT
        from models_fer_vit.latent_vit import LatentViT

        models = {
            "latent_d2": (LatentViT(depth=2, embed_dim=512, heads=8, seq_len=18), (18, 512), 19, (1, 2, 3, 8)),
            "latent_d6": (LatentViT(), (18, 512), 19, (1, 2, 3, 8)),
            "image_d2": (ImageViT(img_size=224, patch_size=16, embed_dim=512, depth=2, heads=8, mlp_dim=2048),
                         (3, 224, 224), 197, (1,)),
        }
    else:
        models = prenorm_models()
    arms = {}  # name -> (callable, launches)
    keep = []
    for name, (m, shape, tokens, batches) in models.items():
        m = m.to(dev).eval()
        for B in batches:
            x = torch.randn(B, *shape, device=dev)

            def eager(m=m, x=x):
                with torch.no_grad():
                    return m(x)

            arms[f"{name}/B{B}/eager"] = (eager, count_launches(eager))
            plans = ["off"] + (["on"] if B * tokens <= SKINNY_MAX_ROWS else [])
            for plan in plans:
                s = InferenceSession(m, batch_size=B, skinny=plan)
                keep.append(s)
                arms[f"{name}/B{B}/{'skinny' if plan == 'on' else 'graph'}"] = (
                    (lambda s=s, x=x: s.run(x)), count_launches(s._forward))
    samples = {k: [] for k in arms}
    for _ in range(args.repeats):
        for k, (fn, _) in arms.items():
            samples[k].append(time_arm(fn, args.warmup, args.iters))
    res = {}
    for k, reps in samples.items():
        allv = np.array([v for r in reps for v in r])
        meds = [float(np.median(r)) for r in reps]
        res[k] = dict(mean=round(float(allv.mean()), 2), std=round(float(allv.std()), 2),
                      median=round(float(np.median(allv)), 2), p10=round(float(np.percentile(allv, 10)), 2),
                      p90=round(float(np.percentile(allv, 90)), 2), repeat_medians=[round(v, 2) for v in meds],
                      spread=round(max(meds) - min(meds), 2), launches=arms[k][1])
    line = json.dumps(dict(tool="infer_latency_bench", family=args.family, unit="us",
                           device=torch.cuda.get_device_name(0),
                           precision="bf16", warmup=args.warmup, iters=args.iters, repeats=args.repeats, arms=res))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for s in keep:
        s.close()


if __name__ == "__main__":
    main()
