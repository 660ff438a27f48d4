"""Times the AFS style-extractor training step (three forwards of h, one backward: s = h(w_src),
t = h(w_tgt), n = h((w_src - s) + t), loss = l1(n, t.detach())) natively and as a torch-eager restatement
on the same GPU.

    python tools/afs_bench.py [--batches 8 64] [--iters 30]

The eager arm is self-contained: the default StyleExtractor's arithmetic written with torch.nn.functional
over the native model's own parameter values (fp32, or under torch.autocast(bfloat16) for the bf16 arm).
The two arms alternate step by step (native, eager, native, ...), each step bracketed by its own pair of
HIP events after 5 untimed steps of each; median and fastest step per arm, their ratio, and the launches
per step (native: libfervit calls counted at the ops wrappers; eager: device kernels seen by
torch.profiler, when it is available) go out as one JSON line per (batch, precision).
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fer-vit_amd"))


def eager_h(P, bufs, G, n_hw, momentum):
    """h(w) from a {state_dict key: tensor} of leaf parameters; BatchNorm in train mode."""

    def lin(x, pre):
        return F.linear(x, P[pre + ".weight"], P[pre + ".bias"])

    def h(w):
        outs = []
        for g in range(G):
            b = f"blocks.{g}."
            x = lin(w[:, g], b + "down")
            for j in range(n_hw):
                hw = f"{b}highways.{j}."
                bn = hw + "nonlinear.1."
                gate = torch.sigmoid(lin(x, hw + "gate"))
                n = F.batch_norm(lin(x, hw + "nonlinear.0"), bufs[bn + "running_mean"], bufs[bn + "running_var"],
                                 P[bn + "weight"], P[bn + "bias"], True, momentum, 1e-5)
                x = gate * F.leaky_relu(n, 0.2) + (1.0 - gate) * lin(x, hw + "linear")
            outs.append(lin(x, b + "up"))
        return torch.stack(outs, dim=1)

    return h


def step(h, params, w_src, w_tgt):
    for p in params:
        p.grad = None
    s = h(w_src)
    t = h(w_tgt)
    n = h((w_src - s) + t)
    loss = (n - t.detach()).abs().mean()
    loss.backward()
    return loss


def timed_pair(a, b, iters):
    for _ in range(5):
        a()
        b()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(iters):
        for k, fn in enumerate((a, b)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return [(statistics.median(m), min(m)) for m in ms]


def native_launches(fn):
    from fervit import ops

    count, real = [0], ops.check

    def counting(rc, what=""):
        count[0] += 1
        return real(rc, what)

    ops.check = counting
    try:
        fn()
    finally:
        ops.check = real
    return count[0]


def eager_kernels(fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if getattr(e, "device_type", None) is not None
                   and "cuda" in str(e.device_type).lower())
    except Exception as exc:  # the profiler is optional: the times do not depend on it
        return f"unavailable ({type(exc).__name__})"


def main():
    from afs import StyleExtractor

    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    dev = "cuda"
    torch.manual_seed(0)
    model = StyleExtractor().to(dev).train()
    G = model.n_layers
    P = {k: v.detach().clone().requires_grad_() for k, v in model.named_parameters()}
    bufs = {k: v.detach().clone() for k, v in model.named_buffers()}
    h_eager = eager_h(P, bufs, G, 2, 0.1)
    for B in args.batches:
        w_src, w_tgt = torch.randn(B, G, 512, device=dev), torch.randn(B, G, 512, device=dev)
        for prec in ("bf16", "fp32"):
            model.set_precision(prec)

            def native():
                return step(model, model.parameters(), w_src, w_tgt)

            def eager():
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec == "bf16"):
                    return step(h_eager, P.values(), w_src, w_tgt)

            (nat, nat_min), (eag, eag_min) = timed_pair(native, eager, args.iters)
            print(json.dumps({"B": B, "precision": prec, "native_ms": round(nat, 3), "native_min_ms": round(nat_min, 3),
                              "eager_ms": round(eag, 3), "eager_min_ms": round(eag_min, 3),
                              "eager_over_native": round(eag / nat, 2), "native_launches": native_launches(native),
                              "eager_kernels": eager_kernels(eager)}), flush=True)


if __name__ == "__main__":
    main()
