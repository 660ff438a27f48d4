"""Times fer_attention_probs and fer_attention_rollout_cls at the ViT-B/16 eval shape against the
torch composition on the same GPU (DESIGN.md "Attention maps").

    python tools/attn_maps_bench.py [--batch 256] [--iters 30]

Each arm: 5 untimed calls, then `iters` calls each bracketed by its own pair of HIP events on the
current stream; the median and the fastest call are printed, one JSON line per arm.
  probs: head-averaged full, head-averaged CLS row only, per-head full, vs
         softmax((q @ k^T).float() * scale, -1) [+ .mean(1) / [:, :, :1]] on the same bf16 qkv
  rollout: 12 layers, CLS row, vs twelve torch.bmm on [B, 197, 197]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fer-vit_amd"))


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    from fervit import ops

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    B, N, H, dh, L = args.batch, 197, 12, 64, 12
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = (2 * torch.randn(B * N, 3 * H * dh, device=dev, generator=g)).to(torch.bfloat16)
    x = qkv.view(B, N, 3, H, dh)
    q, k = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2)  # [B, H, N, dh] views
    scale = 1.0 / math.sqrt(dh)

    def torch_probs(qq):
        return torch.softmax((qq @ k.transpose(-1, -2)).float() * scale, dim=-1)

    avg = torch.empty(B, N, N, device=dev)
    cls = torch.empty(B, 1, N, device=dev)
    per = torch.empty(B, H, N, N, device=dev)
    arms = [
        ("probs head-avg full, fervit", lambda: ops.attention_probs(qkv, B, N, H, dh, out=avg)),
        ("probs head-avg full, torch", lambda: torch_probs(q).mean(1)),
        ("probs head-avg CLS row, fervit", lambda: ops.attention_probs(qkv, B, N, H, dh, q_count=1, out=cls)),
        ("probs head-avg CLS row, torch (full softmax, then [:, :, :1])", lambda: torch_probs(q)[:, :, :1].mean(1)),
        ("probs head-avg CLS row, torch (row-sliced q)", lambda: torch_probs(q[:, :, :1]).mean(1)),
        ("probs per-head full, fervit", lambda: ops.attention_probs(qkv, B, N, H, dh, average_heads=False, out=per)),
        ("probs per-head full, torch", lambda: torch_probs(q)),
    ]
    maps = torch.softmax(3 * torch.randn(L, B, N, N, device=dev, generator=g), dim=-1)
    r = torch.empty(B, N, device=dev)
    eye = torch.eye(N, device=dev)

    def torch_rollout():
        R = eye.expand(B, N, N)
        for l in range(L):
            R = torch.bmm(0.5 * eye + 0.5 * maps[l], R)
        return R[:, 0]

    arms += [("rollout 12 layers CLS row, fervit", lambda: ops.attention_rollout_cls(maps, 0.5, out=r)),
             ("rollout 12 layers, torch (12 x bmm)", torch_rollout)]
    for name, fn in arms:
        med, best = timed(fn, args.iters)
        print(json.dumps({"arm": name, "B": B, "median_ms": round(med, 4), "min_ms": round(best, 4)}), flush=True)


if __name__ == "__main__":
    main()
