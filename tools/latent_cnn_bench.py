"""Times the full LatentCNN ('standard', or 'deep' / '2d' with --kind) train step of the HIP path against the identical torch.nn
model in eager ROCm torch on the same GPU, interleaved (DESIGN.md "LatentCNN step time").

    python tools/latent_cnn_bench.py [--kind standard|deep|2d] [--batches 64 256] [--dtypes bf16 fp32] [--rounds 6] [--steps 20]
    python tools/latent_cnn_bench.py --only native --batches 64 --dtypes bf16 --steps 30   # under a profiler

Step = zero_grad, forward (dropout 0.3), CrossEntropyLoss, backward, AdamW (lr 1e-4, wd 1e-2), the
trainer's defaults, on a fixed synthetic batch (B, 18, 512).
  native: models_fer_vit.latent_cnn + fervit.loss.CrossEntropyLoss + FusedAdamW, set_precision(dtype)
  torch:  the same layers from torch.nn primitives (built here), nn.CrossEntropyLoss, torch.optim.AdamW;
          bf16 = torch.autocast(bfloat16) around the forward and the loss, fp32 = plain
Per (batch, dtype): 10 untimed steps per arm, then `rounds` alternating blocks (native, torch, native,
...) of `steps` steps, each block bracketed by a pair of HIP events and ended by a synchronise; one JSON
line per arm with the median and the fastest block in ms per step, and the ratio native / torch.
--only ARM runs that arm alone (warm-up + one block), for a kernel trace in a run of its own
(tools/prof_csv_summary.py reduces the trace's kernel_stats.csv).
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fer-vit_amd"))


class ConvBlock(nn.Module):
    def __init__(self, cin, cout, p):
        super().__init__()
        self.conv = nn.Conv1d(cin, cout, 3, 1, 1, bias=False)
        self.bn = nn.BatchNorm1d(cout)
        self.drop = nn.Dropout(p)

    def forward(self, x):
        return self.drop(torch.relu(self.bn(self.conv(x))))


class ResBlock(nn.Module):
    def __init__(self, c, p):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv1d(c, c, 3, padding=1, bias=False), nn.BatchNorm1d(c)
        self.conv2, self.bn2 = nn.Conv1d(c, c, 3, padding=1, bias=False), nn.BatchNorm1d(c)
        self.drop = nn.Dropout(p)

    def forward(self, x):
        out = self.drop(torch.relu(self.bn1(self.conv1(x))))
        return torch.relu(self.bn2(self.conv2(out)) + x)


class TorchLatentCNN(nn.Module):
    """Four conv blocks, two residual blocks, mean over the sequence, Linear-BN-ReLU-Dropout-Linear."""

    def __init__(self, d=512, classes=7, p=0.3):
        super().__init__()
        self.convs = nn.Sequential(*[ConvBlock(d, d, p) for _ in range(4)])
        self.res = nn.Sequential(ResBlock(d, p), ResBlock(d, p))
        self.head = nn.Sequential(nn.Linear(d, 512), nn.BatchNorm1d(512), nn.ReLU(), nn.Dropout(p),
                                  nn.Linear(512, classes))

    def forward(self, x):
        x = self.res(self.convs(x.transpose(1, 2)))
        return self.head(x.mean(2))


class TorchLatentCNNDeep(nn.Module):
    """Linear-LayerNorm-ReLU-Dropout to 256, conv + residual stages (256, 384, 512), softmax attention
    pooling over the sequence, Linear-BN-ReLU-Dropout-Linear."""

    def __init__(self, d=512, classes=7, p=0.3):
        super().__init__()
        self.proj = nn.Sequential(nn.Linear(d, 256), nn.LayerNorm(256), nn.ReLU(), nn.Dropout(p * 0.5))
        self.body = nn.Sequential(ConvBlock(256, 256, p), ResBlock(256, p), ConvBlock(256, 384, p), ResBlock(384, p),
                                  ConvBlock(384, 512, p), ResBlock(512, p), ResBlock(512, p))
        self.attention = nn.Sequential(nn.Conv1d(512, 1, kernel_size=1), nn.Softmax(dim=2))
        self.head = nn.Sequential(nn.Linear(512, 512), nn.BatchNorm1d(512), nn.ReLU(), nn.Dropout(p),
                                  nn.Linear(512, classes))

    def forward(self, x):
        x = self.body(self.proj(x).transpose(1, 2))
        return self.head(torch.sum(x * self.attention(x), dim=2))


class TorchLatentCNN2D(nn.Module):
    """The (18, 512) code as a one-channel image: three Conv2d(3x3)-BN-ReLU stages (64, 128, 256) with
    MaxPool2d((2, 2)) behind the last two and Dropout2d, global average pool, Linear-BN-ReLU-Dropout-Linear."""

    def __init__(self, classes=7, p=0.3):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(1, 64, 3, padding=1), nn.BatchNorm2d(64), nn.ReLU(), nn.Dropout2d(p * 0.5),
            nn.Conv2d(64, 128, 3, padding=1), nn.BatchNorm2d(128), nn.ReLU(), nn.MaxPool2d((2, 2)), nn.Dropout2d(p * 0.5),
            nn.Conv2d(128, 256, 3, padding=1), nn.BatchNorm2d(256), nn.ReLU(), nn.MaxPool2d((2, 2)), nn.Dropout2d(p))
        self.head = nn.Sequential(nn.Linear(256, 256), nn.BatchNorm1d(256), nn.ReLU(), nn.Dropout(p),
                                  nn.Linear(256, classes))

    def forward(self, x):
        return self.head(self.features(x.unsqueeze(1)).mean((2, 3)))


KIND = "standard"


def native_step(dtype, x, y):
    from fervit.loss import CrossEntropyLoss
    from fervit.optim import FusedAdamW
    from models_fer_vit.latent_cnn import LatentCNN2D, create_latent_cnn

    m = (LatentCNN2D() if KIND == "2d" else create_latent_cnn(KIND)).cuda()
    m.set_precision(dtype)
    m.train()
    opt = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=1e-2, model=m)
    crit = CrossEntropyLoss()

    def step():
        opt.zero_grad()
        loss = crit(m(x), y)
        loss.backward()
        opt.step()
        return loss

    return step


def torch_step(dtype, x, y):
    m = {"deep": TorchLatentCNNDeep, "2d": TorchLatentCNN2D, "standard": TorchLatentCNN}[KIND]().cuda()
    m.train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-2)
    crit = nn.CrossEntropyLoss()

    def step():
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == "bf16"):
            loss = crit(m(x), y)
        loss.backward()
        opt.step()
        return loss

    return step


def block(step, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    global KIND
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="standard", choices=["standard", "deep", "2d"])
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "fp32"], choices=["bf16", "fp32"])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", choices=["native", "torch"])
    args = ap.parse_args()
    KIND = args.kind
    if not torch.cuda.is_available():
        raise SystemExit("latent_cnn_bench: needs a ROCm device (timings on a CPU say nothing)")
    for B in args.batches:
        for dtype in args.dtypes:
            g = torch.Generator(device="cuda").manual_seed(B)
            x = torch.randn(B, 18, 512, device="cuda", generator=g)
            y = torch.randint(0, 7, (B,), device="cuda", generator=g)
            arms = {"native": native_step, "torch": torch_step}
            if args.only:
                arms = {args.only: arms[args.only]}
            steps = {k: mk(dtype, x, y) for k, mk in arms.items()}
            for s in steps.values():
                for _ in range(10):
                    loss = s()
                assert torch.isfinite(loss).item()
            torch.cuda.synchronize()
            peak = None
            if args.only:  # one arm alone in the process: its peak device memory over a step
                torch.cuda.reset_peak_memory_stats()
                steps[args.only]()
                torch.cuda.synchronize()
                peak = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
            ms = {k: [] for k in steps}
            for _ in range(1 if args.only else args.rounds):
                for k, s in steps.items():
                    ms[k].append(block(s, args.steps))
            med = {k: statistics.median(v) for k, v in ms.items()}
            for k, v in ms.items():
                rec = {"arm": k, "model": f"latent_cnn {KIND}", "B": B, "dtype": dtype, "steps_per_block": args.steps,
                       "blocks": len(v), "median_ms_per_step": round(med[k], 4), "min_ms_per_step": round(min(v), 4)}
                if peak is not None:
                    rec["peak_allocated_MiB"] = peak
                if k == "native" and "torch" in med:
                    rec["native_over_torch"] = round(med["native"] / med["torch"], 3)
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
