"""AFS style extractor h : W+ -> w_sty (reference `afs/style_extractor.py`): one independent StyleBlock
per w+ layer, Linear(512, 256) -> 2 x HighwayLayer(256) -> Linear(256, 512), input and output [B, 18, 512].

Same constructors, defaults, attributes, construction order and state_dict keys as the reference (the
modules below are the reference's nn.Linear / nn.BatchNorm1d containers, built in the same order, so the
default initialisers consume the RNG identically); the forward runs on the HIP path (fervit/afs.py):
one launch per stage over all blocks. HighwayLayer and StyleBlock called on their own run the same
kernels with one group.

BatchNorm's running_mean, running_var and num_batches_tracked are real buffers of each nn.BatchNorm1d.
In a StyleExtractor they are views of three contiguous backing tensors ([num_highway, n_layers, mid_dim]
statistics, [num_highway, n_layers] counters), so one highway launch updates all blocks' statistics;
`_apply` (`.to()`, `.cuda()`) rebinds them, and every forward checks the binding (object identity of the 108
buffers). The store is float32 and int64, the kernels' types, whatever dtype `_apply` casts the module to
(the flat parameter store is float32 in the same way).
"""
from typing import List

import torch
import torch.nn as nn

from fervit import ops
from fervit.afs import AfsCfg, HwStats, StyleBlocksFn, block_stride
from fervit.module import FerModule


def _compute_input(x: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    if x.requires_grad and torch.is_grad_enabled():
        return x.to(dt).contiguous()
    x = x.contiguous().float()
    return ops.cast_bf16(x) if dt == torch.bfloat16 else x


def _check_batch(B: int, C: int, train: bool) -> None:
    if train and B < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {torch.Size([B, C])}")


def _bn_consts(bn: nn.BatchNorm1d):
    if bn.momentum is None or not bn.affine or not bn.track_running_stats or bn.running_mean is None:
        raise NotImplementedError("fervit: the highway kernel needs BatchNorm1d(affine=True, "
                                  "track_running_stats=True) with a momentum")
    return float(bn.momentum), float(bn.eps)


class _Grouped(FerModule):
    """Shared driver: `_blocks()` lists the structurally identical blocks' parameters, `_hw_stats()` the
    highway layers' BatchNorm buffers over them."""

    def _layout(self, flat, blocks):
        """(block stride, flat parameter list) of this flat store: the module tree is walked once per store."""
        cached = getattr(self, "_afs_layout", None)
        if cached is None or cached[0] is not flat:
            bl = blocks()
            cached = (flat, block_stride(flat, bl), [p for ps in bl for p in ps], len(bl))
            object.__setattr__(self, "_afs_layout", cached)
        return cached[1:]

    def _run(self, x3, blocks, stats, n_hw, ends, act):
        """blocks: callable returning the blocks' parameter lists (called when the flat store is new)."""
        flat = self.fer_flat()
        stride, P, G = self._layout(flat, blocks)
        cfg = AfsCfg(G, n_hw, ends, act, self.training, stride, self.need_grad(x3, P))
        y = StyleBlocksFn.apply(_compute_input(x3, self.compute_dtype()), cfg, flat, stats, *P)
        return y.to(x3.dtype)


class HighwayLayer(_Grouped):
    """y = gate * act(BN(W_n x)) + (1 - gate) * W_l x, gate = sigmoid(W_g x) (`style_extractor.py:5-40`)."""

    def __init__(self, dim: int, act: str = "lrelu", momentum: float = 0.1) -> None:
        super().__init__()
        self.nonlinear = nn.Sequential(
            nn.Linear(dim, dim),
            nn.BatchNorm1d(dim, momentum=momentum),
        )
        self.linear = nn.Linear(dim, dim)
        self.gate = nn.Linear(dim, dim)
        if act == "relu":
            self.act = nn.ReLU()
        elif act == "lrelu":
            self.act = nn.LeakyReLU(negative_slope=0.2)
        else:
            raise ValueError(f"Unknown activation '{act}': choose 'relu' or 'lrelu'")
        self._act_name = act

    def _stats(self) -> HwStats:
        bn = self.nonlinear[1]
        mom, eps = _bn_consts(bn)
        C = bn.num_features
        return HwStats(bn.running_mean.view(1, C), bn.running_var.view(1, C), bn.num_batches_tracked.view(1), mom, eps)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, dim] -> [B, dim] in x's dtype."""
        B, C = x.shape
        _check_batch(B, C, self.training)
        y = self._run(x.unsqueeze(1), lambda: [list(self.parameters())], [self._stats()], 1, False, self._act_name)
        return y.squeeze(1)


class StyleBlock(_Grouped):
    """Linear(in_dim, mid_dim) -> HighwayLayer x num_highway -> Linear(mid_dim, in_dim)
    (`style_extractor.py:43-73`)."""

    def __init__(self, in_dim: int = 512, mid_dim: int = 256, num_highway: int = 2, act: str = "lrelu",
                 momentum: float = 0.1) -> None:
        super().__init__()
        self.down = nn.Linear(in_dim, mid_dim)
        self.highways = nn.ModuleList(
            [HighwayLayer(mid_dim, act=act, momentum=momentum) for _ in range(num_highway)]
        )
        self.up = nn.Linear(mid_dim, in_dim)
        self._act_name = act

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, in_dim] -> [B, in_dim] in x's dtype."""
        B = x.shape[0]
        _check_batch(B, self.down.out_features, self.training and len(self.highways) > 0)
        y = self._run(x.unsqueeze(1), lambda: [list(self.parameters())], [hw._stats() for hw in self.highways],
                      len(self.highways), True, self._act_name)
        return y.squeeze(1)


class StyleExtractor(_Grouped):
    """w [B, n_layers, latent_dim] -> w_sty [B, n_layers, latent_dim]; the identity part is w - h(w)
    (`style_extractor.py:76-116`)."""

    def __init__(self, n_layers: int = 18, latent_dim: int = 512, mid_dim: int = 256, num_highway: int = 2,
                 act: str = "lrelu", momentum: float = 0.1) -> None:
        super().__init__()
        self.n_layers = n_layers
        self.blocks = nn.ModuleList(
            [
                StyleBlock(latent_dim, mid_dim, num_highway, act, momentum)
                for _ in range(n_layers)
            ]
        )
        self._act_name = act
        self._num_highway = num_highway
        self._mid_dim = mid_dim
        object.__setattr__(self, "_afs_store", None)
        self._bind_stats()

    # ---- BatchNorm buffers: views of one backing store per kind
    def _bns(self) -> List[List[nn.BatchNorm1d]]:
        return [[blk.highways[j].nonlinear[1] for blk in self.blocks] for j in range(self._num_highway)]

    def _bind_stats(self) -> None:
        bns = self._bns()
        if not bns or not self.n_layers:
            return
        dev = bns[0][0].running_mean.device
        H, G, C = self._num_highway, self.n_layers, self._mid_dim
        rm = torch.empty(H, G, C, dtype=torch.float32, device=dev)
        rv = torch.empty(H, G, C, dtype=torch.float32, device=dev)
        nbt = torch.empty(H, G, dtype=torch.int64, device=dev)
        views = []
        with torch.no_grad():
            for j in range(H):
                for g, bn in enumerate(bns[j]):
                    views.append((bn._buffers, rm[j, g], rv[j, g], nbt[j, g]))
                    rm[j, g].copy_(bn.running_mean)
                    rv[j, g].copy_(bn.running_var)
                    nbt[j, g].copy_(bn.num_batches_tracked)
                    bn._buffers["running_mean"], bn._buffers["running_var"], bn._buffers["num_batches_tracked"] = \
                        views[-1][1:]
        object.__setattr__(self, "_afs_store", (rm, rv, nbt))
        object.__setattr__(self, "_afs_views", views)

    def _bound(self) -> bool:
        """Every BatchNorm still holds the view it was given (`.to()` on a child, or an assigned buffer,
        replaces the tensor object)."""
        if self._afs_store is None:
            return False
        return all(b["running_mean"] is m and b["running_var"] is v and b["num_batches_tracked"] is n
                   for b, m, v, n in self._afs_views)

    def _apply(self, fn, recurse=True):
        r = super()._apply(fn, recurse)
        self._bind_stats()
        return r

    def forward(self, w: torch.Tensor) -> torch.Tensor:
        B, G, D = w.shape
        if G != self.n_layers:
            raise ValueError(f"StyleExtractor: expected {self.n_layers} w+ layers, got {G}")
        if G == 0:
            return torch.stack([], dim=1)
        _check_batch(B, self._mid_dim, self.training and self._num_highway > 0)
        if not self._bound():
            self._bind_stats()
        rm, rv, nbt = self._afs_store
        stats = []
        for j in range(self._num_highway):
            mom, eps = _bn_consts(self.blocks[0].highways[j].nonlinear[1])
            stats.append(HwStats(rm[j], rv[j], nbt[j], mom, eps))
        blocks = lambda: [list(blk.parameters()) for blk in self.blocks]
        return self._run(w, blocks, stats, self._num_highway, True, self._act_name)
