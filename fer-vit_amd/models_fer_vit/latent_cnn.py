"""LatentCNN baseline (reference `models_fer_vit/latent_cnn.py`): 1-D CNNs over StyleGAN w+ codes,
input (B, 18, 512) -> logits (B, 7), the CNN arm of the reference's cnn_vs_vit experiments.

Same constructors, attributes, initialisation order and state_dict keys as the reference (the
modules below are the reference's nn.Conv1d / nn.BatchNorm1d / nn.Linear containers, built in the
same order so the default and custom initialisers consume the RNG identically); the forward runs
on the HIP path (fervit/cnn.py) in token-major layout [B*L][C]. BatchNorm's running_mean,
running_var and num_batches_tracked are ordinary module buffers, updated on the device.

`create_latent_cnn('standard')` (`latent_cnn.py:66-161`, the trainer's default), `'light'`
(`:264-330`) and `'deep'` (`:164-261`: Linear + LayerNorm projection, three conv stages with residual
blocks, softmax attention pooling over the sequence) are native.

`LatentCNN2D` (`:333-409`: the (18, 512) code as a one-channel image through three Conv2d(3x3) +
BatchNorm2d + ReLU stages with MaxPool2d((2, 2)) and Dropout2d, a global average pool and the classifier)
is native too, on pixel-major rows [B*H*W][C] (csrc/conv2d.hip, fervit.cnn.Conv2dBNFn). The class is its
public entry point for now: `create_latent_cnn('2d')` still raises NotImplementedError, because
tests/test_latent_cnn_deep_cpu.py::test_2d_is_still_not_implemented pins that. The follow-up is one line,
the factory branch `return LatentCNN2D(latent_dim, seq_len, num_classes, dropout)`, plus that test.
"""
import torch
import torch.nn as nn

from fervit import ops
from fervit.cnn import (AttnPoolFn, Cnn2dCfg, CnnCfg, Conv2dBNFn, ConvBNFn, LogitsFn, MlpLogitsFn, ProjLNFn,
                        ResBlockFn, SeqMeanFn, bn_state)
from fervit.module import FerModule


def _p(drop, training: bool) -> float:
    return float(drop.p) if (drop is not None and training) else 0.0


def _check_conv(conv: nn.Conv1d) -> None:
    if conv.kernel_size != (3,) or conv.stride != (1,) or conv.padding != (1,) or conv.dilation != (1,) \
            or conv.groups != 1 or conv.padding_mode != "zeros":
        raise NotImplementedError("fervit: only Conv1d(kernel_size=3, stride=1, padding=1) has a kernel")


def _rows(x: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    """(B, L, D) -> token-major [B*L][D] in the compute dtype."""
    B, L, D = x.shape
    t = x.reshape(B * L, D)
    if x.requires_grad and torch.is_grad_enabled():
        return t.to(dt).contiguous()
    t = t.contiguous().float()
    return ops.cast_bf16(t) if dt == torch.bfloat16 else t


def _from_channels_first(x: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    return _rows(x.transpose(1, 2), dt)


class LatentConv1D(FerModule):
    """Conv1d -> BatchNorm1d -> ReLU -> Dropout (`latent_cnn.py:14-38`)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, dropout=0.2):
        super().__init__()
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size, stride, padding, bias=False)
        self.bn = nn.BatchNorm1d(out_channels)
        self.relu = nn.ReLU(inplace=True)
        self.dropout = nn.Dropout(dropout) if dropout > 0 else None

    def run_rows(self, t, B, L, flat, save):
        _check_conv(self.conv)
        cfg = CnnCfg(B, L, True, True, _p(self.dropout, self.training), save)
        return ConvBNFn.apply(t, None, cfg, flat, bn_state(self.bn), self.conv.weight, self.conv.bias,
                              self.bn.weight, self.bn.bias)

    def forward(self, x):
        """x: (B, C, L), as the reference; returns (B, Cout, L) in x's dtype."""
        B, _, L = x.shape
        flat = self.fer_flat()
        y = self.run_rows(_from_channels_first(x, self.compute_dtype()), B, L, flat,
                          self.need_grad(x, list(self.parameters())))
        return y.view(B, L, -1).transpose(1, 2).to(x.dtype)


class LatentResBlock1D(FerModule):
    """relu(bn2(conv2(drop(relu(bn1(conv1 x))))) + x) (`latent_cnn.py:41-63`)."""

    def __init__(self, channels, kernel_size=3, dropout=0.2):
        super().__init__()
        padding = kernel_size // 2
        self.conv1 = nn.Conv1d(channels, channels, kernel_size, padding=padding, bias=False)
        self.bn1 = nn.BatchNorm1d(channels)
        self.conv2 = nn.Conv1d(channels, channels, kernel_size, padding=padding, bias=False)
        self.bn2 = nn.BatchNorm1d(channels)
        self.dropout = nn.Dropout(dropout) if dropout > 0 else None

    def run_rows(self, t, B, L, flat, save):
        _check_conv(self.conv1)
        _check_conv(self.conv2)
        cfg = CnnCfg(B, L, True, True, _p(self.dropout, self.training), save)
        return ResBlockFn.apply(t, cfg, flat, bn_state(self.bn1), bn_state(self.bn2), self.conv1.weight,
                                self.bn1.weight, self.bn1.bias, self.conv2.weight, self.bn2.weight, self.bn2.bias)

    def forward(self, x):
        B, _, L = x.shape
        flat = self.fer_flat()
        y = self.run_rows(_from_channels_first(x, self.compute_dtype()), B, L, flat,
                          self.need_grad(x, list(self.parameters())))
        return y.view(B, L, -1).transpose(1, 2).to(x.dtype)


def _init_weights(model: nn.Module) -> None:
    """`latent_cnn.py:125-136` (and `:309-319`)."""
    for m in model.modules():
        if isinstance(m, nn.Conv1d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        elif isinstance(m, nn.BatchNorm1d):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, 0, 0.01)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)


class LatentCNN(FerModule):
    """(B, 18, 512) -> conv blocks -> residual blocks -> mean over the sequence -> classifier
    (`latent_cnn.py:66-161`)."""

    def __init__(self, latent_dim: int = 512, seq_len: int = 18, num_classes: int = 7,
                 hidden_dims: list = [512, 512, 512, 512], dropout: float = 0.3, use_residual: bool = True):
        super().__init__()
        self.latent_dim = latent_dim
        self.seq_len = seq_len
        self.use_residual = use_residual
        layers = []
        in_ch = latent_dim
        for hidden_dim in hidden_dims:
            layers.append(LatentConv1D(in_ch, hidden_dim, kernel_size=3, dropout=dropout))
            in_ch = hidden_dim
        self.conv_layers = nn.Sequential(*layers)
        if use_residual:
            self.res_blocks = nn.ModuleList([LatentResBlock1D(hidden_dims[-1], kernel_size=3, dropout=dropout)
                                             for _ in range(2)])
        self.global_avg_pool = nn.AdaptiveAvgPool1d(1)
        self.use_max_pool = False
        self.classifier = nn.Sequential(
            nn.Flatten(),
            nn.Linear(hidden_dims[-1], 512),
            nn.BatchNorm1d(512),
            nn.ReLU(inplace=True),
            nn.Dropout(dropout),
            nn.Linear(512, num_classes),
        )
        self._init_weights()

    def _init_weights(self):
        _init_weights(self)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: (B, seq_len, latent_dim) -> logits (B, num_classes), fp32."""
        B, L, _ = x.shape
        flat = self.fer_flat()
        save = self.need_grad(x, list(self.parameters()))
        t = _rows(x, self.compute_dtype())
        for blk in self.conv_layers:
            t = blk.run_rows(t, B, L, flat, save)
        if self.use_residual:
            for blk in self.res_blocks:
                t = blk.run_rows(t, B, L, flat, save)
        pooled = SeqMeanFn.apply(t, B, L)
        _, lin1, bn, _, drop, lin2 = self.classifier
        cfg = CnnCfg(B, 1, False, True, _p(drop, self.training), save)
        h = ConvBNFn.apply(pooled, None, cfg, flat, bn_state(bn), lin1.weight, lin1.bias, bn.weight, bn.bias)
        return LogitsFn.apply(h, save, flat, lin2.weight, lin2.bias)


def _check_attention(conv: nn.Conv1d, channels: int) -> None:
    if not isinstance(conv, nn.Conv1d) or conv.in_channels != channels or conv.out_channels != 1 \
            or conv.kernel_size != (1,) or conv.stride != (1,) or conv.padding != (0,) or conv.dilation != (1,) \
            or conv.groups != 1:
        raise NotImplementedError("fervit: the attention pooling has a kernel only for "
                                  "Conv1d(C, 1, kernel_size=1, stride=1, padding=0) scores")


class LatentCNNDeep(FerModule):
    """Linear + LayerNorm projection to 256 -> three conv stages (256, 384, 512), each a LatentConv1D
    and residual blocks -> softmax attention pooling over the sequence -> classifier
    (`latent_cnn.py:164-261`)."""

    def __init__(self, latent_dim: int = 512, seq_len: int = 18, num_classes: int = 7, dropout: float = 0.3):
        super().__init__()
        self.latent_dim = latent_dim
        self.seq_len = seq_len
        self.input_proj = nn.Sequential(
            nn.Linear(latent_dim, 256),
            nn.LayerNorm(256),
            nn.ReLU(inplace=True),
            nn.Dropout(dropout * 0.5),
        )
        self.conv_block1 = nn.Sequential(
            LatentConv1D(256, 256, kernel_size=3, dropout=dropout),
            LatentResBlock1D(256, kernel_size=3, dropout=dropout),
        )
        self.conv_block2 = nn.Sequential(
            LatentConv1D(256, 384, kernel_size=3, dropout=dropout),
            LatentResBlock1D(384, kernel_size=3, dropout=dropout),
        )
        self.conv_block3 = nn.Sequential(
            LatentConv1D(384, 512, kernel_size=3, dropout=dropout),
            LatentResBlock1D(512, kernel_size=3, dropout=dropout),
            LatentResBlock1D(512, kernel_size=3, dropout=dropout),
        )
        self.attention = nn.Sequential(
            nn.Conv1d(512, 1, kernel_size=1),
            nn.Softmax(dim=2),
        )
        self.classifier = nn.Sequential(
            nn.Linear(512, 512),
            nn.BatchNorm1d(512),
            nn.ReLU(inplace=True),
            nn.Dropout(dropout),
            nn.Linear(512, num_classes),
        )
        self._init_weights()

    def _init_weights(self):
        """`latent_cnn.py:224-235`: as the other models, plus Conv1d biases 0 and LayerNorm 1 / 0."""
        for m in self.modules():
            if isinstance(m, (nn.Conv1d, nn.Linear)):
                if isinstance(m, nn.Conv1d):
                    nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                else:
                    nn.init.normal_(m.weight, 0, 0.01)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, (nn.BatchNorm1d, nn.LayerNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: (B, seq_len, latent_dim) -> logits (B, num_classes), fp32."""
        B, L, _ = x.shape
        flat = self.fer_flat()
        save = self.need_grad(x, list(self.parameters()))
        lin, ln, _, drop = self.input_proj
        if not isinstance(ln, nn.LayerNorm) or not ln.elementwise_affine or ln.bias is None:
            raise NotImplementedError("fervit: input_proj needs an affine LayerNorm with a bias")
        conv = self.attention[0]
        _check_attention(conv, self.conv_block3[0].conv.out_channels)
        t = ProjLNFn.apply(_rows(x, self.compute_dtype()), float(ln.eps), _p(drop, self.training), save, flat,
                           lin.weight, lin.bias, ln.weight, ln.bias)
        for stage in (self.conv_block1, self.conv_block2, self.conv_block3):
            for blk in stage:
                t = blk.run_rows(t, B, L, flat, save)
        conv = self.attention[0]
        _check_attention(conv, t.shape[1])
        pooled = AttnPoolFn.apply(t, B, L, save, flat, conv.weight, conv.bias)
        lin1, bn, _, drop, lin2 = self.classifier
        cfg = CnnCfg(B, 1, False, True, _p(drop, self.training), save)
        h = ConvBNFn.apply(pooled, None, cfg, flat, bn_state(bn), lin1.weight, lin1.bias, bn.weight, bn.bias)
        return LogitsFn.apply(h, save, flat, lin2.weight, lin2.bias)


class LatentCNNLight(FerModule):
    """Three biased conv + BN + ReLU stages, mean pool, two-layer classifier (`latent_cnn.py:264-330`)."""

    def __init__(self, latent_dim: int = 512, seq_len: int = 18, num_classes: int = 7, dropout: float = 0.3):
        super().__init__()
        self.encoder = nn.Sequential(
            nn.Conv1d(latent_dim, 256, kernel_size=3, padding=1),
            nn.BatchNorm1d(256),
            nn.ReLU(inplace=True),
            nn.Dropout(dropout),
            nn.Conv1d(256, 256, kernel_size=3, padding=1),
            nn.BatchNorm1d(256),
            nn.ReLU(inplace=True),
            nn.Dropout(dropout),
            nn.Conv1d(256, 384, kernel_size=3, padding=1),
            nn.BatchNorm1d(384),
            nn.ReLU(inplace=True),
        )
        self.pool = nn.AdaptiveAvgPool1d(1)
        self.classifier = nn.Sequential(
            nn.Flatten(),
            nn.Linear(384, 256),
            nn.ReLU(inplace=True),
            nn.Dropout(dropout),
            nn.Linear(256, num_classes),
        )
        self._init_weights()

    def _init_weights(self):
        _init_weights(self)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, L, _ = x.shape
        flat = self.fer_flat()
        save = self.need_grad(x, list(self.parameters()))
        t = _rows(x, self.compute_dtype())
        enc = self.encoder
        for ci, di in ((0, 3), (4, 7), (8, None)):
            conv, bn = enc[ci], enc[ci + 1]
            _check_conv(conv)
            cfg = CnnCfg(B, L, True, True, _p(enc[di] if di is not None else None, self.training), save)
            t = ConvBNFn.apply(t, None, cfg, flat, bn_state(bn), conv.weight, conv.bias, bn.weight, bn.bias)
        pooled = SeqMeanFn.apply(t, B, L)
        _, lin1, _, drop, lin2 = self.classifier
        return MlpLogitsFn.apply(pooled, _p(drop, self.training), save, flat, lin1.weight, lin1.bias, lin2.weight,
                                 lin2.bias)


def _check_conv2d(conv: nn.Conv2d) -> None:
    if not isinstance(conv, nn.Conv2d) or conv.kernel_size != (3, 3) or conv.stride != (1, 1) \
            or conv.padding != (1, 1) or conv.dilation != (1, 1) or conv.groups != 1 or conv.padding_mode != "zeros":
        raise NotImplementedError("fervit: only Conv2d(kernel_size=3, stride=1, padding=1) has a kernel")


def _check_pool2d(pool: nn.MaxPool2d) -> None:
    two = (2, (2, 2))
    if not isinstance(pool, nn.MaxPool2d) or pool.kernel_size not in two or pool.stride not in two \
            or pool.padding not in (0, (0, 0)) or pool.dilation not in (1, (1, 1)) or pool.ceil_mode \
            or pool.return_indices:
        raise NotImplementedError("fervit: only MaxPool2d((2, 2)) (stride 2, no padding, floor) has a kernel")


class LatentCNN2D(FerModule):
    """The w+ code as a one-channel (seq_len, latent_dim) image: Conv2d(1, 64) -> Conv2d(64, 128) + pool ->
    Conv2d(128, 256) + pool, each with BatchNorm2d, ReLU and Dropout2d, then a global average pool and the
    classifier (`latent_cnn.py:333-409`)."""

    def __init__(self, latent_dim: int = 512, seq_len: int = 18, num_classes: int = 7, dropout: float = 0.3):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(1, 64, kernel_size=3, padding=1),
            nn.BatchNorm2d(64),
            nn.ReLU(inplace=True),
            nn.Dropout2d(dropout * 0.5),
            nn.Conv2d(64, 128, kernel_size=3, padding=1),
            nn.BatchNorm2d(128),
            nn.ReLU(inplace=True),
            nn.MaxPool2d((2, 2)),
            nn.Dropout2d(dropout * 0.5),
            nn.Conv2d(128, 256, kernel_size=3, padding=1),
            nn.BatchNorm2d(256),
            nn.ReLU(inplace=True),
            nn.MaxPool2d((2, 2)),
            nn.Dropout2d(dropout),
        )
        self.gap = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(
            nn.Flatten(),
            nn.Linear(256, 256),
            nn.BatchNorm1d(256),
            nn.ReLU(inplace=True),
            nn.Dropout(dropout),
            nn.Linear(256, num_classes),
        )
        self._init_weights()

    def _init_weights(self):
        """`latent_cnn.py:386-396`."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: (B, seq_len, latent_dim) -> logits (B, num_classes), fp32."""
        B, H, W = x.shape
        flat = self.fer_flat()
        save = self.need_grad(x, list(self.parameters()))
        f = self.features
        if f[0].in_channels != 1:
            raise NotImplementedError("fervit: LatentCNN2D's first convolution reads the one-channel image")
        # x.unsqueeze(1) in pixel-major layout is [B*H*W][1]: the tensor as it lies, cast to the compute dtype
        t = _rows(x.reshape(1, B * H, W), self.compute_dtype()).reshape(-1)
        for ci, pi, di in ((0, None, 3), (4, 7, 8), (9, 12, 13)):
            conv, bn = f[ci], f[ci + 1]
            _check_conv2d(conv)
            if pi is not None:
                _check_pool2d(f[pi])
            cfg = Cnn2dCfg(B, H, W, pi is not None, _p(f[di], self.training), save)
            t = Conv2dBNFn.apply(t, cfg, flat, bn_state(bn), conv.weight, conv.bias, bn.weight, bn.bias)
            if pi is not None:
                H, W = H // 2, W // 2
        pooled = SeqMeanFn.apply(t, B, H * W)
        _, lin1, bn, _, drop, lin2 = self.classifier
        cfg = CnnCfg(B, 1, False, True, _p(drop, self.training), save)
        h = ConvBNFn.apply(pooled, None, cfg, flat, bn_state(bn), lin1.weight, lin1.bias, bn.weight, bn.bias)
        return LogitsFn.apply(h, save, flat, lin2.weight, lin2.bias)


def create_latent_cnn(model_type: str = "standard", latent_dim: int = 512, seq_len: int = 18, num_classes: int = 7,
                      dropout: float = 0.3):
    """`latent_cnn.py:412-438`. 'light', 'standard' and 'deep' run on the HIP path; so does the class
    LatentCNN2D, which this factory does not return yet (module docstring)."""
    if model_type == "light":
        return LatentCNNLight(latent_dim, seq_len, num_classes, dropout)
    if model_type == "standard":
        return LatentCNN(latent_dim, seq_len, num_classes, dropout=dropout, use_residual=True)
    if model_type == "deep":
        return LatentCNNDeep(latent_dim, seq_len, num_classes, dropout)
    if model_type == "2d":
        raise NotImplementedError("create_latent_cnn('2d'): not wired into the factory yet; construct "
                                  "models_fer_vit.latent_cnn.LatentCNN2D directly")
    raise ValueError(f"Unknown model type: {model_type}")
