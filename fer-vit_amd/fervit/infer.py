"""InferenceSession: a model's eval forward captured once as a HIP graph and replayed per call.

FER is a per-frame workload (one to three faces per frame); the reference measures it as single-sample latency
(`scripts/measure_full_pipeline.py`: 20 warm-up + 100 timed forwards under no_grad). Served through the
training machinery, that forward is host-bound: every layer is walked in Python, every activation is
allocated, and each launch is issued from the host. A session removes the host from the loop:

    sess = InferenceSession(model, batch_size=1)      # model.eval(), on a ROCm device, in the model's precision
    logits = sess.run(x)                              # device fp32 [B, C]; no host synchronisation
    pred, probs = sess.predict(x)                     # argmax / softmax of the same replay, on the device
    sess.refresh()                                    # after load_state_dict / optimizer steps
    sess.close()

Two forward plans:
  * graph-only: the model's own eval forward under no_grad, captured as is. Any FerModule model, batch size and
    precision; logits are bit-identical to the eager eval forward.
  * skinny: for a post-norm encoder stack (fervit.blocks.Encoder of EncoderLayers: LatentViT, LatentViTv2 with
    its w+ prologue, ImageViT) in bf16 with B * N <= 64 token rows. The session issues the launches itself: the
    model's token assembly, then five launches per layer with both LayerNorms folded into their consumers
    (csrc/skinny.hip fer_skinny_linear), z_prev being the previous layer's un-normalised output:
        1. qkv = skinny(LN2_prev-on-load(z_prev))         (first layer: the tokens, no LayerNorm)
        2. o   = fer_attention_fwd(qkv)
        3. y   = skinny(o) + LN2_prev(z_prev)
        4. g   = act(skinny(LN1-on-load(y)))
        5. z   = skinny(g) + LN1(y)
    then fer_layernorm_fwd (the last LN2) on the B CLS rows only and fer_head_fwd. Numerically it differs from
    the eager bf16 forward only in where bf16 roundings fall (the residual operand LN(.) stays fp32).
    The pre-norm family (HybridLatentViT: timm Blocks with an optional AdapterModule after each; ExpressionAwareViT:
    the model's own decomposer call and w+ prologue, then the hybrid) runs the same launches in pre-norm order,
    x being the block's input:
        1. qkv = skinny(norm1-on-load(x))
        2. o   = fer_attention_fwd(qkv)
        3. x1  = skinny(o) + x
        4. g   = gelu(skinny(norm2-on-load(x1)))
        5. x2  = skinny(g) + x1
        6. x3  = x2 + alpha * adapter(x2)                  (csrc/skinny_adapter.hip fer_skinny_adapter; alpha is
                                                            read on the device), where the model has adapters
    then fer_head_fwd on the B CLS rows (row stride N; it applies the head's LayerNorm itself).
  skinny="auto" takes the skinny plan where it applies and B * N <= SKINNY_AUTO_MAX_ROWS (post-norm models) or
  SKINNY_AUTO_MAX_ROWS_PRENORM (pre-norm family), "on" requires it (RuntimeError outside its contract), "off"
  always captures the model's own forward.

The capture is a single stream without forks (the weight-gradient stream is a backward-only device), warmed up
eagerly on that stream first so that every library workspace is sized before capture.

A session is a snapshot of the model as of its construction or its last refresh(): it captures a private deep
copy of the model (its own flat parameter store: fp32 masters, bf16 shadow), so load_state_dict or optimizer steps
on the model change nothing a run() computes until refresh() is called. refresh() copies the model's current
state_dict into the private copy in place, makes that copy's store re-check its parameters (begin_pass's job) and
re-cast its bf16 shadow, and recaptures only if an address the graph captured has moved.

run() returns the session's static output buffer: the next run() overwrites it (clone() it to keep it).
"""
from __future__ import annotations

import copy
from typing import Optional, Tuple

import torch

from . import layers, ops
from .blocks import AdapterModule, Block, Encoder, EncoderLayer
from .layers import LatentTokensFn, LayerCfg, PatchTokensFn
from .module import FerModule

SKINNY_MAX_ROWS = 64  # fer_skinny_linear's M cap

# Largest B * N at which skinny="auto" takes the skinny plan: the largest measured token-row count at which its
# median latency was below the graph-only plan's by more than that arm's repeat-to-repeat spread at BOTH depths
# (tools/infer_latency_bench.py, profiles/infer_latency_bench.json; medians in us, skinny vs graph-only):
#   19 rows (B = 1): depth 2  99.6 vs 137.2, depth 6 271.1 vs 367.0   (spreads <= 0.6)
#   38 rows (B = 2): depth 2 122.3 vs 141.2, depth 6 348.4 vs 377.6   (spreads <= 0.6)
#   57 rows (B = 3): depth 2 140.8 vs 144.2, depth 6 408.7 vs 385.0   -> loses per layer: graph-only
SKINNY_AUTO_MAX_ROWS = 38

# The same cut-off for the pre-norm family (HybridLatentViT, ExpressionAwareViT; 12 blocks, six launches per block
# with adapters), at the tiny (D 192) and the base (D 768, BASELINE config 4) size, adapters of width 64
# (tools/infer_latency_bench.py --family prenorm, profiles/infer_latency_prenorm.json; medians in us, skinny vs
# graph-only, the arms' spreads in brackets):
#   19 rows (B = 1): tiny 376.1 [0.5] vs 717.5 [8.6], base  676.0 [1.3] vs 1198.6 [80.5]
#   38 rows (B = 2): tiny 425.1 [0.2] vs 749.8 [8.3], base  870.6 [1.3] vs 1165.2 [31.5]
#   57 rows (B = 3): tiny 488.3 [0.5] vs 767.7 [7.1], base 1022.5 [1.8] vs 1208.1 [8.0]
#   37 rows (tiny concat, B = 1): 474.9 [0.5] vs 827.4 [6.7]
# The skinny plan wins at every measured row count; 57 is the largest one measured (58 - 64 rows: unmeasured,
# left graph-only).
SKINNY_AUTO_MAX_ROWS_PRENORM = 57

ADAPTER_MAX_WIDTH = 128  # fer_skinny_adapter's R cap


def _is_hybrid(m) -> bool:
    """HybridLatentViT's parts: input_proj, cls_token, pos_embed, a transformer of fervit Blocks, optional
    adapters, head = LayerNorm, Dropout, Linear."""
    tr, head = getattr(m, "transformer", None), getattr(m, "head", None)
    return (isinstance(tr, torch.nn.Sequential) and len(tr) > 0 and all(isinstance(b, Block) for b in tr)
            and all(hasattr(m, a) for a in ("input_proj", "cls_token", "pos_embed", "seq_len"))
            and isinstance(head, torch.nn.Sequential) and len(head) == 3
            and isinstance(head[0], torch.nn.LayerNorm) and isinstance(head[2], torch.nn.Linear))


class _Plan:
    """What the skinny plan needs of a model: the module whose forward assembles the tokens, the encoder,
    the head's LayerNorm and Linear, the token count and the per-sample input shape."""

    def __init__(self, model):
        self.why = None  # reason the model is outside the skinny contract
        self.spec = None
        self.decompose = None  # ExpressionAwareViT: the model's own decomposer call
        self.prenorm = False
        core = model
        if hasattr(model, "backbone") and hasattr(model, "_spec"):  # LatentViTv2
            core = model.backbone
            if model.use_spe or model.use_lwn or model.use_leam:
                self.spec = model._spec
        elif hasattr(model, "decomposer") and _is_hybrid(getattr(model, "vit", None)):  # ExpressionAwareViT
            core = model.vit
        self.core = core
        if _is_hybrid(core):
            self._prenorm(model, core)
            return
        enc = getattr(core, "transformer", None)
        if isinstance(enc, Encoder) and hasattr(core, "input_proj") and hasattr(core, "mlp_head"):
            self.kind = "latent"
            self.N = core.seq_len + 1
            self.sample_shape = (core.seq_len, core.input_proj.in_features)
            self.head_ln, self.head_lin = core.mlp_head[0], core.mlp_head[1]
        elif isinstance(enc, Encoder) and hasattr(core, "patch_embed") and hasattr(core, "head"):
            self.kind = "image"
            pe = core.patch_embed
            self.N = core.n_patches + 1
            self.sample_shape = (pe.proj.in_channels, pe.img_size, pe.img_size)
            self.head_ln, self.head_lin = core.norm, core.head
        else:
            self.kind = None
            self.why = ("the model is neither a post-norm encoder stack (fervit.blocks.Encoder of EncoderLayers) nor "
                        "a HybridLatentViT / ExpressionAwareViT")
            return
        self.enc = enc
        lay = list(enc.layers)
        if not lay or not all(isinstance(l, EncoderLayer) and not l.norm_first for l in lay):
            self.why = "the encoder's layers are not post-norm EncoderLayers"
            return
        D = lay[0].linear1.in_features
        F = lay[0].linear1.out_features
        if D % 8 or F % 8 or D > 1024:
            self.why = f"embed_dim {D} / mlp_dim {F} must be multiples of 8, embed_dim <= 1024"

    def _prenorm(self, model, core):
        """A HybridLatentViT `core`, on its own or as the `vit` of an ExpressionAwareViT `model`."""
        self.kind, self.prenorm = "hybrid", True
        self.N = core.seq_len + 1
        self.blocks = list(core.transformer)
        self.adapters = list(core.adapters) if getattr(core, "use_adapter", False) else None
        self.head_ln, self.head_lin = core.head[0], core.head[2]
        if model is core:
            self.sample_shape = (core.seq_len, core.input_proj.in_features)
        else:
            dec = model.decomposer
            self.sample_shape = (dec.seq_len, dec.latent_dim)
            self.decompose = lambda x: dec(x, output_mode=model.output_mode, enhance_alpha=model.enhance_alpha,
                                           decompose_mode=model.decompose_mode)
            if model.use_spe or model.use_lwn or model.use_leam:
                from modules._wplus import WplusSpec  # the package the model's class itself comes from

                self.spec = lambda: WplusSpec(spe=getattr(model, "spe", None), lwn=getattr(model, "lwn", None),
                                              leam=getattr(model, "leam", None))
            tokens = dec.seq_len * (2 if model.output_mode == "concat" else 1)
            if tokens != core.seq_len or dec.latent_dim != core.input_proj.in_features:
                self.why = (f"the decomposer's output ({tokens} x {dec.latent_dim}) does not match the hybrid's input "
                            f"({core.seq_len} x {core.input_proj.in_features})")
                return
        D = self.blocks[0].mlp.fc1.in_features
        F = self.blocks[0].mlp.fc1.out_features
        if D % 16 or F % 8 or D > 1024:
            self.why = f"embed_dim {D} must be a multiple of 16 and <= 1024, mlp_dim {F} a multiple of 8"
            return
        if self.adapters is not None:
            if len(self.adapters) != len(self.blocks) or not all(isinstance(a, AdapterModule) for a in self.adapters):
                self.why = "the adapters are not one AdapterModule per block"
                return
            R = self.adapters[0].adapter[0].out_features
            if R % 16 or not 16 <= R <= ADAPTER_MAX_WIDTH:
                self.why = (f"the adapter width {R} is outside fer_skinny_adapter's contract (a multiple of 16, "
                            f"16 <= width <= {ADAPTER_MAX_WIDTH})")


class InferenceSession:
    def __init__(self, model: FerModule, batch_size: int = 1, skinny: str = "auto",
                 input_shape: Optional[Tuple[int, ...]] = None, warmup: int = 2):
        """model: a FerModule in eval() mode on a ROCm device; batch_size: the B every run() takes;
        skinny: "auto" / "on" / "off" (module doc); input_shape: per-sample input shape, needed only for
        models the session cannot read it from (anything but LatentViT, LatentViTv2, ImageViT, HybridLatentViT,
        ExpressionAwareViT)."""
        if skinny not in ("auto", "on", "off"):
            raise ValueError(f"InferenceSession: skinny must be 'auto', 'on' or 'off', not {skinny!r}")
        if not isinstance(model, FerModule):
            raise TypeError("InferenceSession: the model must be a FerModule")
        if int(batch_size) < 1:
            raise ValueError("InferenceSession: batch_size must be >= 1")
        p = next(model.parameters(), None)
        if p is None or not p.is_cuda:
            raise RuntimeError("InferenceSession: the model is on the CPU: move it to a ROCm device first "
                               "(there is no CPU path)")
        self.source = model
        self.model = copy.deepcopy(model)  # the snapshot the graph reads (builds its own flat store)
        self.B = int(batch_size)
        self.device = p.device
        self.warmup = max(1, int(warmup))
        self._check_state()
        plan = _Plan(self.model)
        self.dtype = model.compute_dtype()
        rows = self.B * plan.N if plan.kind else 0
        why = plan.why
        if why is None and self.dtype != torch.bfloat16:
            why = "the model runs in fp32 (the skinny kernels are bf16)"
        if why is None and rows > SKINNY_MAX_ROWS:
            why = f"batch_size * tokens = {rows} rows exceeds the skinny kernels' {SKINNY_MAX_ROWS}"
        if skinny == "on" and why is not None:
            raise RuntimeError(f"InferenceSession: skinny='on' but {why}")
        auto_rows = SKINNY_AUTO_MAX_ROWS_PRENORM if plan.prenorm else SKINNY_AUTO_MAX_ROWS
        self.skinny = why is None and (skinny == "on" or (skinny == "auto" and rows <= auto_rows))
        self.plan = plan
        shape = tuple(input_shape) if input_shape is not None else (plan.sample_shape if plan.kind else None)
        if shape is None:
            raise ValueError("InferenceSession: pass input_shape (per sample) for this model")
        self.x_in = torch.zeros((self.B,) + tuple(shape), dtype=torch.float32, device=self.device)
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.out: Optional[torch.Tensor] = None
        self._addr = None
        self.captures = 0
        self._capture()

    # ------------------------------------------------------------------ checks
    def _check_state(self) -> None:
        if self.source.training:
            raise RuntimeError("InferenceSession: the model is in train() mode: call model.eval() first")
        if layers.ATTN_TAP is not None:
            raise RuntimeError("InferenceSession: an attention tap (fervit.layers.ATTN_TAP) is installed; "
                               "taps read activations on the host and cannot run inside a replayed graph")
        if layers.TOKEN_TAP is not None:
            raise RuntimeError("InferenceSession: a token tap (fervit.layers.TOKEN_TAP) is installed; "
                               "taps read activations on the host and cannot run inside a replayed graph")

    def _addresses(self, flat):
        return (id(flat), flat.data.data_ptr(), None if flat.half is None else flat.half.data_ptr())

    # ------------------------------------------------------------------ the two forwards
    def _forward(self) -> torch.Tensor:
        if not self.skinny:
            return self.model(self.x_in).float()
        return self._skinny_forward()

    def _prenorm_forward(self) -> torch.Tensor:
        m, plan, B, N = self.model, self.plan, self.B, self.plan.N
        core = plan.core
        flat = m.fer_flat()
        dt = torch.bfloat16
        x = self.x_in
        if plan.decompose is not None:
            x = plan.decompose(x)
        if plan.spec is not None:
            x = plan.spec().run(x, flat, False)
        cfg = LayerCfg(B=B, N=N, H=1, save=False)
        t = LatentTokensFn.apply(x, cfg, flat, dt, core.input_proj.weight, core.input_proj.bias, core.cls_token,
                                 core.pos_embed)
        M, D = t.shape
        for i, blk in enumerate(plan.blocks):
            a, mlp = blk.attn, blk.mlp
            H = a.num_heads
            dh = D // H
            ln1 = (blk.norm1.weight.data, blk.norm1.bias.data, blk.norm1.eps)
            ln2 = (blk.norm2.weight.data, blk.norm2.bias.data, blk.norm2.eps)
            qkv = ops.skinny_linear(t, flat.half_view(a.qkv.weight), a.qkv.bias.data, ln_a=ln1)
            o = torch.empty(M, D, dtype=dt, device=t.device)
            ops.attention_fwd(qkv, o, ops.attention_saved(qkv, B, N, H, dh), B, N, H, dh)
            x1 = ops.skinny_linear(o, flat.half_view(a.proj.weight), a.proj.bias.data, res=t)
            g = ops.skinny_linear(x1, flat.half_view(mlp.fc1.weight), mlp.fc1.bias.data, act="gelu", ln_a=ln2)
            t = ops.skinny_linear(g, flat.half_view(mlp.fc2.weight), mlp.fc2.bias.data, res=x1)
            if plan.adapters is not None:
                fc1, fc2 = plan.adapters[i].adapter[0], plan.adapters[i].adapter[2]
                t = ops.skinny_adapter(t, flat.half_view(fc1.weight), fc1.bias.data, flat.half_view(fc2.weight),
                                       fc2.bias.data, plan.adapters[i].alpha.data)
        # the head on the B CLS rows (row stride N): its LayerNorm is part of fer_head_fwd
        ln, lin = plan.head_ln, plan.head_lin
        logits, _ = ops.head_fwd(t, N, ln.weight.data, ln.bias.data, ln.eps, lin.weight.data, lin.bias.data, B)
        return logits

    def _skinny_forward(self) -> torch.Tensor:
        if self.plan.prenorm:
            return self._prenorm_forward()
        m, plan, B, N = self.model, self.plan, self.B, self.plan.N
        core = plan.core
        flat = m.fer_flat()
        dt = torch.bfloat16
        x = self.x_in
        if plan.spec is not None:
            x = plan.spec().run(x, flat, False)
        cfg = LayerCfg(B=B, N=N, H=1, dropout=0.0, save=False)
        if plan.kind == "latent":
            t = LatentTokensFn.apply(x, cfg, flat, dt, core.input_proj.weight, core.input_proj.bias, core.cls_token,
                                     core.pos_emb)
        else:
            pe = core.patch_embed.proj
            t = PatchTokensFn.apply(x, cfg, flat, dt, core.patch_size, pe.weight, pe.bias, core.cls_token,
                                    core.pos_embed)
        M, D = t.shape
        z, ln_prev = t, None
        for layer in plan.enc.layers:
            a = layer.self_attn
            H = a.num_heads
            dh = D // H
            ln1 = (layer.norm1.weight.data, layer.norm1.bias.data, layer.norm1.eps)
            qkv = ops.skinny_linear(z, flat.half_view(a.in_proj_weight), a.in_proj_bias.data, ln_a=ln_prev)
            o = torch.empty(M, D, dtype=dt, device=z.device)
            ops.attention_fwd(qkv, o, ops.attention_saved(qkv, B, N, H, dh), B, N, H, dh)
            y = ops.skinny_linear(o, flat.half_view(a.out_proj.weight), a.out_proj.bias.data, res=z, ln_res=ln_prev)
            g = ops.skinny_linear(y, flat.half_view(layer.linear1.weight), layer.linear1.bias.data,
                                  act=layer.activation, ln_a=ln1)
            z = ops.skinny_linear(g, flat.half_view(layer.linear2.weight), layer.linear2.bias.data, res=y, ln_res=ln1)
            ln_prev = (layer.norm2.weight.data, layer.norm2.bias.data, layer.norm2.eps)
        # the last LN2 on the B CLS rows only (row stride N * D), then the head on those rows
        cls = torch.empty(B, D, dtype=dt, device=z.device)
        ops.layernorm_fwd(z.view(B, N * D)[:, :D], ln_prev[0], ln_prev[1], ln_prev[2], out=cls)
        ln, lin = plan.head_ln, plan.head_lin
        logits, _ = ops.head_fwd(cls, 1, ln.weight.data, ln.bias.data, ln.eps, lin.weight.data, lin.bias.data, B)
        return logits

    # ------------------------------------------------------------------ capture / replay
    def _capture(self) -> None:
        self._check_state()
        self.graph = None
        cur = torch.cuda.current_stream(self.device)
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(cur)
        with torch.no_grad():
            with torch.cuda.stream(side):  # eager warm-up: sizes every workspace, casts the bf16 shadow
                for _ in range(self.warmup):
                    self._forward()
            cur.wait_stream(side)
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            side.wait_stream(cur)
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                self.out = self._forward()
            cur.wait_stream(side)
        self.graph = g
        # the library workspaces the captured launches point at (grow-only per stream: a later, larger request
        # on a stream with the same handle would otherwise free them under the graph)
        self._ws = [b for k, b in ops.WS.buf.items() if k[2] == side.cuda_stream]
        self._addr = self._addresses(self.model.fer_flat())
        self.captures += 1

    def run(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, ...] (device or host tensor) -> device fp32 logits [B, C] of this replay (the session's
        static output buffer). Enqueues a copy and one graph launch on the current stream; no host sync."""
        if self.graph is None:
            raise RuntimeError("InferenceSession: the session is closed")
        if tuple(x.shape) != tuple(self.x_in.shape):
            raise RuntimeError(f"InferenceSession: input shape {tuple(x.shape)} does not match the captured "
                               f"{tuple(self.x_in.shape)} (batch_size is fixed per session)")
        if self.source.training:
            raise RuntimeError("InferenceSession: the model is in train() mode: call model.eval() first")
        self.x_in.copy_(x, non_blocking=True)
        self.graph.replay()
        return self.out

    def predict(self, x: torch.Tensor):
        """(pred int64 [B], probs fp32 [B, C]) of run(x), on the device."""
        logits = self.run(x)
        return logits.argmax(dim=1), torch.softmax(logits, dim=1)

    def refresh(self) -> None:
        """Later runs use the model's current weights: they are copied into the session's private copy, whose
        flat store re-checks its parameters and re-casts its bf16 shadow; the graph is recaptured only if an
        address it captured has moved."""
        if self.graph is None:
            raise RuntimeError("InferenceSession: the session is closed")
        self._check_state()
        if self.source.compute_dtype() != self.dtype:
            raise RuntimeError("InferenceSession: the model's precision changed since the capture: open a new session")
        with torch.no_grad():
            self.model.load_state_dict(self.source.state_dict())
        flat = self.model.fer_flat()  # begin_pass: adopts re-pointed parameters, rebuilds a broken store
        if self.dtype == torch.bfloat16:
            flat.bf16()
        if self._addresses(flat) != self._addr:
            self._capture()

    def close(self) -> None:
        self.graph = None
        self.out = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
