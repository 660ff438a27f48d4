"""FerModule: nn.Module base that owns (or shares) a FlatParams store.

The outermost FerModule that runs a forward owns the flat buffers of all its
parameters (nested FerModules share the owner's). The store is (re)built lazily on
the module's device, so `model.cuda()` / `model.to(dev)` keep working: the
Parameter objects stay the same (optimizers hold them), only their `.data` is
re-pointed at the flat views.
"""
from __future__ import annotations

import copy
import weakref
from typing import List, Optional

import torch
import torch.nn as nn

from .runtime import FlatParams, default_precision


class FerModule(nn.Module):
    def __init__(self):
        super().__init__()
        object.__setattr__(self, "_fer_flat", None)
        object.__setattr__(self, "_fer_owner", None)
        object.__setattr__(self, "fer_precision", default_precision())

    # ---- ordering hook: modules may reorder their parameters in the flat buffer
    def fer_param_order(self) -> List[nn.Parameter]:
        seen, out = set(), []
        for m in self.modules():
            hook = getattr(m, "_fer_local_order", None)
            if hook is not None:
                for p in hook():
                    if id(p) not in seen:
                        seen.add(id(p))
                        out.append(p)
        for p in self.parameters():
            if id(p) not in seen:
                seen.add(id(p))
                out.append(p)
        return out

    def _apply(self, fn, recurse=True):
        """`.cuda()` / `.to()` / `.float()`: the store is kept when the call changed nothing (every
        parameter is the same object, still fp32 on the same device, still its flat view -- an
        optimizer bound to the store keeps its moments) and dropped otherwise, to be rebuilt by
        the next forward."""
        r = super()._apply(fn, recurse)
        for m in self.modules():
            if isinstance(m, FerModule):
                holder, flat = m._fer_store()
                if flat is not None and not flat.intact():
                    holder._fer_drop()
        return r

    def __deepcopy__(self, memo):
        """The copy owns cloned, standalone parameters (Parameter.__deepcopy__) and no flat store,
        owner or hook state of the original: it builds its own store on its first forward."""
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = None if k in ("_fer_flat", "_fer_owner") else copy.deepcopy(v, memo)
        return new

    def _fer_store(self):
        """(module that holds it, flat store this module reads): the owner's, else its own."""
        owner = self._fer_owner() if self._fer_owner is not None else None
        if owner is not None and owner._fer_flat is not None:
            return owner, owner._fer_flat
        if self._fer_flat is not None:
            return self, self._fer_flat
        return None, None

    def _fer_drop(self) -> None:
        for m in self.modules():
            if isinstance(m, FerModule):
                object.__setattr__(m, "_fer_flat", None)
                object.__setattr__(m, "_fer_owner", None)

    def fer_params_changed(self) -> None:
        """Call after writing parameters in place through `.data` (`p.data.mul_()`,
        `p.data.copy_()`): such writes bump no version counter, so nothing else tells the bf16
        shadow and its transposed copies to refresh. (In-place ops on the Parameter under
        no_grad, nn.init, load_state_dict, torch optimizers and `p.data = t` need no call.)"""
        flat = self._fer_store()[1]
        if flat is not None:
            flat.mark_stale()

    def fer_flat(self) -> FlatParams:
        holder, flat = self._fer_store()
        if flat is not None:
            if holder is not self and flat.owner_active:
                return flat
            # the owner's forward, or a child module run on its own (e.g. `model.backbone(x)`, not
            # inside the owner's forward): start a pass so the store re-checks the parameters
            # (they may have been changed in place, re-pointed or replaced since the last pass)
            if flat.begin_pass():
                return flat
            holder._fer_drop()
        params = self.fer_param_order()
        if not params:
            raise RuntimeError("fervit: module has no parameters")
        if not params[0].is_cuda:
            raise RuntimeError("fervit: move the model to a ROCm device first (no CPU path)")
        slots = [(m._parameters, n, p) for m in self.modules() for n, p in m._parameters.items() if p is not None]
        object.__setattr__(self, "_fer_flat", FlatParams(params, slots))
        # the hooks look the store up on the module they run on, so a deep copy's act on its own
        if _enter not in self._forward_pre_hooks.values():
            self.register_forward_pre_hook(_enter)
            self.register_forward_hook(_leave, always_call=True)
        ref = weakref.ref(self)
        for m in self.modules():
            if m is not self and isinstance(m, FerModule):
                object.__setattr__(m, "_fer_owner", ref)
                object.__setattr__(m, "_fer_flat", None)
        return self._fer_flat

    def set_precision(self, precision: str):
        """'bf16' (MFMA fast path, fp32 accumulation) or 'fp32' (exact parity path)."""
        if precision not in ("bf16", "fp32"):
            raise ValueError(precision)
        for m in self.modules():
            if isinstance(m, FerModule):
                object.__setattr__(m, "fer_precision", precision)
        return self

    def compute_dtype(self) -> torch.dtype:
        return torch.bfloat16 if self.fer_precision == "bf16" else torch.float32

    @staticmethod
    def need_grad(x: Optional[torch.Tensor], params) -> bool:
        if not torch.is_grad_enabled():
            return False
        if x is not None and x.requires_grad:
            return True
        return any(p.requires_grad for p in params)


def _enter(m, _inp):
    if m._fer_flat is not None:
        m._fer_flat.owner_active = True


def _leave(m, _inp, _out):
    if m._fer_flat is not None:
        m._fer_flat.owner_active = False
