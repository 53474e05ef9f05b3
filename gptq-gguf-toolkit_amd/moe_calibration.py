"""Fused experts in front of the Quantizer: a calibration stand-in for transformers' MixtralExperts (5.x), which keeps its
experts as two 3-D parameters, gate_up_proj [E, 2I, H] and down_proj [E, H, I] -- nothing a Linear-level quantizer can hook.

    installed = install(model, "model.layers.3.", regex, mode)   # Quantizer._quantize, per block, before select_layers
    ...                                                          # forward #1, the column walks, forward #2
    restore(installed)                                           # the original module is back, with the quantized weights

`CalibExperts` takes the place of a module that packed_experts.experts_shaped() accepts (SiLU only).  Per expert e it has
three nn.Linear children, `<e>.w1`, `<e>.w3`, `<e>.w2`, whose weights are VIEWS of the fused storage -- the gate rows
gate_up_proj[e, :I], the up rows gate_up_proj[e, I:], and down_proj[e]; nothing is copied.  GPTQ handles, BlockSchedule and its
leader / follower rule for shared inputs (w1 / w3) work on these children as on any Linear; `layer.weight.data = w`, how a
handle's result is written back, copies into the view (_SliceParameter), so the fused parameters hold the quantized weights
when the original module is put back.  The trees are written under the CHECKPOINT's names (checkpoint_name: `mlp.experts` in
memory is `block_sparse_moe.experts` on disk), which is what pack_gptq_into_gguf's index_map is keyed by.

Two forwards with the same result, bit for bit:

  * "loop", on any device: transformers' MixtralExperts.forward operation for operation -- the same one_hot / nonzero, the same
    torch.where order (by choice k, then by token), the same single F.linear on the fused [2I, H] slice, the same index_add_.
    The children's forward pre-hooks (what BlockSchedule registers) fire on the gathered [n_e, H] input and on act(gate) * up;
    an expert no token names is not called and its hooks never fire.
  * "routed", on the GPU: ops.moe_route on the TRANSPOSED index (pair p = k T + t: its stable sort yields transformers' row
    order inside each expert), one gather of x into the expert-sorted [n, H] matrix, ONE host read (expert_start: the counts)
    instead of E + 1, per expert a contiguous slice of that matrix through the same F.linear calls -- the slices are what the
    handles keep by reference --, and one ops.fwd_moe_combine launch instead of 3 E launches of multiply / cast / index_add_.
    The activation stays `act_fn(gate) * up` on the two halves of the fused GEMM's output: ops.fwd_silu_mul takes contiguous
    operands, and copying the halves out costs more than the two eager kernels.
    Routed is trusted the way forward_fused.py trusts a kernel: only after it has reproduced "loop" bit for bit on the first
    real input of a (T, K, E, H, I, dtype) class; a mismatch leaves "loop" in place for that class.  Inputs it does not take
    -- more pairs or experts than ops.moe_route sorts, K > 8, fp32, non-contiguous, H % 8, CPU tensors -- go to "loop".
"""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .packed_experts import PackedExperts, experts_shaped

# in-memory module path -> checkpoint tensor path of an expert Linear (transformers 5.x renames on load and on save)
NAME_TABLE = ((".mlp.experts.", ".block_sparse_moe.experts."),)
LINEARS = ("w1", "w3", "w2")  # gate rows, up rows, down: the order they are fed in
# fused_forward levels at which the routed forward is installed on the GPU (DESIGN.md K29 has the measurement behind it)
ROUTED_LEVELS = ("exact", "all")

_routed_verdict: Dict[tuple, bool] = {}  # (T, K, E, H, I, dtype) -> routed == loop on the first input of the class


def reset_verdicts() -> None:
    """Forget what has been verified (the Quantizer calls this at the start of a run)."""
    _routed_verdict.clear()


def checkpoint_name(module_name: str) -> str:
    """The name a synthesized expert Linear's tree is written under: the checkpoint's (iter_hf_entries') name of its tensor
    without ".weight".  A name outside NAME_TABLE is its own checkpoint name."""
    for mem, disk in NAME_TABLE:
        m = re.fullmatch(rf"(.*){re.escape(mem)}(\d+\.w[123])", module_name)
        if m:
            return f"{m.group(1)}{disk}{m.group(2)}"
    return module_name


def synthesized_names(name: str, num_experts: int) -> List[str]:
    """The Linear names CalibExperts exposes in place of the module `name`."""
    return [f"{name}.{e}.{w}" for e in range(num_experts) for w in LINEARS]


class _SliceParameter(nn.Parameter):
    """A Parameter over a slice of a fused expert tensor.  `p.data = w` -- how BlockSchedule writes a dequantized weight back
    -- copies into the slice instead of rebinding the Parameter: the write lands in the fused storage."""

    @property
    def data(self):
        return torch.Tensor.data.__get__(self)

    @data.setter
    def data(self, w):
        torch.Tensor.data.__get__(self).copy_(w)


def _view_linear(view: torch.Tensor) -> nn.Linear:
    lin = nn.Linear(view.shape[1], view.shape[0], bias=False, device="meta")  # (no storage of its own)
    lin.weight = _SliceParameter(view, requires_grad=False)
    return lin


class _Expert(nn.Module):
    def __init__(self, gate_up: torch.Tensor, down: torch.Tensor):
        super().__init__()
        inter = down.shape[1]
        self.w1, self.w3, self.w2 = _view_linear(gate_up[:inter]), _view_linear(gate_up[inter:]), _view_linear(down)


def _feed(linear: nn.Linear, x: torch.Tensor) -> None:
    """Fire `linear`'s forward pre-hooks on x, as nn.Module.__call__ would ahead of a GEMM that is not run here (the fused
    F.linear computes gate and up at once)."""
    for hook in list(linear._forward_pre_hooks.values()):
        if hook(linear, (x,)) is not None:
            raise NotImplementedError("CalibExperts: a forward pre-hook that replaces the input of an expert Linear")


def why_not_adaptable(layer: nn.Module) -> Optional[str]:
    """None when CalibExperts can stand in for `layer`, else the reason."""
    if isinstance(layer, (CalibExperts, PackedExperts)) or not experts_shaped(layer):
        return "it does not keep its experts as gate_up_proj [E, 2I, H] and down_proj [E, H, I]"
    if not isinstance(layer.gate_up_proj, nn.Parameter) or not isinstance(layer.down_proj, nn.Parameter):
        return "its gate_up_proj / down_proj are not parameters"
    if len(list(layer.parameters())) != 2:
        return "it holds more than the two fused parameters (a bias, a shared expert)"
    act = getattr(layer, "act_fn", None)
    if act is None or not (isinstance(act, nn.SiLU) or "silu" in type(act).__name__.lower()):
        return f"its activation is {type(act).__name__}, the calibration forward computes silu(gate) * up only"
    return None


class CalibExperts(nn.Module):
    def __init__(self, original: nn.Module, mode: str = "loop"):
        super().__init__()
        if mode not in ("loop", "routed"):
            raise ValueError(f"CalibExperts: mode must be 'loop' or 'routed', got {mode!r}")
        why = why_not_adaptable(original)
        if why:
            raise NotImplementedError(f"CalibExperts cannot stand in for a {type(original).__name__}: {why}")
        self.__dict__["original"] = original  # (not a child: its parameters are reachable through the views only)
        self.mode = mode
        self.num_experts, self.hidden_dim, self.intermediate_dim = (int(n) for n in original.down_proj.shape)
        self.train(original.training)
        for e in range(self.num_experts):
            self.add_module(str(e), _Expert(original.gate_up_proj.data[e], original.down_proj.data[e]))

    def expert(self, e: int) -> _Expert:
        return self._modules[str(int(e))]

    # ---------------------------------------------------------------------------------------------- forwards
    def forward(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor, top_k_weights: torch.Tensor) -> torch.Tensor:
        if self.mode != "routed" or not self._routed_takes(hidden_states, top_k_index, top_k_weights):
            return self._forward_loop(hidden_states, top_k_index, top_k_weights)
        T, K = top_k_index.shape
        key = (T, K, self.num_experts, self.hidden_dim, self.intermediate_dim, hidden_states.dtype)
        verdict = _routed_verdict.get(key)
        if verdict:
            return self._forward_routed(hidden_states, top_k_index, top_k_weights)
        if verdict is None:  # first input of this class: "loop" decides, and is what is returned (its hooks fire, once)
            got = self._forward_routed(hidden_states, top_k_index, top_k_weights, feed=False)
            want = self._forward_loop(hidden_states, top_k_index, top_k_weights)
            _routed_verdict[key] = bool(torch.equal(want, got))
            return want
        return self._forward_loop(hidden_states, top_k_index, top_k_weights)

    def _routed_takes(self, x, idx, w) -> bool:
        return (x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and x.dim() == 2 and x.is_contiguous()
                and idx.dim() == 2 and idx.shape[0] == x.shape[0] >= 1 and w.shape == idx.shape and w.is_contiguous()
                and w.dtype in (torch.float32, x.dtype) and 1 <= idx.shape[1] <= ops.MOE_COMBINE_MAX_K
                and idx.numel() <= ops.MOE_ROUTE_MAX_PAIRS and self.num_experts <= ops.MOE_ROUTE_MAX_EXPERTS
                and x.shape[1] % 8 == 0 and self.original.down_proj.dtype == x.dtype and not torch.is_grad_enabled())

    def _forward_loop(self, hidden_states, top_k_index, top_k_weights):
        """transformers' MixtralExperts.forward, operation for operation, with the children's pre-hooks in between."""
        o = self.original
        final_hidden_states = torch.zeros_like(hidden_states)
        with torch.no_grad():
            expert_mask = F.one_hot(top_k_index, num_classes=self.num_experts)
            expert_mask = expert_mask.permute(2, 1, 0)
            expert_hit = torch.greater(expert_mask.sum(dim=(-1, -2)), 0).nonzero()
        for expert_idx in expert_hit:
            expert_idx = expert_idx[0]
            if expert_idx == self.num_experts:
                continue
            top_k_pos, token_idx = torch.where(expert_mask[expert_idx])
            current_state = hidden_states[token_idx]
            ex = self.expert(expert_idx)
            _feed(ex.w1, current_state)
            _feed(ex.w3, current_state)
            gate, up = F.linear(current_state, o.gate_up_proj[expert_idx]).chunk(2, dim=-1)
            current_hidden_states = o.act_fn(gate) * up
            _feed(ex.w2, current_hidden_states)
            current_hidden_states = F.linear(current_hidden_states, o.down_proj[expert_idx])
            current_hidden_states = current_hidden_states * top_k_weights[token_idx, top_k_pos, None]
            final_hidden_states.index_add_(0, token_idx, current_hidden_states.to(final_hidden_states.dtype))
        return final_hidden_states

    def _forward_routed(self, x, top_k_index, top_k_weights, feed: bool = True):
        o, E = self.original, self.num_experts
        T, K = top_k_index.shape
        pairs = top_k_index.t().to(torch.int32).contiguous().view(-1)  # pair p = k T + t
        route = ops.moe_route(pairs, E)
        start = route[0].tolist()  # the one host read: where every expert's run begins, and the number of valid pairs
        n = start[E]
        if n == 0:
            return torch.zeros_like(x)
        sorted_x = x.index_select(0, torch.remainder(route[1][:n], T))  # row s: the token of pair order[s]
        ys = []
        for e in range(E):
            a, b = start[e], start[e + 1]
            if a == b:
                continue  # an expert no token names is not called
            current_state = sorted_x[a:b]
            ex = self.expert(e)
            if feed:
                _feed(ex.w1, current_state)
                _feed(ex.w3, current_state)
            gate, up = F.linear(current_state, o.gate_up_proj[e]).chunk(2, dim=-1)
            h = o.act_fn(gate) * up
            if feed:
                _feed(ex.w2, h)
            ys.append(F.linear(h, o.down_proj[e]))
        if n < T * K:  # masked pairs: rows from n on are never read, they only complete the [P, H] extent
            ys.append(x.new_empty(T * K - n, x.shape[1]))
        y = torch.cat(ys) if len(ys) > 1 else ys[0]
        return ops.fwd_moe_combine(y, pairs, route, top_k_weights, E)

    def extra_repr(self) -> str:
        return (f"num_experts={self.num_experts}, hidden_dim={self.hidden_dim}, intermediate_dim={self.intermediate_dim}, "
                f"mode={self.mode}, original={type(self.original).__name__}")


# ------------------------------------------------------------------------------------------------ install / restore
def _fused_expert_count(layer: nn.Module) -> int:
    """E when `layer` holds parameters of three or more dimensions of its own (experts fused along dim 0), else 0."""
    dims = [p.shape[0] for p in layer.parameters(recurse=False) if p.dim() >= 3]
    return int(dims[0]) if dims else 0


def named_fused_experts(model: nn.Module, prefix: str, regex: str) -> List[Tuple[str, nn.Module]]:
    """The modules under `prefix` ("model.layers.3.": a dotted module path) that keep fused experts AND at least one of whose
    synthesized Linear names `regex` matches."""
    out = []
    root = prefix.rstrip(".")
    for name, layer in (model.get_submodule(root) if root else model).named_modules(prefix=root):
        if not name.startswith(prefix) or isinstance(layer, CalibExperts):
            continue
        E = _fused_expert_count(layer)
        if E and any(re.search(regex, n) for n in synthesized_names(name, E)):
            out.append((name, layer))
    return out


def install(model: nn.Module, prefix: str, regex: str, mode: str = "loop") -> List[Tuple[nn.Module, str, nn.Module, str]]:
    """Replace every fused-expert module under `prefix` that `regex` names an expert Linear of by a CalibExperts; ->
    [(parent, attribute, original, module name)] for restore().  NotImplementedError, naming the module, when such a module
    cannot be adapted; a regex that names no expert installs nothing."""
    found = named_fused_experts(model, prefix, regex)
    for name, layer in found:  # everything is refused before anything is replaced
        why = why_not_adaptable(layer)
        if why:
            raise NotImplementedError(f"{name} ({type(layer).__name__}): --quantizable_modules names its experts, but {why}")
    installed = []
    for name, layer in found:
        parent_name, _, leaf = name.rpartition(".")
        parent = model.get_submodule(parent_name) if parent_name else model
        setattr(parent, leaf, CalibExperts(layer, mode))
        installed.append((parent, leaf, layer, name))
    return installed


def restore(installed) -> None:
    """Put the original modules back (their fused parameters hold whatever was written through the views)."""
    while installed:
        parent, leaf, original, _ = installed.pop()
        setattr(parent, leaf, original)
