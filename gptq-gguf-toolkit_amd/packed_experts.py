"""The experts of a sparse-MoE layer whose weights exist only in the form they are stored in: the stacked GGUF tensors
`blk.N.ffn_{gate,up,down}_exps.weight` as block bytes (K-quants, Q8_0, IQ4_NL, IQ4_XS) on the device.

    mods = install_experts(model, names)        # the named MixtralExperts-shaped modules become PackedExperts, their dense
                                                # [E, 2I, H] / [E, H, I] parameters are dropped (prefill="grouped": see below)
    mods[name].set_level("gate", blocks, q_type)  # and "up", "down": references only, no copy, no launch
    model(ids)

PackedExperts.forward has the signature of transformers' MixtralExperts.forward (hidden_states [T, H], top_k_index [T, K],
top_k_weights [T, K]).  Three paths:

  * the decode path, for T <= gemv_max_t tokens and T * K <= grouped_max_pairs pairs with all three levels packed: three
    ops.gemv_packed_experts launches (gate, up, down: one launch each over every (token, expert) pair, the expert ids read
    on the device), ops.fwd_silu_mul in between, then the sum over k in fp32, k ascending, and one rounding to the model's
    dtype.  Nothing on this path reads a result back: no nonzero, no where-without-other, no .item().
  * the prefill path, for any other input of a module with prefill = "grouped", all three levels packed and at most
    ops.MOE_ROUTE_MAX_EXPERTS experts: per chunk of at most prefill_max_pairs // K tokens one ops.moe_route launch (the
    pairs sorted by expert on the device), three ops.linear_packed_experts launches (gate and up with the hidden states,
    down with the [P, I] activation; an expert's tokens are gathered and its results scattered to pair order inside the
    kernel) with ops.fwd_silu_mul in between, and the decode path's combine.  Nothing on this path reads a result back
    either: no unique, no nonzero, no where-without-other, no .item().  The chunks bound the three [P, I] temporaries
    (about 0.7 GB at Mixtral's I = 14336 and the default 8192 pairs).
  * the loop path, otherwise (prefill = "loop" is the default): per hit expert its tokens are gathered and multiplied with the expert's slice of the stacked
    tensor (a view) by ops.gemv_packed (1 .. gemv_max_t tokens) or ops.linear_packed, and added with index_add_, as
    transformers does.  Finding the hit experts and their tokens synchronises with the host.

The paths are one model up to the fp32 summation order of the GEMMs and of the sum over k (the loop path rounds every
expert's term and adds in the module's dtype; the other two add in fp32 and round once).  A level that is a dense
[E, R, C] tensor of the module's dtype goes through F.linear on its slice (loop path only).  There is no fallback: a
PackedExperts without its three levels, or with an input of another dtype, raises."""
from typing import Dict, Iterable, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._cabi import GQError

ROLES = ("gate", "up", "down")


class PackedExperts(nn.Module):
    # T <= gemv_max_t and T * K <= grouped_max_pairs take the decode path; grouped_max_pairs = 0 switches it off.  The
    # defaults are the kernels' limits (DESIGN K24 has the measurement); an instance may override either.
    gemv_max_t = ops.GEMV_MAX_T
    grouped_max_pairs = ops.MOE_MAX_PAIRS
    # What an input that does not take the decode path takes: "loop" (per hit expert, with host synchronisations) or "grouped"
    # (device-side routing and one grouped GEMM per projection, in chunks of at most prefill_max_pairs // K tokens; DESIGN K25
    # has the measurement).  An instance may override either.
    prefill = "loop"
    prefill_max_pairs = 8192

    def __init__(self, num_experts: int, hidden_dim: int, intermediate_dim: int, dtype: torch.dtype = torch.float16):
        super().__init__()
        if dtype not in (torch.float16, torch.bfloat16):
            raise TypeError(f"PackedExperts computes in fp16 or bf16 (there is no fp32 path), not {dtype}")
        self.num_experts, self.hidden_dim, self.intermediate_dim = int(num_experts), int(hidden_dim), int(intermediate_dim)
        E, H, I = self.num_experts, self.hidden_dim, self.intermediate_dim
        # shape and bit accounting only (numel() / .shape / .dtype): tensors without storage, no parameters
        self.gate_up_proj = torch.empty(E, 2 * I, H, dtype=dtype, device="meta")
        self.down_proj = torch.empty(E, H, I, dtype=dtype, device="meta")
        self.levels: Dict[str, Optional[tuple]] = {r: None for r in ROLES}  # role -> (blocks, q_type or None)

    @property
    def dtype(self) -> torch.dtype:
        return self.down_proj.dtype

    def role_shape(self, role: str):
        """(R, C) of one expert's matrix: gate / up [I, H], down [H, I]."""
        if role not in ROLES:
            raise GQError(f"PackedExperts: role {role!r} is not one of {ROLES}")
        return (self.hidden_dim, self.intermediate_dim) if role == "down" else (self.intermediate_dim, self.hidden_dim)

    def set_level(self, role: str, blocks: torch.Tensor, q_type: Optional[int]) -> None:
        """Make a stored level current for "gate", "up" or "down": `blocks` the stacked tensor's packed uint8 bytes (expert
        major, as in the file) with its q_type (10..14 or 8), or q_type None and a dense [E, R, C] tensor of the module's
        dtype.  Each role has its own type.  Keeps references only."""
        R, C = self.role_shape(role)
        E = self.num_experts
        if q_type is None:
            if blocks.dtype != self.dtype or tuple(blocks.shape) != (E, R, C):
                raise GQError(f"PackedExperts.set_level({role}): a dense level must be a {self.dtype} {(E, R, C)} tensor; got "
                              f"{blocks.dtype} {tuple(blocks.shape)}")
        else:
            bs, ts = ops.block_geometry(q_type)
            need = E * R * (C // bs) * ts
            if blocks.dtype != torch.uint8 or C % 256 or blocks.numel() != need or not blocks.is_contiguous():
                raise GQError(f"PackedExperts.set_level({role}): packed level of q_type {int(q_type)} for {(E, R, C)} must be "
                              f"{need} contiguous uint8 (C % 256 == 0); got {blocks.dtype} {tuple(blocks.shape)}")
        self.levels[role] = (blocks, None if q_type is None else int(q_type))

    def _level(self, role: str):
        if self.levels[role] is None:
            raise GQError(f"PackedExperts has no {role} level yet (set_level was never called): there is no weight to compute with")
        return self.levels[role]

    def _linear(self, role: str, e: int, x: torch.Tensor) -> torch.Tensor:
        """x [n, C] times expert e's matrix of `role`, read from its slice of the stacked tensor (a view, no copy)."""
        blocks, q_type = self._level(role)
        if q_type is None:
            return F.linear(x, blocks[e])
        few = 1 <= x.shape[0] <= min(self.gemv_max_t, ops.GEMV_MAX_T)
        return (ops.gemv_packed if few else ops.linear_packed)(q_type, blocks.view(self.num_experts, -1)[e], x.contiguous())

    def takes_decode_path(self, T: int, K: int) -> bool:
        """Whether forward sends T tokens with K experts each through the three grouped launches."""
        return (1 <= T <= min(self.gemv_max_t, ops.GEMV_MAX_T) and 1 <= T * K <= min(self.grouped_max_pairs, ops.MOE_MAX_PAIRS)
                and all(self.levels[r] is not None and self.levels[r][1] is not None for r in ROLES))

    def takes_prefill_path(self, T: int, K: int) -> bool:
        """Whether forward sends T tokens with K experts each through the device-side routing and the grouped GEMMs."""
        return (self.prefill == "grouped" and T >= 1 and 1 <= K <= min(self.prefill_max_pairs, ops.MOE_ROUTE_MAX_PAIRS)
                and self.num_experts <= ops.MOE_ROUTE_MAX_EXPERTS and not self.takes_decode_path(T, K)
                and all(self.levels[r] is not None and self.levels[r][1] is not None for r in ROLES))

    def forward(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor, top_k_weights: torch.Tensor) -> torch.Tensor:
        for r in ROLES:
            self._level(r)
        if hidden_states.dtype != self.dtype or hidden_states.dim() != 2 or hidden_states.shape[1] != self.hidden_dim:
            raise GQError(f"PackedExperts.forward: hidden_states must be {self.dtype} [T, {self.hidden_dim}]; got "
                          f"{hidden_states.dtype} {tuple(hidden_states.shape)}")
        T, K = top_k_index.shape
        if T != hidden_states.shape[0] or tuple(top_k_weights.shape) != (T, K):
            raise GQError(f"PackedExperts.forward: top_k_index {tuple(top_k_index.shape)} and top_k_weights "
                          f"{tuple(top_k_weights.shape)} must both be [T={hidden_states.shape[0]}, K]")
        if self.prefill not in ("loop", "grouped"):
            raise GQError(f"PackedExperts.prefill must be 'loop' or 'grouped', got {self.prefill!r}")
        if self.takes_decode_path(T, K):
            return self._forward_grouped(hidden_states.contiguous(), top_k_index, top_k_weights)
        if self.takes_prefill_path(T, K):
            return self._forward_prefill(hidden_states.contiguous(), top_k_index, top_k_weights)
        return self._forward_loop(hidden_states, top_k_index, top_k_weights)

    def _combine(self, down, pairs, top_k_weights):
        """out [T, H] = sum_k w[t, k] down[t K + k] over the valid pairs: fp32, k ascending, one rounding to the module's dtype.  A
        pair whose id lies outside [0, E) was skipped by the launches (its rows hold whatever the allocator left, NaN
        included): it contributes nothing, as in transformers, where E is the id of a masked pair."""
        T, K = top_k_weights.shape
        valid = ((pairs >= 0) & (pairs < self.num_experts)).view(T, K, 1)
        terms = torch.where(valid, down.view(T, K, -1).float() * top_k_weights.float().unsqueeze(-1), 0.0)
        acc = terms[:, 0]
        for k in range(1, K):  # fp32, k ascending
            acc = acc + terms[:, k]
        return acc.to(self.dtype)

    def _forward_grouped(self, x, top_k_index, top_k_weights):
        E, I, H = self.num_experts, self.intermediate_dim, self.hidden_dim
        T, K = top_k_index.shape
        pairs = top_k_index.reshape(-1).to(torch.int32)  # pair p = (token p // K, choice p % K); stays on the device
        (gb, gq), (ub, uq), (db, dq) = (self.levels[r] for r in ROLES)
        gate = ops.gemv_packed_experts(gq, gb, E, I, x, pairs, K)
        up = ops.gemv_packed_experts(uq, ub, E, I, x, pairs, K)
        down = ops.gemv_packed_experts(dq, db, E, H, ops.fwd_silu_mul(gate, up), pairs, 1)  # [T * K, H]
        return self._combine(down, pairs, top_k_weights)

    def _forward_prefill(self, x, top_k_index, top_k_weights):
        E, I, H = self.num_experts, self.intermediate_dim, self.hidden_dim
        T, K = top_k_index.shape
        (gb, gq), (ub, uq), (db, dq) = (self.levels[r] for r in ROLES)
        step = max(1, min(self.prefill_max_pairs, ops.MOE_ROUTE_MAX_PAIRS) // K)  # tokens of a chunk
        outs = []
        for t0 in range(0, T, step):
            xs, ws = x[t0:t0 + step], top_k_weights[t0:t0 + step]
            pairs = top_k_index[t0:t0 + step].reshape(-1).to(torch.int32)  # stays on the device
            route = ops.moe_route(pairs, E)
            gate = ops.linear_packed_experts(gq, gb, E, I, xs, route, K)
            up = ops.linear_packed_experts(uq, ub, E, I, xs, route, K)
            down = ops.linear_packed_experts(dq, db, E, H, ops.fwd_silu_mul(gate, up), route, 1)  # [pairs, H]
            outs.append(self._combine(down, pairs, ws))
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    def _forward_loop(self, hidden_states, top_k_index, top_k_weights):
        out = torch.zeros_like(hidden_states)
        with torch.no_grad():
            hit = torch.unique(top_k_index).tolist()  # (host synchronisation: accepted on this path)
        for e in hit:
            if not 0 <= e < self.num_experts:
                continue
            top_k_pos, token_idx = torch.where((top_k_index == e).T)  # transformers' order: by choice, then by token
            cur = hidden_states[token_idx]
            h = ops.fwd_silu_mul(self._linear("gate", e, cur), self._linear("up", e, cur))
            h = self._linear("down", e, h) * top_k_weights[token_idx, top_k_pos, None]
            out.index_add_(0, token_idx, h.to(out.dtype))
        return out

    @torch.no_grad()
    def dense_weight(self, role: str, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """The current level of "gate", "up" or "down" as a fresh [E, R, C] tensor (default: the module's dtype), decoded by
        the call a dense level switch makes."""
        R, C = self.role_shape(role)
        blocks, q_type = self._level(role)
        out = torch.empty(self.num_experts * R, C, dtype=dtype or self.dtype, device=blocks.device)
        ops.level_switch([(blocks.reshape(self.num_experts * R, -1) if q_type is None else blocks, out, q_type, None)])
        return out.view(self.num_experts, R, C)

    @torch.no_grad()
    def dense_gate_up(self, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """transformers' fused parameter [E, 2I, H]: per expert the gate rows, then the up rows."""
        return torch.cat([self.dense_weight("gate", dtype), self.dense_weight("up", dtype)], dim=1)

    def extra_repr(self) -> str:
        types = ", ".join(f"{r}_q_type={None if self.levels[r] is None else self.levels[r][1]}" for r in ROLES)
        return (f"num_experts={self.num_experts}, hidden_dim={self.hidden_dim}, intermediate_dim={self.intermediate_dim}, "
                f"{types}")


def experts_shaped(layer: nn.Module) -> bool:
    """Whether `layer` keeps its experts the way transformers' MixtralExperts does: gate_up_proj [E, 2I, H] and down_proj
    [E, H, I]."""
    gu, dn = getattr(layer, "gate_up_proj", None), getattr(layer, "down_proj", None)
    return (isinstance(gu, torch.Tensor) and isinstance(dn, torch.Tensor) and gu.dim() == 3 and dn.dim() == 3
            and gu.shape[0] == dn.shape[0] and gu.shape[1] == 2 * dn.shape[2] and gu.shape[2] == dn.shape[1])


def replace_experts(model: nn.Module, name: str, prefill: str = "loop") -> PackedExperts:
    """Swap the MixtralExperts-shaped module `name` for a PackedExperts of its shape and dtype; its dense parameters are
    dropped.  The activation must be SiLU (ops.fwd_silu_mul is the only fused activation).  prefill: "loop" (the class
    default) or "grouped", the path of inputs beyond the decode step."""
    if prefill not in ("loop", "grouped"):
        raise ValueError(f"PackedExperts: prefill must be 'loop' or 'grouped', got {prefill!r}")
    layer = model.get_submodule(name)
    if isinstance(layer, PackedExperts) or not experts_shaped(layer):
        raise TypeError(f"PackedExperts replaces a module with gate_up_proj [E, 2I, H] and down_proj [E, H, I] only, {name} is "
                        f"a {type(layer).__name__}")
    act = getattr(layer, "act_fn", None)
    if act is not None and not isinstance(act, nn.SiLU) and "silu" not in type(act).__name__.lower():
        raise TypeError(f"PackedExperts computes silu(gate) * up only, {name} has the activation {type(act).__name__}")
    E, H, I = layer.down_proj.shape
    packed = PackedExperts(E, H, I, layer.down_proj.dtype)
    packed.train(layer.training)
    if prefill != PackedExperts.prefill:
        packed.prefill = prefill
    parent, _, leaf = name.rpartition(".")
    setattr(model.get_submodule(parent) if parent else model, leaf, packed)
    return packed


def install_experts(model: nn.Module, names: Iterable[str], prefill: str = "loop") -> Dict[str, PackedExperts]:
    """{name: PackedExperts}: every named expert module of `model` replaced; nothing holds their dense storage afterwards
    (unless the caller does).  prefill="grouped": their inputs beyond the decode step take the device-side routing and the
    grouped GEMMs instead of the per-expert loop."""
    return {name: replace_experts(model, name, prefill) for name in names}
