"""The projections of one input of a packed dense layer's decode step in one launch each (ops.gemv_packed_group_q8,
ops.gemv_swiglu_packed_q8; gq_gemv_packed_group_a8): with decode_act="q8" a Llama / Qwen3 layer at T <= ops.GEMV_A8_MAX_T
issues four Linear launches -- qkv, o, gate-up-SwiGLU, down -- instead of eight.

    n = install_groups(model)      # after the levels are set (gguf_loader.load_into_model(..., packed_decode_group=True) does this)
    model(ids)                     # the same logits, bit for bit
    restore(model)                 # undoes it

q / k / v.  The module that holds q_proj, k_proj and v_proj is not touched: the three PackedLinear children share one
QKVGroup.  When q_proj is called on an input the group serves, ONE launch computes all three outputs; the group keeps the input
tensor object and the outputs of k and v, and a sibling called with THAT tensor object (`x is group.x`, unchanged since) takes
its output, exactly once.  A sibling called with any other input, or before q_proj, takes its own PackedLinear.forward, so the
result is right in every order and for every caller.  The bias is added per member afterwards, as PackedLinear does.

gate / up.  An MLP with gate_proj, up_proj, down_proj as PackedLinear and a SiLU act_fn gets an instance `forward` that runs,
for such inputs, ops.gemv_swiglu_packed_q8 (gate and up of one type; the gate and up results are never written) or, for a
mixed pair, ops.gemv_packed_group_q8 and ops.fwd_silu_mul, and then down_proj.  Every other input takes the class's forward.

An input is served when it has 1 .. ops.GEMV_A8_MAX_T tokens, every member holds a packed level of ops.A8_TYPES with
decode_act == "q8" and its quantized image fits LDS (ops.gemv_a8_plan) -- the conditions under which each member alone would
run ops.gemv_packed_q8, whose bits the group launch repeats.  The levels are read at call time: a level switch needs no
reinstall.  There is no fallback to a dense weight anywhere."""
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .packed_linear import PackedLinear


def _served(members: List[PackedLinear], x: torch.Tensor) -> bool:
    C = members[0].in_features
    T = x.numel() // C
    return (1 <= T <= ops.GEMV_A8_MAX_T and x.shape[-1] == C
            and all(m.decode_act == "q8" and m.q_type in ops.A8_TYPES and m.in_features == C for m in members)
            and ops.gemv_a8_plan(T, 1, C)["fits"])


class QKVGroup:
    """The shared state of the q / k / v PackedLinear of one attention block (the module docstring's protocol)."""

    def __init__(self, members: List[PackedLinear]):
        self.members = list(members)
        self.x: Optional[torch.Tensor] = None  # the input the kept outputs belong to
        self.version = 0
        self.kept = {}                         # member index -> output not yet taken

    def forward(self, i: int, x: torch.Tensor) -> torch.Tensor:
        me = self.members[i]
        if i == 0 and _served(self.members, x):
            ys = ops.gemv_packed_group_q8([(m.q_type, m.blocks, m.row_src) for m in self.members], x.contiguous())
            self.x, self.version, self.kept = x, x._version, dict(enumerate(ys))
        if self.x is x and self.version == x._version and i in self.kept:
            y = self.kept.pop(i)
            if not self.kept:
                self.x = None
            return y if me.bias is None else y + me.bias
        return PackedLinear.forward(me, x)


def _is_silu(act) -> bool:
    return isinstance(act, nn.SiLU) or act is F.silu or type(act).__name__ == "SiLUActivation"


def _mlp_forward(mlp: nn.Module, x: torch.Tensor) -> torch.Tensor:
    g, u = mlp.gate_proj, mlp.up_proj
    if g.bias is not None or u.bias is not None or g.out_features != u.out_features or not _served([g, u], x):
        return type(mlp).forward(mlp, x)
    x = x.contiguous()
    if g.q_type == u.q_type and g.row_src is None and u.row_src is None:
        act = ops.gemv_swiglu_packed_q8(g.q_type, g.blocks, u.blocks, x)
    else:
        act = ops.fwd_silu_mul(*ops.gemv_packed_group_q8([(g.q_type, g.blocks, g.row_src), (u.q_type, u.blocks, u.row_src)], x))
    return mlp.down_proj(act)


def _packed(mod: nn.Module, names) -> Optional[List[PackedLinear]]:
    kids = [getattr(mod, n, None) for n in names]
    return kids if all(isinstance(k, PackedLinear) and k.decode_act == "q8" for k in kids) else None


def install_groups(model: nn.Module) -> int:
    """Attach a QKVGroup to every (q_proj, k_proj, v_proj) and the fused forward to every (gate_proj, up_proj, down_proj) MLP
    with a SiLU act_fn, where these are PackedLinear with decode_act == "q8" -> the number of groups attached.  Idempotent."""
    restore(model)
    n = 0
    for mod in list(model.modules()):
        qkv = _packed(mod, ("q_proj", "k_proj", "v_proj"))
        if qkv:
            group = QKVGroup(qkv)
            for i, m in enumerate(qkv):
                m.forward = lambda x, group=group, i=i: group.forward(i, x)
                m.decode_group = group
            n += 1
        if _packed(mod, ("gate_proj", "up_proj", "down_proj")) and _is_silu(getattr(mod, "act_fn", None)):
            mod.forward = lambda x, mod=mod: _mlp_forward(mod, x)
            mod.decode_group = True
            n += 1
    return n


def restore(model: nn.Module) -> None:
    """Undo install_groups: every module calls its class's forward again."""
    for mod in model.modules():
        if "decode_group" in mod.__dict__:
            del mod.__dict__["decode_group"], mod.__dict__["forward"]
