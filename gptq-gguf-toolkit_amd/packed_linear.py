"""A Linear whose weight exists only in the form it is stored in: GGUF block bytes (K-quants, Q8_0, IQ4_NL, IQ4_XS) on the device.

    mods = install(model, names)                       # the named nn.Linear modules become PackedLinear, their dense storage is dropped
    mods[name].set_level(blocks, q_type, row_src)      # references only: no copy, no launch
    model(ids)                                         # forward = ops.linear_packed (gq_linear_packed): a GEMM that reads the block bytes
                                                       # (ops.gemv_packed for the 1 .. gemv_max_t tokens of a decode step)

The weight operand of that GEMM is, bit for bit, what a dense level switch (ops.level_switch) writes for the same level, so
a packed-resident model differs from a dense-resident one only by the fp32 summation order of its Linears.  A level that
is a dense tensor of the model's dtype (the database's plain F16 / BF16 levels) goes through F.linear on the stored tensor.
There is no fallback: a PackedLinear without a level, or with an input of another dtype, raises."""
from typing import Dict, Iterable, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._cabi import GQError


class PackedLinear(nn.Module):
    # Inputs of 1 .. gemv_max_t tokens go through ops.gemv_packed, everything else through ops.linear_packed; 0 switches the
    # routing off.  The default is the largest T at which profiles/qgemv_rate.txt has the GEMV no slower than the tile kernel
    # for every type and shape measured (DESIGN K22); an instance may override it.
    gemv_max_t = ops.GEMV_MAX_T

    def __init__(self, in_features: int, out_features: int, bias: Optional[nn.Parameter] = None,
                 dtype: torch.dtype = torch.float16):
        super().__init__()
        if dtype not in (torch.float16, torch.bfloat16):
            raise TypeError(f"PackedLinear computes in fp16 or bf16 (there is no fp32 path), not {dtype}")
        self.in_features, self.out_features = int(in_features), int(out_features)
        self.register_parameter("bias", bias)
        # what the search's bit accounting reads (weight.numel() / .shape / .dtype): a tensor without storage, no parameter
        self.weight = torch.empty(self.out_features, self.in_features, dtype=dtype, device="meta")
        self.blocks = self.q_type = self.row_src = None

    @property
    def dtype(self) -> torch.dtype:
        return self.weight.dtype

    def set_level(self, blocks: torch.Tensor, q_type: Optional[int], row_src: Optional[torch.Tensor] = None) -> None:
        """Make a stored level current: `blocks` packed uint8 with its q_type (10..14, 8, 20 or 23) and optional row gather, or
        q_type None and a dense [out_features, in_features] tensor of the module's dtype.  Keeps references only."""
        if q_type is None:
            if blocks.dtype != self.dtype or tuple(blocks.shape) != (self.out_features, self.in_features) or row_src is not None:
                raise GQError(f"PackedLinear.set_level: a dense level must be a {self.dtype} "
                              f"{(self.out_features, self.in_features)} tensor without a row gather; got {blocks.dtype} "
                              f"{tuple(blocks.shape)}")
        else:
            bs, ts = ops.block_geometry(q_type)
            need = self.out_features * (self.in_features // bs) * ts
            if blocks.dtype != torch.uint8 or self.in_features % 256 or blocks.numel() != need:
                raise GQError(f"PackedLinear.set_level: packed level of q_type {int(q_type)} for "
                              f"{(self.out_features, self.in_features)} must be {need} uint8 (in_features % 256 == 0); got "
                              f"{blocks.dtype} {tuple(blocks.shape)}")
        self.blocks, self.q_type, self.row_src = blocks, (None if q_type is None else int(q_type)), row_src

    def _need_level(self):
        if self.blocks is None:
            raise GQError("PackedLinear has no level yet (set_level was never called): there is no weight to compute with")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self._need_level()
        if self.q_type is None:
            return F.linear(x, self.blocks, self.bias)
        few = 1 <= x.numel() // self.in_features <= min(self.gemv_max_t, ops.GEMV_MAX_T)
        y = (ops.gemv_packed if few else ops.linear_packed)(self.q_type, self.blocks, x.contiguous(), self.row_src)
        return y if self.bias is None else y + self.bias

    @torch.no_grad()
    def dense_weight(self, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """The current level as a fresh [out_features, in_features] tensor (default: the module's dtype), decoded by the
        call a dense level switch makes."""
        self._need_level()
        out = torch.empty(self.out_features, self.in_features, dtype=dtype or self.dtype, device=self.blocks.device)
        ops.level_switch([(self.blocks, out, self.q_type, self.row_src)])
        return out

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"q_type={self.q_type}")


def replace_linear(model: nn.Module, name: str) -> PackedLinear:
    """Swap the nn.Linear `name` for a PackedLinear of its shape, dtype and bias; its dense weight is dropped."""
    layer = model.get_submodule(name)
    if not isinstance(layer, nn.Linear):
        raise TypeError(f"PackedLinear replaces nn.Linear only, {name} is a {type(layer).__name__}")
    packed = PackedLinear(layer.in_features, layer.out_features, layer.bias, layer.weight.dtype)
    packed.train(layer.training)
    parent, _, leaf = name.rpartition(".")
    setattr(model.get_submodule(parent) if parent else model, leaf, packed)
    return packed


def install(model: nn.Module, names: Iterable[str]) -> Dict[str, PackedLinear]:
    """{name: PackedLinear}: every named nn.Linear of `model` replaced; nothing holds their dense [R, C] storage afterwards
    (unless the caller does)."""
    return {name: replace_linear(model, name) for name in names}


def dense_bytes(layer: nn.Linear) -> int:
    """The device bytes replace_linear frees for this Linear."""
    return layer.weight.numel() * layer.weight.element_size()
