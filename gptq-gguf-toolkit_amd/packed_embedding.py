"""An Embedding whose table exists only in the form it is stored in: GGUF block bytes (K-quants, Q8_0, IQ4_NL, IQ4_XS) on the device.

    emb = replace_embedding(model, "model.embed_tokens")   # the nn.Embedding becomes a PackedEmbedding, its dense table is dropped
    emb.set_level(blocks, q_type)                          # a reference only: no copy, no launch
    model(ids)                                             # forward = ops.embed_packed: the rows `ids` decoded from the block bytes

The rows it returns are, bit for bit, the rows of ops.dequantize_blocks(q_type, blocks, dtype): a packed embedding and a
dense-loaded one are the same function.  `blocks` may be the tensor a PackedLinear lm_head holds (a tied model: one device
copy serves both ends).  A level that is a dense tensor of the module's dtype goes through F.embedding.  There is no
fallback: a PackedEmbedding without a level raises.  Token ids are not range-checked on the device."""
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._cabi import GQError


class PackedEmbedding(nn.Module):
    def __init__(self, num_embeddings: int, embedding_dim: int, dtype: torch.dtype = torch.float16):
        super().__init__()
        if dtype not in (torch.float16, torch.bfloat16, torch.float32):
            raise TypeError(f"PackedEmbedding decodes to fp16, bf16 or fp32, not {dtype}")
        self.num_embeddings, self.embedding_dim = int(num_embeddings), int(embedding_dim)
        # what shape / dtype readers see (weight.numel() / .shape / .dtype): a tensor without storage, no parameter
        self.weight = torch.empty(self.num_embeddings, self.embedding_dim, dtype=dtype, device="meta")
        self.blocks = self.q_type = None

    @property
    def dtype(self) -> torch.dtype:
        return self.weight.dtype

    def set_level(self, blocks: torch.Tensor, q_type: Optional[int]) -> None:
        """Make a stored table current: `blocks` packed uint8 with its q_type (10..14 or 8), or q_type None and a dense
        [num_embeddings, embedding_dim] tensor of the module's dtype.  Keeps a reference only."""
        shape = (self.num_embeddings, self.embedding_dim)
        if q_type is None:
            if blocks.dtype != self.dtype or tuple(blocks.shape) != shape:
                raise GQError(f"PackedEmbedding.set_level: a dense level must be a {self.dtype} {shape} tensor; got "
                              f"{blocks.dtype} {tuple(blocks.shape)}")
        else:
            bs, ts = ops.block_geometry(q_type)
            need = self.num_embeddings * (self.embedding_dim // bs) * ts
            if blocks.dtype != torch.uint8 or self.embedding_dim % 256 or blocks.numel() != need:
                raise GQError(f"PackedEmbedding.set_level: packed level of q_type {int(q_type)} for {shape} must be {need} "
                              f"uint8 (embedding_dim % 256 == 0); got {blocks.dtype} {tuple(blocks.shape)}")
        self.blocks, self.q_type = blocks, (None if q_type is None else int(q_type))

    def forward(self, ids: torch.Tensor) -> torch.Tensor:
        if self.blocks is None:
            raise GQError("PackedEmbedding has no level yet (set_level was never called): there is no table to read")
        if self.q_type is None:
            return F.embedding(ids, self.blocks)
        return ops.embed_packed(self.q_type, self.blocks.view(self.num_embeddings, -1), ids, self.dtype)

    def extra_repr(self) -> str:
        return f"num_embeddings={self.num_embeddings}, embedding_dim={self.embedding_dim}, q_type={self.q_type}"


def replace_embedding(model: nn.Module, name: str) -> PackedEmbedding:
    """Swap the nn.Embedding `name` for a PackedEmbedding of its shape and dtype; its dense table is dropped."""
    layer = model.get_submodule(name)
    if not isinstance(layer, nn.Embedding):
        raise TypeError(f"PackedEmbedding replaces nn.Embedding only, {name} is a {type(layer).__name__}")
    # (padding_idx only stops gradients: the forward value of an nn.Embedding does not depend on it)
    packed = PackedEmbedding(layer.num_embeddings, layer.embedding_dim, layer.weight.dtype)
    packed.train(layer.training)
    parent, _, leaf = name.rpartition(".")
    setattr(model.get_submodule(parent) if parent else model, leaf, packed)
    return packed
