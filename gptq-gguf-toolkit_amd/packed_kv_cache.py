"""A KV cache kept as Q8_0 blocks (8.5 bits per value instead of 16) for the decode of `generate`: llama.cpp's
`-ctk q8_0 -ctv q8_0`.  Q8KVCache is a transformers Cache whose layers own uint8 [B, Hkv, S_cap, D / 32 * 34] tensors for K and
V (the layout of include/gptq_gguf_kvcache.h); update() encodes the new rows with ops.kv_append_q8_0 and the attention function
registered here reads them in that form with ops.attn_decode_q8_0.

    cache = Q8KVCache(model.config, batch, capacity, dtype, device)
    install(model, cache)
    try:
        out = model(input_ids=ids, past_key_values=cache, use_cache=True)   # ... and the decode steps
    finally:
        restore(model)

The attention function takes the kernel for the steps of a decode -- G * T <= ops.ATTN_DECODE_MAX_COLS query columns per KV
head on a non-empty cache, under a causal mask with optional left padding -- and the fallback otherwise: the prefill, a mask
of any other form, more tokens.  The fallback decodes the slabs it needs with ops.dequantize_blocks and calls torch SDPA with
the caller's mask; on an empty cache the prefill attends over the fresh 16-bit K / V, as llama.cpp does.  Left padding is
declared by the caller (`cache.set_left_padding(attention_mask)`): a 4-D mask is not searched for its form on the device, so an
undeclared mask is a general one.  Architectures: those whose attention is LlamaAttention's forward (Llama, Mixtral, Qwen3);
a model with sliding-window layers is refused by name.

`Q8KVCache(..., prefill="q8_0")` sends the calls of MORE than ops.ATTN_DECODE_MAX_COLS columns on a non-empty cache -- a later
chunk of a prompt fed in pieces, a later turn of a conversation -- to ops.attn_prefill_q8_0, which reads the cache at its stored
size, under the same condition on the mask; the default prefill="sdpa" keeps the fallback for them."""
import torch
from transformers import AttentionInterface, AttentionMaskInterface
from transformers.cache_utils import Cache, CacheLayerMixin
from transformers.masking_utils import sdpa_mask

from . import ops

ATTN_NAME = "gq_q8_kv"
MODEL_TYPES = ("llama", "mixtral", "qwen3")
PREFILLS = ("sdpa", "q8_0")  # many query columns over a non-empty cache: the 16-bit fallback, or gq_attn_prefill_q8_0


class Q8Layer(CacheLayerMixin):
    """K and V of one layer as Q8_0 rows; `length` positions of `capacity` are filled (the host owns the length)."""
    is_sliding = False
    is_compileable = False

    def __init__(self, batch, kv_heads, head_dim, capacity, device):
        super().__init__()
        self.row_bytes = ops.kv_row_bytes(head_dim)
        self.batch, self.kv_heads, self.head_dim, self.device = batch, kv_heads, head_dim, device
        self.capacity = max(4, (int(capacity) + 3) // 4 * 4)
        self.length = 0
        self.keys, self.values = self._alloc(self.capacity), self._alloc(self.capacity)
        self.is_initialized = True

    def _alloc(self, capacity):
        return torch.empty(self.batch, self.kv_heads, capacity, self.row_bytes, dtype=torch.uint8, device=self.device)

    def lazy_initialization(self, key_states, value_states):
        pass

    def update(self, key_states, value_states, *args, **kwargs):
        """Append the [B, Hkv, T, D] rows; returns them as they came -- the attention function reads the cache itself."""
        T = key_states.shape[2]
        if self.length + T > self.capacity:  # grow by doubling: a byte copy of the filled rows
            self.capacity = max(2 * self.capacity, (self.length + T + 3) // 4 * 4)
            old = (self.keys, self.values)
            self.keys, self.values = self._alloc(self.capacity), self._alloc(self.capacity)
            self.keys[:, :, :self.length].copy_(old[0][:, :, :self.length])
            self.values[:, :, :self.length].copy_(old[1][:, :, :self.length])
        ops.kv_append_q8_0(self.keys, self.values, key_states, value_states, self.length)
        self.length += T
        return key_states, value_states

    def decoded(self, dtype):
        """(K, V) [B, Hkv, length, D] in dtype: gq_dequantize_blocks of the filled rows"""
        def one(c):
            rows = c[:, :, :self.length].reshape(-1, self.row_bytes)
            return ops.dequantize_blocks(8, rows, dtype).view(self.batch, self.kv_heads, self.length, self.head_dim)
        return one(self.keys), one(self.values)

    def get_seq_length(self):
        return self.length

    def get_mask_sizes(self, query_length):
        return self.length + query_length, 0

    def get_max_length(self):
        return -1

    def reset(self):
        self.length = 0


class Q8KVCache(Cache):
    def __init__(self, config, batch, capacity, dtype=None, device=None, prefill="sdpa"):
        cfg = config.get_text_config()
        refuse_unsupported(cfg)
        if prefill not in PREFILLS:
            raise ValueError(f"Q8KVCache: prefill={prefill!r} (one of {PREFILLS})")
        self.prefill = prefill
        head_dim = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
        super().__init__(layers=[Q8Layer(batch, cfg.num_key_value_heads, head_dim, capacity, device)
                                 for _ in range(cfg.num_hidden_layers)])
        self.dtype, self.kv_start, self._max_start = dtype, None, 0

    def set_left_padding(self, attention_mask):
        """attention_mask [B, L] of a LEFT-padded prompt (zeros, then ones): positions below the first one are masked for
        every later step.  Read once, on the host."""
        first = attention_mask.shape[1] - attention_mask.to(torch.int64).sum(1)
        if not bool((attention_mask[:, -1] != 0).all()) or not bool((attention_mask[:, 1:] >= attention_mask[:, :-1]).all()):
            raise ValueError("Q8KVCache.set_left_padding: the mask is not left padding")
        self.kv_start = first.to(torch.int32).contiguous()
        self._max_start = int(first.max())

    def nbytes(self):
        return sum(l.keys.numel() + l.values.numel() for l in self.layers)


def refuse_unsupported(cfg):
    if getattr(cfg, "model_type", None) not in MODEL_TYPES:
        raise ValueError(f"Q8KVCache: model_type {getattr(cfg, 'model_type', None)!r} (one of {MODEL_TYPES}: LlamaAttention's forward)")
    sliding = any("sliding" in str(t) for t in (getattr(cfg, "layer_types", None) or ()))
    if sliding or (getattr(cfg, "sliding_window", None) and getattr(cfg, "use_sliding_window", True)):
        raise ValueError("Q8KVCache: sliding-window attention layers are not supported (sliding_window is set in the config)")


def _causal(T, S, device):  # query t at position S - T + t sees positions 0 .. S - T + t
    return torch.ones(T, S, dtype=torch.bool, device=device).tril(S - T)


def q8_kv_attention(module, query, key, value, attention_mask, dropout=0.0, scaling=None, **kwargs):
    """The attention function of a model with a Q8KVCache installed: (out [B, T, Hq, D], None)."""
    cache = module._gq_q8_cache
    layer = cache.layers[module.layer_idx]
    B, Hq, T, D = query.shape
    pos0, G = layer.length - T, Hq // layer.kv_heads  # (update() has appended this step's rows)
    scale = float(scaling if scaling is not None else D ** -0.5)
    if pos0 > 0 and G * T <= ops.ATTN_DECODE_MAX_COLS and (attention_mask is None or cache.kv_start is not None):
        if cache.kv_start is not None and cache._max_start > pos0:
            raise ValueError(f"Q8KVCache: left padding of {cache._max_start} positions exceeds the cache's {pos0}")
        return ops.attn_decode_q8_0(query, layer.keys, layer.values, pos0, scale, cache.kv_start), None
    if pos0 > 0 and cache.prefill == "q8_0" and (attention_mask is None or cache.kv_start is not None):
        return ops.attn_prefill_q8_0(query, layer.keys, layer.values, pos0, scale, cache.kv_start), None
    if pos0 > 0:
        key, value = layer.decoded(query.dtype)
    if attention_mask is None and T > 1:
        attention_mask = _causal(T, key.shape[2], query.device)
    if G > 1:
        key, value = key.repeat_interleave(G, 1), value.repeat_interleave(G, 1)
    out = torch.nn.functional.scaled_dot_product_attention(query, key, value, attn_mask=attention_mask, dropout_p=0.0, scale=scale)
    return out.transpose(1, 2).contiguous(), None


def _mask_none_when_causal(*args, attention_mask=None, allow_is_causal_skip=True, **kwargs):
    """The mask function of a cache with prefill="q8_0": sdpa_mask, but None for EVERY plain causal call without a padding
    mask -- sdpa_mask builds a 4-D mask for a chunk of tokens on a non-empty cache, and a 4-D mask is a general one here.  The
    kernels apply the causal mask themselves, and the fallback builds its own when it is given none."""
    if attention_mask is None and allow_is_causal_skip:
        return None
    return sdpa_mask(*args, attention_mask=attention_mask, allow_is_causal_skip=allow_is_causal_skip, **kwargs)


def install(model, cache):
    """Point the model at the Q8_0 attention for the time `cache` is in use; restore(model) undoes it."""
    if hasattr(model, "_gq_q8_prev_attn"):
        raise RuntimeError("Q8KVCache: install() on a model that has a cache installed; restore(model) first")
    refuse_unsupported(model.config.get_text_config())
    AttentionInterface.register(ATTN_NAME, q8_kv_attention)
    AttentionMaskInterface.register(ATTN_NAME, _mask_none_when_causal if cache.prefill == "q8_0" else sdpa_mask)
    model._gq_q8_prev_attn = model.config._attn_implementation
    model.config._attn_implementation = ATTN_NAME
    for m in model.modules():
        if hasattr(m, "layer_idx") and hasattr(m, "q_proj"):
            m._gq_q8_cache = cache
    return cache


def restore(model):
    model.config._attn_implementation = model._gq_q8_prev_attn
    del model._gq_q8_prev_attn
    for m in model.modules():
        if hasattr(m, "_gq_q8_cache"):
            del m._gq_q8_cache
