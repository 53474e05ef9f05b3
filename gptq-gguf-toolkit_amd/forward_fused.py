"""HIP kernels for the elementwise part of the calibration forward.

The reference runs every decoder layer through the HF eager modules (reference quantizer.py:293
`block(inp_batch, **kwargs)`); on an MI355X that forward is 60 % of a whole-model run and a third of
it is 2-8 torch elementwise kernels per RMSNorm / rotary embedding / SwiGLU.  `fused_forward()` replaces exactly
those three with one gfx950 kernel each (csrc/gq_forward.hip) for the duration of a `with` block:

    LlamaRMSNorm.forward       -> ops.fwd_rmsnorm   (fp32 statistics, rounded to the dtype where the module rounds)
    apply_rotary_pos_emb       -> ops.fwd_rope      (per-op rounding of the eager expression)
    LlamaMLP.forward           -> down_proj(ops.fwd_silu_mul(gate_proj(x), up_proj(x)))
    Qwen3Attention.forward     -> q_norm, k_norm and the rotary embedding of both through ONE ops.fwd_qk_norm_rope
                                  (csrc/forward/gq_qk_norm_rope.hip; the per-head norms are 64 .. 256 wide, which the
                                  RMSNorm kernels above do not take, so without it they are HF eager code)

The Linear modules are still called through `nn.Module.__call__`, so the Hessian hooks see the same inputs.  Two guards
(ADVICE r03): (1) the kernels were written for ONE definition of each function -- `_PINNED` holds the hashes of the
normalised source of LlamaRMSNorm.forward, apply_rotary_pos_emb (+ rotate_half) and LlamaMLP.forward they implement; if the
installed transformers' Llama differs (a `pretraining_tp` branch, a new keyword, ...) that function is NOT patched, and a
model family is patched only when its module text equals the pinned Llama text (Mistral, Qwen2 ... copy it verbatim);
(2) every kernel is trusted for a (shape class, dtype) only after it has reproduced the eager expression bit for bit on
the first real input of that class -- RMSNorm (output + the fp32 statistics), the rotary embedding and SwiGLU alike; a
mismatch leaves the eager code in place for that class.  Every patched function also falls back to the original for inputs
the kernels do not take (fp32, non-contiguous, odd sizes, CPU tensors, unknown keywords) -- the originals are torch code,
not a CPU restatement of ours.  Levels (`level_of`): "exact"
-- the Quantizer's default -- installs only kernels that are bit-identical to HF eager: the rotary embedding and SwiGLU
(tests/test_gpu_forward.py: torch.equal, every finite 16-bit gate value included), and RMSNorm through
gq_fwd_rmsnorm_ordered, which sums mean(x^2) in the order of ATen's reduce kernel and rounds rsqrt the way torch.rsqrt
does -- trusted only after it has reproduced the eager module bit for bit on the first real input of each
(hidden size, dtype); a Quantizer run at this level saves the same bytes as one on plain HF eager.  "all" also uses
the free-order RMSNorm kernel (<= 2 ulp on < 0.1 % of the elements) where the ordered one is not verified; "off"
patches nothing.
"""
from __future__ import annotations

import contextlib
import hashlib
import importlib
import inspect
import warnings
from typing import List, Tuple

import torch

from . import ops

_FAMILIES = ("llama", "mistral", "qwen2", "qwen3", "mixtral", "gemma")  # candidates; each is checked against Llama's text
_16BIT = (torch.float16, torch.bfloat16)


def _body(fn) -> str:
    """Source of a function without its signature's class name / decorators / docstring, whitespace-normalised."""
    src = inspect.getsource(fn)
    lines = [ln.strip() for ln in src.splitlines()]
    lines = [ln for ln in lines if ln and not ln.startswith("@") and not ln.startswith("#")]
    text = "\n".join(lines)
    doc = inspect.getdoc(fn)
    if doc:
        start, end = text.find('"""'), text.find('"""', text.find('"""') + 3)
        if start >= 0 and end > start:
            text = text[:start] + text[end + 3:]
    return "\n".join(ln for ln in text.splitlines() if ln.strip())


def _sha(fn) -> str:
    return hashlib.sha256(_body(fn).encode()).hexdigest()[:16]


# The semantics csrc/gq_forward.hip implements, as sha256[:16] of `_body(fn)` of transformers' Llama (5.x):
#   LlamaRMSNorm.forward:  x32 = x.float(); var = x32.pow(2).mean(-1, keepdim=True); x32 = x32 * rsqrt(var + eps);
#                          return weight * x32.to(input dtype)
#   apply_rotary_pos_emb:  (q * cos) + (rotate_half(q) * sin), same for k, cos / sin unsqueezed at unsqueeze_dim
#   rotate_half:           cat((-x[..., D/2:], x[..., :D/2]), -1)
#   LlamaMLP.forward:      down_proj(act_fn(gate_proj(x)) * up_proj(x))
#   Qwen3Attention.forward (transformers' Qwen3, 5.x): q_norm(q_proj(x).view(B, L, -1, D)).transpose(1, 2), the same for
#                          k with k_norm, v without a norm; apply_rotary_pos_emb(q, k, cos, sin); the cache update; the
#                          attention interface; o_proj -- Qwen3RMSNorm.forward being LlamaRMSNorm.forward's text
_PINNED = {"norm": "3480f6ca9ea40b53", "rope": "d2c323856b661430", "rotate_half": "e011a50957282b58", "mlp": "1923407024d5de0b",
           "qwen3_attn": "d7e568784937795f"}
QK_NORM_HEAD_DIMS = (64, 128, 256)  # include/gptq_gguf_qknorm.h

_norm_verdict = {}  # (C, dtype, rows) -> True: the ordered kernel reproduced the eager module bit for bit on first use
_rope_verdict = {}  # (L, heads q, heads k, D, dtype, batch) -> True: fwd_rope == the eager expression on first use
_mlp_verdict = {}   # (intermediate size, dtype, rows) -> True: fwd_silu_mul == act_fn(g) * u on first use
_qkn_verdict = {}   # _qkn_key(...) -> True: fwd_qk_norm_rope == q_norm / k_norm / apply_rotary_pos_emb (outputs and statistics)


def reset_verdicts():
    """Forget what has been verified (the Quantizer calls this at the start of a run: every run re-checks cheaply)."""
    _norm_verdict.clear()
    _rope_verdict.clear()
    _mlp_verdict.clear()
    _qkn_verdict.clear()


def _rmsnorm_forward(orig, allow_free_order: bool):
    """LlamaRMSNorm.forward through gq_fwd_rmsnorm_ordered -- mean(x^2) summed in ATen's order, torch.rsqrt's rounding --
    once that kernel has reproduced the eager module BIT FOR BIT on the first real input of its (hidden size, dtype):
    the output and, row by row, the fp32 mean and rsqrt themselves (a different summation order shows in about half
    of the rows' means, while the 16-bit outputs would hide most of it).  Not verified (another
    PyTorch build, an unusual shape): the eager module stays -- or, with allow_free_order (level "all"), the
    free-order kernel (<= 2 ulp)."""
    def forward(self, hidden_states):
        w = self.weight
        x = hidden_states
        if not (x.is_cuda and x.dtype in _16BIT and w.dtype == x.dtype and x.is_contiguous() and w.is_contiguous()
                and x.numel() > 0 and not torch.is_grad_enabled()):
            return orig(self, x)
        C = x.shape[-1]
        # ATen's reduce configuration depends on the number of rows as well as on C: every (C, dtype, rows) is verified
        key = (C, x.dtype, x.numel() // C)
        if C % 512 == 0 and x.numel() // C >= 8:
            ok = _norm_verdict.get(key)
            if ok is None:
                # the outputs (rounded to 16 bits) would hide most order differences: the statistics themselves must agree,
                # row by row, with what torch computes for the module's own expression
                want = orig(self, x)
                got, stats = ops.fwd_rmsnorm_ordered(x, w, self.variance_epsilon, want_stats=True)
                var = x.to(torch.float32).pow(2).mean(-1, keepdim=True)
                r = torch.rsqrt(var + self.variance_epsilon)
                _norm_verdict[key] = bool(torch.equal(want, got) and torch.equal(stats[:, 0], var.reshape(-1))
                                          and torch.equal(stats[:, 1], r.reshape(-1)))
                return want
            if ok:
                return ops.fwd_rmsnorm_ordered(x, w, self.variance_epsilon)
        if allow_free_order and C % 8 == 0:
            return ops.fwd_rmsnorm(x, w, self.variance_epsilon)
        return orig(self, x)
    return forward


def _rope(orig):
    def apply_rotary_pos_emb(q, k, cos, sin, *args, **kwargs):
        # anything but the pinned signature (q, k, cos, sin, unsqueeze_dim=1) goes to the original untouched
        if len(args) > 1 or (kwargs and set(kwargs) != {"unsqueeze_dim"}) or (args and kwargs):
            return orig(q, k, cos, sin, *args, **kwargs)
        unsqueeze_dim = args[0] if args else kwargs.get("unsqueeze_dim", 1)
        ok = (unsqueeze_dim == 1 and q.is_cuda and q.dim() == 4 and k.dim() == 4 and cos.dim() == 3 and q.dtype in _16BIT
              and k.dtype == q.dtype == cos.dtype == sin.dtype and q.shape[-1] % 16 == 0 and q.numel() > 0
              and not torch.is_grad_enabled())
        if ok:
            qt, kt = q.transpose(1, 2), k.transpose(1, 2)  # [B, L, H, D]: the projections' own memory layout
            B, L, _, D = qt.shape
            ok = (qt.is_contiguous() and kt.is_contiguous() and cos.shape[-1] == D and cos.shape[1] == L
                  and cos.shape == sin.shape and cos.shape[0] in (1, B))
        if not ok:
            return orig(q, k, cos, sin, unsqueeze_dim)
        key = (L, qt.shape[2], kt.shape[2], D, q.dtype, B)
        verdict = _rope_verdict.get(key)
        if verdict is False:
            return orig(q, k, cos, sin, unsqueeze_dim)
        c, s_ = cos, sin
        if c.shape[0] != B:
            c, s_ = c.expand(B, L, D), s_.expand(B, L, D)
        c, s_ = c.contiguous(), s_.contiguous()
        got = ops.fwd_rope(qt, c, s_).transpose(1, 2), ops.fwd_rope(kt, c, s_).transpose(1, 2)
        if verdict is None:  # first input of this class: the eager expression decides, and is what is returned
            want = orig(q, k, cos, sin, unsqueeze_dim)
            _rope_verdict[key] = bool(torch.equal(want[0], got[0]) and torch.equal(want[1], got[1]))
            return want
        return got
    return apply_rotary_pos_emb


def _mlp_forward(orig):
    def forward(self, x):
        act = self.act_fn
        if (x.is_cuda and x.dtype in _16BIT and not torch.is_grad_enabled()
                and (isinstance(act, torch.nn.SiLU) or type(act).__name__ == "SiLUActivation")):
            # the three Linears are entered exactly once each, through nn.Module.__call__: the Hessian hooks see every
            # input once whether or not the kernel is trusted yet
            g, u = self.gate_proj(x), self.up_proj(x)
            if g.is_contiguous() and u.is_contiguous() and g.numel() % 8 == 0 and g.numel() > 0:
                key = (g.shape[-1], g.dtype, g.numel() // g.shape[-1])
                verdict = _mlp_verdict.get(key)
                if verdict:
                    return self.down_proj(ops.fwd_silu_mul(g, u))
                want = act(g) * u
                if verdict is None:
                    _mlp_verdict[key] = bool(torch.equal(want, ops.fwd_silu_mul(g, u)))
                return self.down_proj(want)
            return self.down_proj(act(g) * u)
        return orig(self, x)
    return forward


def _qkn_key(B, L, Hq, Hk, D, dtype):
    """The class of inputs one verdict of the fused q / k norm + rotary kernel covers.  ATen's summation order at these row
    lengths was measured NOT to depend on the number of rows (profiles/qk_norm_order_probe.py), unlike at
    the wide rows of _rmsnorm_forward; the sizes stay in the key all the same -- they are what the eager rotary expression
    and the kernel's lane arithmetic see, and a re-check per shape costs one forward's worth of eager code."""
    return (B, L, Hq, Hk, D, dtype)


def _qwen3_attention_forward(orig, mod):
    """Qwen3Attention.forward with q_norm, k_norm and apply_rotary_pos_emb through ops.fwd_qk_norm_rope.  `mod` is the
    modelling module: its apply_rotary_pos_emb, attention registry and eager attention are looked up at call time, as the
    original's globals are.  Everything but the three replaced calls is the original's text."""
    def forward(self, hidden_states, position_embeddings, attention_mask, past_key_values=None, **kwargs):
        x = hidden_states
        D = getattr(self, "head_dim", None)
        qn, kn = getattr(self, "q_norm", None), getattr(self, "k_norm", None)
        ok = (past_key_values is None and torch.is_tensor(x) and x.is_cuda and x.dtype in _16BIT and x.dim() == 3
              and x.numel() > 0 and not torch.is_grad_enabled() and D in QK_NORM_HEAD_DIMS
              and isinstance(position_embeddings, (tuple, list)) and len(position_embeddings) == 2
              and type(qn) is mod.Qwen3RMSNorm and type(kn) is mod.Qwen3RMSNorm
              and qn.variance_epsilon == kn.variance_epsilon and qn.weight.dtype == kn.weight.dtype == x.dtype
              and qn.weight.shape == kn.weight.shape == (D,))
        if ok:
            cos, sin = position_embeddings
            B, L = x.shape[:2]
            ok = (torch.is_tensor(cos) and torch.is_tensor(sin) and cos.dim() == 3 and cos.shape == sin.shape
                  and cos.dtype == sin.dtype == x.dtype and cos.shape[1] == L and cos.shape[2] == D and cos.shape[0] in (1, B))
        if not ok:
            return orig(self, hidden_states, position_embeddings, attention_mask, past_key_values, **kwargs)
        input_shape = x.shape[:-1]
        hidden_shape = (*input_shape, -1, D)
        # the four Linears are entered exactly once each, through nn.Module.__call__, in the original's order: the Hessian
        # hooks see every input once whether or not the kernel is trusted
        q4, k4 = self.q_proj(x).view(hidden_shape), self.k_proj(x).view(hidden_shape)
        value_states = self.v_proj(x).view(hidden_shape).transpose(1, 2)
        key = _qkn_key(B, L, q4.shape[2], k4.shape[2], D, x.dtype)
        verdict = _qkn_verdict.get(key) if q4.is_contiguous() and k4.is_contiguous() else False
        got = None
        if verdict is not False:
            c, s_ = cos, sin
            if c.shape[0] != B:
                c, s_ = c.expand(B, L, D), s_.expand(B, L, D)
            got = ops.fwd_qk_norm_rope(q4, k4, qn.weight.contiguous(), kn.weight.contiguous(), c.contiguous(), s_.contiguous(),
                                       qn.variance_epsilon, want_stats=verdict is None)
        if verdict:
            query_states, key_states = got[0].transpose(1, 2), got[1].transpose(1, 2)
        else:  # the eager expressions: what is returned until the kernel has reproduced them on this class, and if it has not
            query_states, key_states = mod.apply_rotary_pos_emb(qn(q4).transpose(1, 2), kn(k4).transpose(1, 2), cos, sin)
            if verdict is None:
                # 16-bit outputs hide most differences of the summation order: the fp32 statistics must agree row by row too
                var = torch.cat([q4.to(torch.float32).pow(2).mean(-1).reshape(-1), k4.to(torch.float32).pow(2).mean(-1).reshape(-1)])
                r = torch.rsqrt(var + qn.variance_epsilon)
                _qkn_verdict[key] = bool(torch.equal(query_states, got[0].transpose(1, 2)) and torch.equal(key_states, got[1].transpose(1, 2))
                                         and torch.equal(got[2][:, 0], var) and torch.equal(got[2][:, 1], r))
        attention_interface = mod.ALL_ATTENTION_FUNCTIONS.get_interface(self.config._attn_implementation, mod.eager_attention_forward)
        attn_output, attn_weights = attention_interface(
            self, query_states, key_states, value_states, attention_mask,
            dropout=0.0 if not self.training else self.attention_dropout, scaling=self.scaling,
            sliding_window=self.sliding_window, **kwargs)
        attn_output = attn_output.reshape(*input_shape, -1).contiguous()
        return self.o_proj(attn_output), attn_weights
    return forward


def _targets(free_order_norm: bool = True, qk_norm_rope: bool = True) -> List[Tuple[object, str, object]]:
    """(owner, attribute, replacement) for every installed family whose module text equals Llama's.  free_order_norm:
    RMSNorm may fall back to the free-order kernel where the ordered one is not verified (level "all")."""
    from transformers.models.llama import modeling_llama as ref
    # what the installed Llama computes must be what the kernels were written for; a function whose text moved is left
    # to the eager code (for every family), loudly
    have = {"norm": (ref.LlamaRMSNorm.forward,), "rope": (ref.apply_rotary_pos_emb,), "rotate_half": (ref.rotate_half,),
            "mlp": (ref.LlamaMLP.forward,)}
    pinned = {}
    for k, (fn,) in have.items():
        try:
            pinned[k] = _sha(fn) == _PINNED[k]
        except (OSError, TypeError):
            pinned[k] = False
    pinned["rope"] = pinned["rope"] and pinned["rotate_half"]
    moved = [k for k in ("norm", "rope", "mlp") if not pinned[k]]
    if moved:
        warnings.warn(f"forward_fused: transformers' Llama {moved} differ from the definitions the HIP kernels implement; "
                      "these stay on HF eager code", RuntimeWarning)
    want_norm = _body(ref.LlamaRMSNorm.forward) if pinned["norm"] else None
    want_rope = _body(ref.apply_rotary_pos_emb) if pinned["rope"] else None
    want_mlp = _body(ref.LlamaMLP.forward) if pinned["mlp"] else None
    out = []
    for fam in _FAMILIES:
        try:
            mod = importlib.import_module(f"transformers.models.{fam}.modeling_{fam}")
        except Exception:
            continue
        for name, cls in vars(mod).items():
            if not inspect.isclass(cls) or getattr(cls, "__module__", None) != mod.__name__:
                continue
            try:
                if want_norm and name.endswith("RMSNorm") and _body(cls.forward) == want_norm:
                    out.append((cls, "forward", _rmsnorm_forward(cls.forward, free_order_norm)))
                elif want_mlp and name.endswith("MLP") and _body(cls.forward) == want_mlp:
                    out.append((cls, "forward", _mlp_forward(cls.forward)))
            except (OSError, TypeError):
                continue
        fn = vars(mod).get("apply_rotary_pos_emb")
        try:
            rh = vars(mod).get("rotate_half")
            if (want_rope and fn is not None and getattr(fn, "__module__", None) == mod.__name__ and _body(fn) == want_rope
                    and rh is not None and _sha(rh) == _PINNED["rotate_half"]):
                out.append((mod, "apply_rotary_pos_emb", _rope(fn)))
        except (OSError, TypeError):
            pass
        attn = vars(mod).get("Qwen3Attention") if fam == "qwen3" else None
        if qk_norm_rope and attn is not None:
            # the fused kernel is ONE definition of the norm, the rotary embedding and the attention forward around them:
            # all three texts of this module must be the pinned ones
            try:
                same = (_sha(attn.forward) == _PINNED["qwen3_attn"] and want_norm is not None and want_rope is not None
                        and _body(mod.Qwen3RMSNorm.forward) == want_norm and _body(mod.apply_rotary_pos_emb) == want_rope
                        and _sha(mod.rotate_half) == _PINNED["rotate_half"])
            except (OSError, TypeError, AttributeError):
                same = False
            if same:
                out.append((attn, "forward", _qwen3_attention_forward(attn.forward, mod)))
            else:
                warnings.warn("forward_fused: transformers' Qwen3 ['attention'] differ from the definitions the HIP kernels "
                              "implement; these stay on HF eager code", RuntimeWarning)
    return out


# Level "exact" installs the fused q / k norm + rotary kernel: it is bit-identical or not used, and it was measured not to be
# slower than the two eager Qwen3RMSNorm + two fwd_rope launches it replaces at any of the three points of
# profiles/qk_norm_rope_rate.txt (0.26 - 0.34 of their time).  False keeps it behind "all" only.
QK_NORM_ROPE_IN_EXACT = True


def level_of(flag) -> str:
    """Normalise the Quantizer's `fused_forward` argument: "off" (False / None / "off" / "0"), "exact" (bit-exact
    kernels only: rotary embedding, SwiGLU, and RMSNorm once verified on this PyTorch) or "all" (True / "all" / "1":
    RMSNorm through the free-order kernel, <= 2 ulp, wherever the exact one is not verified)."""
    if flag is None or flag is False:
        return "off"
    if flag is True:
        return "all"
    f = str(flag).lower()
    if f in ("off", "0", "false", "no", "none", ""):
        return "off"
    if f in ("all", "1", "true", "yes"):
        return "all"
    if f == "exact":
        return "exact"
    raise ValueError(f"fused_forward={flag!r}: expected off / exact / all")


@contextlib.contextmanager
def fused_forward(enabled=True):
    """Within the block, the matching HF modules run the gfx950 kernels (`enabled`: see level_of).  Raises (does not
    fall back) if the HIP library is missing; restores the originals on exit."""
    level = level_of(enabled)
    if level == "off":
        yield []
        return
    ops.lib()  # fail loudly here, not in the middle of a forward
    saved = []
    try:
        for owner, attr, new in _targets(free_order_norm=(level == "all"), qk_norm_rope=(level == "all" or QK_NORM_ROPE_IN_EXACT)):
            saved.append((owner, attr, vars(owner)[attr] if attr in vars(owner) else getattr(owner, attr)))
            setattr(owner, attr, new)
        yield [f"{getattr(o, '__name__', o)}.{a}" for o, a, _ in saved]
    finally:
        for owner, attr, old in reversed(saved):
            setattr(owner, attr, old)
