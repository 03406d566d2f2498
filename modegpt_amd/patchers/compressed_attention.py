"""Attention of a compressed model.

A compressed layer keeps r_qk <= head_dim columns of every q/k head (chosen per kv head, in RoPE pairs, order given by
the layer's rotary mask) and r_vo columns of every v/o head.  The stock HF attention modules assume `head_dim`
everywhere, so the reference ships forked copies of the HF modeling files with the checkpoint
(src/patchers/*Rebuild.py, loaded through config.auto_map).  This engine does not fork the modeling files: it keeps the
stock HF modules and gives their attention the compressed semantics, with the elementwise chain in one HIP kernel:

  * q/k/v are viewed with their own per-layer head widths                        (LlamaRebuild.py:320-326)
  * RoPE: cos/sin are gathered along the feature axis by the rotary mask, per kv head, query heads of a group share
    their kv head's mask; rotate_half pairs the two halves of the KEPT columns   (LlamaRebuild.py:153-176)
    -> modegpt_amd.ops.rope_gather (csrc/rope.hip), which also writes the [B, heads, T, r] layout attention reads
  * Qwen3: q_norm / k_norm normalise over the kept columns with the norm weight gathered by the same mask
    (DenseQwenRebuild.py:262-286) -> fused into the same kernel
  * softmax scale = (compressed q/k head width) ** -0.5                          (LlamaRebuild.py:266,282)
  * OPT: no RoPE, no mask; q is pre-scaled by the compressed width, attention runs with scale 1  (OPTRebuild.py:144-163)
  * the attention product itself goes through HF's attention interface exactly as in the stock modules
    (config._attn_implementation: sdpa / eager / ...) -- PyTorch plumbing, not part of this engine -- unless
    MODEGPT_FUSED_ATTN=1: then a call without a mask, a sliding window or requested weights (the condition under which HF's own
    sdpa path asks for is_causal) runs modegpt_amd.ops.attn_fwd (csrc/attn.hip), a flash-style kernel that takes r_qk != r_vo
    as they are and writes the token-major rows o_proj reads.  Which one served is counted in ATTN_CALLS.  Off by default.
    MODEGPT_FUSED_ATTN_DECODE=1 beside it (no effect alone) sends those of these calls whose queries of one kv head fit one MFMA
    tile -- T * (n_heads / n_kv) <= 32: decode steps, short chunks -- to modegpt_amd.ops.attn_decode (csrc/attn_decode.hip), the
    same product split over the keys so that a small batch fills the device.  Which kernel served is counted in ATTN_KERNELS.
    MODEGPT_FUSED_ATTN_MASK=1 beside MODEGPT_FUSED_ATTN=1 (no effect alone) also serves the calls that come WITH a mask, when it is
    the bool [B or 1, 1 or n_heads, T, S] tensor with a unit last stride that Transformers builds for a padded batch
    (masking_utils.sdpa_mask: the causal rule ANDed with the padding columns, expanded): batched generate with left padding,
    batched evaluation, serving loops.  The kernels take the mask as it is (causal=False: the mask alone decides), nothing is
    inspected and nothing syncs; such calls are also counted in ATTN_MASKED.  Any other mask (additive float, another rank, strided
    keys) and modules with a sliding window stay on the interface.

Two entry points share the forward functions:
  install_compressed_attention(adapter, rotary_masks)   live model right after ModelAdapter.convert_model
  shrink_to_config_ranks(model, arch)                   called by the modeling files shipped with a checkpoint
                                                         (patchers/{LlamaRebuild,DenseQwenRebuild,Qwen2Rebuild,OPTRebuild}.py)

This file travels WITH a compressed checkpoint (model_utils.save_compressed_model copies it next to the *Rebuild.py that
imports it relatively), the way the reference ships its self-contained modeling file (src/model_utils.py:103-124): it
depends on torch and transformers only.  The fused HIP kernel is used when the modegpt_amd package is importable and the
tensors live on a GPU; anywhere else (another machine, a CPU) the same chain runs as plain torch ops, the reference's own
expression op for op -- the checkpoint loads and evaluates wherever the reference's would.  Which path ran is counted in
PATH_CALLS; MODEGPT_REQUIRE_HIP=1 turns the torch path into an error.  One case raises by itself: the engine is installed here but
its library does not load (a broken installation) and the tensors are on a GPU -- unless MODEGPT_ALLOW_TORCH=1.

Inference only: the kernel has no backward.
"""
from __future__ import annotations

import logging
import os
import types
from typing import List, Optional

import torch
import torch.nn as nn

logger = logging.getLogger("MoDeGPT")
PATH_CALLS = {"hip": 0, "torch": 0}     # rope/norm chains served by mdg_rope_gather / by the torch expression
ATTN_CALLS = {"hip": 0, "interface": 0}  # attention products served by the engine's kernels / by HF's attention interface
ATTN_KERNELS = {"fwd": 0, "decode": 0}  # of the "hip" ones: served by mdg_attn_fwd / by mdg_attn_decode (MODEGPT_FUSED_ATTN_DECODE=1)
ATTN_MASKED = {"fwd": 0, "decode": 0}   # of those again: called with a bool mask (MODEGPT_FUSED_ATTN_MASK=1), per kernel
_DECODE_SPLITS = None                   # an int overrides mdg_attn_decode_splits (tests and tuning; not an environment knob)
_HIP_OPS = None
_HIP_BROKEN = None                      # why the engine, although installed here, cannot serve (its library failed to load)


def _hip_ops():
    """modegpt_amd.ops when this process can import the engine AND its library loads, else None -- decided once.  Two different
    reasons for None: the package is simply not on this machine (a checkpoint taken elsewhere: the portable torch path, with one
    warning), or it is here and libmodegpt_hip.so does not load (a broken installation: _HIP_BROKEN holds the reason and GPU
    tensors raise instead of quietly running ten eager passes per layer)."""
    global _HIP_OPS, _HIP_BROKEN
    if _HIP_OPS is None:
        try:
            import modegpt_amd  # noqa: F401
        except Exception as exc:  # not installed here: the portable path
            _HIP_OPS = False
            logger.warning("compressed attention: modegpt_amd is not importable (%s); running the reference's torch expression", exc)
            return None
        try:
            from modegpt_amd import _lib, ops as _ops
            if torch.cuda.is_available():
                _lib.load()
            _HIP_OPS = _ops
        except Exception as exc:
            _HIP_OPS = False
            _HIP_BROKEN = f"{type(exc).__name__}: {exc}"
    return _HIP_OPS or None


def _rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def _rope_gather_torch(x, cos, sin, mask, n_heads, n_kv, norm_weight=None, eps=1e-6):
    """The reference's chain in torch (LlamaRebuild.py:153-186, DenseQwenRebuild.py:262-286): x [B, T, n_heads * r] ->
    optional masked RMSNorm over the r kept columns (fp32, weight gathered by the mask) -> [B, n_heads, T, r] ->
    x * cos[mask] + rotate_half(x) * sin[mask], every op rounded to the tensor dtype as eager torch does."""
    B, T, width = x.shape
    r = width // n_heads
    x = x.view(B, T, n_heads, r)
    m = None
    if mask is not None:
        m = mask.to(x.device)
        if n_heads != n_kv:
            m = torch.repeat_interleave(m, n_heads // n_kv, dim=0)         # query heads share their kv head's row
    if norm_weight is not None:
        xf = x.to(torch.float32)
        normed = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
        x = (norm_weight[m][None, None] * normed).to(x.dtype)
    x = x.transpose(1, 2)                                                  # [B, n_heads, T, r]
    if m is None:
        c, s = cos.unsqueeze(1), sin.unsqueeze(1)
    else:                                                                  # [1, T, H, r] -> [1, H, T, r]
        c, s = cos[:1, :, m].permute(0, 2, 1, 3), sin[:1, :, m].permute(0, 2, 1, 3)
    return x * c + _rotate_half(x) * s


def _rope_gather(x, cos, sin, mask, n_heads, n_kv, head_dim, norm_weight=None, eps=1e-6):
    hip = _hip_ops() if x.is_cuda else None
    if hip is not None:
        PATH_CALLS["hip"] += 1
        return hip.rope_gather(x, cos, sin, mask, n_heads, n_kv, head_dim, norm_weight=norm_weight, eps=eps)
    if os.environ.get("MODEGPT_REQUIRE_HIP", "0") == "1":
        raise RuntimeError("compressed attention: MODEGPT_REQUIRE_HIP=1 but the HIP kernel cannot serve this call "
                           f"(tensor on {x.device}, modegpt_amd importable: {_hip_ops() is not None})")
    if x.is_cuda and _HIP_BROKEN and os.environ.get("MODEGPT_ALLOW_TORCH", "0") != "1":
        # the engine IS installed here and its library does not load: a broken installation on a GPU box, not portability -- say so.
        # (A machine without the engine -- a CUDA box, lm-eval -- takes the portable torch path below with the one warning of
        # _hip_ops, as the reference's self-contained checkpoints do; MODEGPT_REQUIRE_HIP=1 is the strict opt-in.)
        raise RuntimeError("compressed attention: modegpt_amd is installed but libmodegpt_hip.so cannot be used in this process "
                           f"({_HIP_BROKEN}), so mdg_rope_gather is unavailable for these GPU tensors.  Rebuild the engine, or set "
                           "MODEGPT_ALLOW_TORCH=1 to run the reference's torch expression on the GPU instead.")
    PATH_CALLS["torch"] += 1
    return _rope_gather_torch(x, cos.to(x.dtype), sin.to(x.dtype), mask, n_heads, n_kv,
                              None if norm_weight is None else norm_weight.detach().to(x.dtype), eps)


def _attention_interface(module):
    """HF's dispatch on config._attn_implementation, falling back to the model family's eager function."""
    import importlib

    from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS
    eager = importlib.import_module(type(module).__module__).eager_attention_forward
    impl = getattr(module.config, "_attn_implementation", "eager") or "eager"
    if hasattr(ALL_ATTENTION_FUNCTIONS, "get_interface"):
        return ALL_ATTENTION_FUNCTIONS.get_interface(impl, eager)
    return eager if impl == "eager" else ALL_ATTENTION_FUNCTIONS[impl]


def _attend(self, q, k, v, attention_mask, scaling, kwargs, extra=None, want_weights=False):
    """The attention product of both forwards: q [B, n_h, T, r_qk], k [B, n_kv, S, r_qk], v [B, n_kv, S, r_vo] -> (rows for
    o_proj [B, T, n_h * r_vo], weights).  MODEGPT_FUSED_ATTN=1 sends a call that needs no mask tensor to mdg_attn_fwd: no
    attention_mask (with one, HF's interface serves the call as it always did: nothing is inspected, nothing syncs), the module
    causal, no sliding window, no weights requested, no gradients, bf16 / f16 on a GPU with the engine's library loaded.  Query i
    then sees the keys j <= i + (S - T): prefill, and decode with a cache.  With MODEGPT_FUSED_ATTN_DECODE=1 as well, those of these
    calls with T * (n_h / n_kv) <= 32 run mdg_attn_decode, the split-key schedule.  With MODEGPT_REQUIRE_HIP=1 as well, a call that meets
    the conditions but cannot be served by the kernel (the engine's library does not load, a width outside the kernel's range, a
    strided last dimension) raises instead of taking the interface.  MODEGPT_FUSED_ATTN_MASK=1 as well: a call with an
    attention_mask is served too when the mask is a bool [B or 1, 1 or n_h, T, S] tensor on q's device with a unit last stride --
    decided from dtype, shape and strides alone -- by the masked entries with causal=False; with MODEGPT_REQUIRE_HIP=1 any other
    mask raises with the reason."""
    B, T = q.shape[0], q.shape[2]
    if os.environ.get("MODEGPT_FUSED_ATTN", "0") == "1":
        mask = None
        why_mask = None
        if attention_mask is not None and os.environ.get("MODEGPT_FUSED_ATTN_MASK", "0") == "1":
            am = attention_mask
            if not isinstance(am, torch.Tensor) or am.dtype != torch.bool:
                why_mask = f"a mask that is not a torch.bool tensor ({getattr(am, 'dtype', type(am))}; additive masks are out of scope)"
            elif am.dim() != 4 or am.shape[0] not in (1, B) or am.shape[1] not in (1, q.shape[1]) or tuple(am.shape[2:]) != (T, k.shape[2]):
                why_mask = f"a mask of shape {tuple(am.shape)}, not [B or 1, 1 or n_heads, T={T}, S={k.shape[2]}]"
            elif am.device != q.device:
                why_mask = f"a mask on {am.device}"
            elif (am.shape[3] > 1 and am.stride(3) != 1) or any(am.stride(d) < 0 for d in range(3)):
                why_mask = f"a mask with strides {am.stride()} (the keys must be contiguous)"
            else:
                mask = am
        eligible = ((attention_mask is None or mask is not None or why_mask is not None)
                    and getattr(self, "is_causal", True) is not False
                    and getattr(self, "sliding_window", None) is None
                    and not (want_weights or kwargs.get("output_attentions", False))
                    and not (torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad))
                    and q.is_cuda and q.dtype in (torch.bfloat16, torch.float16))
        if eligible:
            why = None
            if _hip_ops() is None:
                why = f"modegpt_amd cannot serve ({_HIP_BROKEN or 'not importable'})"
            elif q.shape[-1] % 2 or q.shape[-1] > 256 or v.shape[-1] > 256:
                why = f"head widths r_qk={q.shape[-1]} (even, <= 256), r_vo={v.shape[-1]} (<= 256)"
            elif k.stride(-1) != 1 or v.stride(-1) != 1:
                why = "k / v without a contiguous last dimension"
            elif why_mask is not None:
                why = why_mask
            if why is None:
                ATTN_CALLS["hip"] += 1
                n_h, n_kv = q.shape[1], k.shape[1]
                ops = _hip_ops()
                decode = (os.environ.get("MODEGPT_FUSED_ATTN_DECODE", "0") == "1" and n_h % n_kv == 0
                          and T * (n_h // n_kv) <= ops.ATTN_DECODE_COLUMNS)
                kernel = "decode" if decode else "fwd"
                ATTN_KERNELS[kernel] += 1
                if mask is not None:
                    ATTN_MASKED[kernel] += 1
                fn, own = (ops.attn_decode, {"splits": _DECODE_SPLITS}) if decode else (ops.attn_fwd, {})
                # with a mask the mask alone decides: it carries the causal rule
                out = fn(q, k, v, float(scaling), causal=mask is None, mask=mask, **own)   # [B, T, n_h, r_vo]
                return out.view(B, T, -1), None
            if os.environ.get("MODEGPT_REQUIRE_HIP", "0") == "1":
                raise RuntimeError("compressed attention: MODEGPT_FUSED_ATTN=1 and MODEGPT_REQUIRE_HIP=1 but mdg_attn_fwd cannot "
                                   f"serve this call: {why}")
    ATTN_CALLS["interface"] += 1
    out, weights = _attention_interface(self)(self, q, k, v, attention_mask, dropout=0.0, scaling=scaling, **(extra or {}), **kwargs)
    return out.reshape(B, T, -1).contiguous(), weights


def _rope_forward(self, hidden_states, position_embeddings=None, attention_mask=None, past_key_values=None, **kwargs):
    """Llama / Qwen2 / Qwen3 (RoPE, optional GQA, optional per-head q/k RMSNorm; projection biases, where the modules carry them,
    act before the norm and the rotation as in the stock modules)."""
    if torch.is_grad_enabled() and hidden_states.requires_grad:
        raise RuntimeError("compressed attention is inference-only (mdg_rope_gather has no backward); use torch.no_grad()")
    B, T, _ = hidden_states.shape
    cfg = self.config
    n_h, n_kv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, self.head_dim
    q = self.q_proj(hidden_states)
    k = self.k_proj(hidden_states)
    v = self.v_proj(hidden_states)
    r_qk = q.shape[-1] // n_h
    v = v.view(B, T, n_kv, v.shape[-1] // n_kv).transpose(1, 2)
    cos, sin = position_embeddings                               # [B or 1, T, head_dim]
    mask = self.layer_rotary_mask                                # int64 [n_kv, r_qk] or None
    if mask is not None and mask.device != q.device:             # a plain attribute (see _install): moved on first use
        mask = self.layer_rotary_mask = mask.to(q.device)
    qw = kw = None
    eps = 1e-6
    if getattr(self, "q_norm", None) is not None:
        if mask is None:                                         # QK stage not run: the stock per-head norm
            q = self.q_norm(q.view(B, T, n_h, r_qk)).view(B, T, -1)
            k = self.k_norm(k.view(B, T, n_kv, r_qk)).view(B, T, -1)
        else:
            qw, kw, eps = self.q_norm.weight, self.k_norm.weight, self.q_norm.variance_epsilon
    if mask is not None:
        # the reference's gather index has batch extent 1 (LlamaRebuild.py:167-175): batch 0's table serves every batch
        cos, sin = cos[:1], sin[:1]
    q = _rope_gather(q, cos, sin, mask, n_h, n_kv, hd, norm_weight=qw, eps=eps)         # [B, n_h,  T, r_qk]
    k = _rope_gather(k, cos, sin, mask, n_kv, n_kv, hd, norm_weight=kw, eps=eps)        # [B, n_kv, T, r_qk]
    if past_key_values is not None:
        k, v = past_key_values.update(k, v, self.layer_idx)
    extra = {"sliding_window": self.sliding_window} if getattr(self, "sliding_window", None) is not None else {}
    out, weights = _attend(self, q, k, v, attention_mask, float(r_qk) ** -0.5, kwargs, extra)
    return self.o_proj(out), weights


def _opt_forward(self, hidden_states, past_key_values=None, attention_mask=None, output_attentions=False, **kwargs):
    B, T, _ = hidden_states.shape
    n_h = self.num_heads
    q = self.q_proj(hidden_states)
    r_qk = q.shape[-1] // n_h
    q = q * (float(r_qk) ** -0.5)                                # pre-scaled, as upstream OPT does; scale 1 below
    k = self.k_proj(hidden_states)
    v = self.v_proj(hidden_states)
    q = q.view(B, T, n_h, r_qk).transpose(1, 2)
    k = k.view(B, T, n_h, r_qk).transpose(1, 2)
    v = v.view(B, T, n_h, v.shape[-1] // n_h).transpose(1, 2)
    if past_key_values is not None:
        k, v = past_key_values.update(k, v, self.layer_idx)
    out, weights = _attend(self, q, k, v, attention_mask, 1.0, kwargs, want_weights=bool(output_attentions))
    return self.out_proj(out), (weights if output_attentions else None)


def _check_mask(mask: torch.Tensor, n_kv: int, head_dim: int, layer: int) -> torch.Tensor:
    """The kernel clamps indices for memory safety only; a mask that does not index head_dim is refused here, once."""
    if mask.dim() != 2 or mask.shape[0] != n_kv or mask.shape[1] % 2:
        raise ValueError(f"layer {layer}: rotary mask must be [n_kv={n_kv}, even width], got {tuple(mask.shape)}")
    mask = mask.to(torch.int64)
    if mask.numel() and (int(mask.min()) < 0 or int(mask.max()) >= head_dim):
        raise ValueError(f"layer {layer}: rotary mask indexes outside head_dim={head_dim}")
    return mask.contiguous()


def _attention_modules(model, arch: str):
    blocks = model.model.decoder.layers if arch == "opt" else model.model.layers
    return [b.self_attn for b in blocks]


def _install(model, arch: str, rotary_masks: Optional[List[torch.Tensor]]) -> None:
    attns = _attention_modules(model, arch)
    if rotary_masks is not None and len(rotary_masks) != len(attns):
        raise ValueError(f"{len(rotary_masks)} rotary masks for {len(attns)} layers")
    for i, attn in enumerate(attns):
        if arch == "opt":
            attn.forward = types.MethodType(_opt_forward, attn)
            continue
        mask = None
        if rotary_masks is not None and rotary_masks[i] is not None:
            mask = _check_mask(rotary_masks[i], attn.config.num_key_value_heads, attn.head_dim, i)
        # a plain attribute, as upstream (LlamaRebuild.py:310): HF materialises unknown buffers of a model built on the
        # meta device as uninitialised memory, which would silently replace the mask
        attn.layer_rotary_mask = mask
        attn.forward = types.MethodType(_rope_forward, attn)


def install_compressed_attention(adapter, rotary_masks: Optional[List[torch.Tensor]]) -> None:
    """Give every attention module of `adapter.model` the compressed-aware forward.  `rotary_masks`: the list
    `compress_qk` returned (one int64 [n_kv, r_qk] tensor per layer, layer order) or None for architectures without
    RoPE masks (OPT) / for an uncompressed QK stage."""
    _install(adapter.model, "opt" if adapter.arch == "opt" else adapter.arch, rotary_masks)


def _resize(linear: nn.Linear, out_features: Optional[int] = None, in_features: Optional[int] = None, bias: bool = False) -> nn.Linear:
    """A Linear of the compressed shape on the device / dtype of the one it replaces: bias-free (ModelAdapter.convert_model builds
    bias-free modules, model_adapter.py:199-208, so the checkpoint holds no bias for them) unless `bias` -- the checkpoint's
    config.projection_biases names this projection: a run that carried the biases (MODEGPT_KEEP_BIAS=1, Qwen2)."""
    o = linear.out_features if out_features is None else out_features
    i = linear.in_features if in_features is None else in_features
    if (o, i) == (linear.out_features, linear.in_features) and (linear.bias is not None) == bias:
        return linear
    return nn.Linear(i, o, bias=bias, device=linear.weight.device, dtype=linear.weight.dtype)


def shrink_to_config_ranks(model, arch: str) -> None:
    """Called from the constructor of a modeling file shipped with a compressed checkpoint, BEFORE the weights are loaded:
    give every projection the per-layer shape recorded by patch_config (q_ranks / k_ranks / v_ranks / o_ranks /
    gate_ranks; qk_ranks / vo_ranks for OPT) and a bias exactly where config.projection_biases says the state dict holds
    one, read rotary_masks.pt from config.mask_path, install the forward."""
    cfg = model.config
    attns = _attention_modules(model, arch)
    blocks = model.model.decoder.layers if arch == "opt" else model.model.layers
    has = set(getattr(cfg, "projection_biases", None) or ())      # (absent: a checkpoint without carried biases, as before)
    for i, (block, attn) in enumerate(zip(blocks, attns)):
        if arch == "opt":
            qk, vo = cfg.qk_ranks[i], cfg.vo_ranks[i]
            attn.q_proj, attn.k_proj = _resize(attn.q_proj, qk, bias="q" in has), _resize(attn.k_proj, qk, bias="k" in has)
            attn.v_proj = _resize(attn.v_proj, vo, bias="v" in has)
            attn.out_proj = _resize(attn.out_proj, in_features=vo, bias="o" in has)
            block.fc1 = _resize(block.fc1, cfg.gate_ranks[i], bias="up" in has)
            block.fc2 = _resize(block.fc2, in_features=cfg.gate_ranks[i], bias="down" in has)
        else:
            attn.q_proj = _resize(attn.q_proj, cfg.q_ranks[i], bias="q" in has)
            attn.k_proj = _resize(attn.k_proj, cfg.k_ranks[i], bias="k" in has)
            attn.v_proj = _resize(attn.v_proj, cfg.v_ranks[i], bias="v" in has)
            attn.o_proj = _resize(attn.o_proj, in_features=cfg.o_ranks[i], bias="o" in has)
            g = cfg.gate_ranks[i]
            block.mlp.gate_proj = _resize(block.mlp.gate_proj, g, bias="gate" in has)
            block.mlp.up_proj = _resize(block.mlp.up_proj, g, bias="up" in has)
            block.mlp.down_proj = _resize(block.mlp.down_proj, in_features=g, bias="down" in has)
    masks = None
    path = getattr(cfg, "mask_path", None)
    if arch != "opt" and path:
        if not os.path.exists(path):
            raise FileNotFoundError(f"config.mask_path = {path} does not exist (the checkpoint stores an absolute path, "
                                    "as upstream does: model_utils.py:105-112)")
        masks = torch.load(path, map_location="cpu")
    _install(model, arch, masks)
