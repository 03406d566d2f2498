"""Fp8KVCache: a KV cache for compressed models that holds K and V as OCP e4m3 with one power-of-two scale per (batch, kv head,
token) -- the layout of include/modegpt_hip.h -- and never copies itself on a decode step.

    cache = Fp8KVCache()                 # capacity doubles when it runs out (the only copy there is)
    cache = Fp8KVCache(max_len=4096)     # fixed capacity: no copy at all, a longer sequence is an error
    model.generate(..., past_key_values=cache)     # or model(input_ids, past_key_values=cache, use_cache=True)

A layer takes its widths (r_qk, r_vo: they differ per layer in a compressed model), batch, kv heads, dtype and device from its first
update, as transformers' DynamicLayer does.  update() appends the new rows with ops.kv8_append (csrc/kv8.hip) and returns two
Fp8Rows -- (data, scale, S, r) views of the layer's K and V planes -- instead of tensors.  The forwards of
patchers/compressed_attention.py recognise them: with MODEGPT_FUSED_ATTN=1 every call the fused kernels serve reads the fp8 planes
directly -- ops.attn_decode_kv8 for a call in the decode kernel's domain when MODEGPT_FUSED_ATTN_DECODE=1 is set as well,
ops.attn_fwd_kv8 for every other one (chunked prefill, later prompts, wide verification steps) -- and a prefill into an empty cache
attends over the fresh k / v it was given.  Only a call that takes HF's attention interface reads the cache back with
ops.kv8_dequant and goes on as it would have with a DynamicCache.  step() is update() with the rotary stage of q and k in front, all in
one launch (ops.rope_kv8_step, csrc/rope_kv8_step.hip); the forward calls it instead of update() under MODEGPT_FUSED_KV_STEP=1.

Engine-only: this module needs libmodegpt_hip.so and a GPU, and is not shipped next to a checkpoint.  Beam search
(reorder_cache) is refused."""
from __future__ import annotations

from typing import Optional

import torch
from transformers.cache_utils import Cache, CacheLayerMixin

from .. import ops


class Fp8Rows:
    """The first S rows of one plane pair of a layer: data uint8 [B, n_kv, cap, pitch], scale float32 [B, n_kv, cap], r elements a
    row; `fresh` is the bf16 / f16 tensor whose rows the last update appended.  It answers what the attention forward asks of a
    key / value tensor before it picks a kernel (shape, stride, device, dtype, requires_grad)."""
    is_kv8 = True
    requires_grad = False

    def __init__(self, data, scale, S, r, fresh, dtype=None):
        # fresh is None for the K rows of a fused step (Fp8KVLayer.step) that wrote no bf16 k: then `dtype` is the layer's
        self.data, self.scale, self.S, self.r, self.fresh = data, scale, S, r, fresh
        self.dtype, self.device = (dtype, data.device) if fresh is None else (fresh.dtype, fresh.device)
        self.shape = torch.Size((data.shape[0], data.shape[1], S, r))

    def stride(self, dim=None):
        st = (self.shape[1] * self.S * self.r, self.S * self.r, self.r, 1)     # of the dequantised tensor
        return st if dim is None else st[dim]

    def dequant(self) -> torch.Tensor:
        return ops.kv8_dequant(self.data, self.scale, self.S, self.r, self.dtype)


class Fp8KVLayer(CacheLayerMixin):
    is_sliding = False
    INITIAL_CAPACITY = 256

    def __init__(self, max_len: Optional[int] = None):
        super().__init__()
        self.max_len = max_len
        self.length = 0
        self.copies = 0          # doublings so far: the only times the cache was copied

    def lazy_initialization(self, key_states: torch.Tensor, value_states: torch.Tensor) -> None:
        if not key_states.is_cuda or key_states.dtype not in (torch.bfloat16, torch.float16):
            raise ValueError(f"Fp8KVCache holds bf16 / f16 states of a GPU model, got {key_states.dtype} on {key_states.device}")
        self.dtype, self.device = key_states.dtype, key_states.device
        self.batch, self.n_kv = key_states.shape[0], key_states.shape[1]
        self.r_qk, self.r_vo = key_states.shape[-1], value_states.shape[-1]
        self.cap = 0
        self.is_initialized = True

    def _planes(self, cap: int, r: int):
        data = torch.empty(self.batch, self.n_kv, cap, ops.kv8_pitch(r), dtype=torch.uint8, device=self.device)
        return data, torch.empty(self.batch, self.n_kv, cap, dtype=torch.float32, device=self.device)

    def _reserve(self, need: int) -> None:
        if need <= self.cap:
            return
        if self.max_len is not None:
            if need > self.max_len:
                raise RuntimeError(f"Fp8KVCache(max_len={self.max_len}) cannot hold {need} tokens")
            cap = self.max_len
        else:
            cap = max(self.INITIAL_CAPACITY, self.cap)
            while cap < need:
                cap *= 2
        old = (self.keys, self.key_scale, self.values, self.value_scale) if self.cap else None
        self.keys, self.key_scale = self._planes(cap, self.r_qk)
        self.values, self.value_scale = self._planes(cap, self.r_vo)
        if old is not None and self.length:
            for new, was in zip((self.keys, self.key_scale, self.values, self.value_scale), old):
                new[:, :, :self.length].copy_(was[:, :, :self.length])
            self.copies += 1
        self.cap = cap

    def update(self, key_states: torch.Tensor, value_states: torch.Tensor, *args, **kwargs):
        if not self.is_initialized:
            self.lazy_initialization(key_states, value_states)
        if (tuple(key_states.shape[:2]) != (self.batch, self.n_kv) or key_states.shape[-1] != self.r_qk
                or value_states.shape[-1] != self.r_vo or key_states.shape[2] != value_states.shape[2]):
            raise ValueError(f"Fp8KVCache layer of [{self.batch}, {self.n_kv}, *, {self.r_qk} / {self.r_vo}] was given k "
                             f"{tuple(key_states.shape)}, v {tuple(value_states.shape)}")
        T = key_states.shape[2]
        self._reserve(self.length + T)
        ops.kv8_append(key_states, self.keys, self.key_scale, self.length)
        ops.kv8_append(value_states, self.values, self.value_scale, self.length)
        self.length += T
        return (Fp8Rows(self.keys, self.key_scale, self.length, self.r_qk, key_states),
                Fp8Rows(self.values, self.value_scale, self.length, self.r_vo, value_states))

    def step(self, q, k, v, cos, sin, mask, n_heads, head_dim, q_norm_weight=None, k_norm_weight=None, eps=1e-6):
        """update() with the rotary stage in front, in one launch (ops.rope_kv8_step): q [B, T, n_heads*r_qk] and k [B, T, n_kv*r_qk]
        as the projections wrote them, v [B, n_kv, T, r_vo] (a view).  Returns (q_rot [B, n_heads, T, r_qk], k_rows, v_rows); the rotated
        k exists as a tensor (k_rows.fresh) only when the layer was empty, where the forward attends over it."""
        B, T, n_kv = v.shape[0], v.shape[2], v.shape[1]
        if k.dim() != 3 or k.shape[-1] % n_kv:
            raise ValueError(f"Fp8KVCache.step: k {tuple(k.shape)} is not [B, T, {n_kv} * r_qk]")
        if not self.is_initialized:
            self.lazy_initialization(k.view(B, T, n_kv, -1).transpose(1, 2), v)
        if (B, n_kv) != (self.batch, self.n_kv) or k.shape[-1] != n_kv * self.r_qk or v.shape[-1] != self.r_vo or k.shape[1] != T:
            raise ValueError(f"Fp8KVCache layer of [{self.batch}, {self.n_kv}, *, {self.r_qk} / {self.r_vo}] was given k "
                             f"{tuple(k.shape)}, v {tuple(v.shape)}")
        self._reserve(self.length + T)
        q_rot, fresh = ops.rope_kv8_step(q, k, v, cos, sin, mask, n_heads, n_kv, head_dim, (self.keys, self.key_scale),
                                         (self.values, self.value_scale), self.length, q_norm_weight=q_norm_weight,
                                         k_norm_weight=k_norm_weight, eps=eps, k_out=True if self.length == 0 else None)
        self.length += T
        return (q_rot, Fp8Rows(self.keys, self.key_scale, self.length, self.r_qk, fresh, self.dtype),
                Fp8Rows(self.values, self.value_scale, self.length, self.r_vo, v))

    def get_seq_length(self) -> int:
        return self.length

    def get_mask_sizes(self, query_length: int) -> tuple[int, int]:
        return self.length + query_length, 0

    def get_max_length(self) -> int:
        return -1 if self.max_len is None else self.max_len

    def reset(self) -> None:
        self.length = 0          # the planes stay: rows at or beyond the length hold anything

    def reorder_cache(self, beam_idx) -> None:
        raise NotImplementedError("Fp8KVCache does not reorder its rows: beam search is out of scope (use a DynamicCache)")


class Fp8KVCache(Cache):
    """One Fp8KVLayer per model layer, created on first use.  max_len=None: capacity starts at 256 tokens and doubles."""

    def __init__(self, max_len: Optional[int] = None):
        super().__init__(layer_class_to_replicate=lambda: Fp8KVLayer(max_len))

    def step(self, layer_idx: int, *args, **kwargs):
        """Fp8KVLayer.step of layer `layer_idx` (created on first use, as update does): the fused rotary + append."""
        while len(self.layers) <= layer_idx:
            self.layers.append(self.layer_class_to_replicate())
        return self.layers[layer_idx].step(*args, **kwargs)
