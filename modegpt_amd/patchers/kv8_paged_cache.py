"""PagedFp8KVCache: the fp8 KV cache of kv8_cache.py with its memory handed out in pages -- the paged layout of
include/modegpt_hip.h -- so that growth never copies, capacity is shared by the sequences instead of reserved for the longest, and a
decode step's launch arguments do not change from step to step.

    cache = PagedFp8KVCache(n_pages=512)           # 512 pages of 64 tokens, shared by every sequence of the batch
    model.generate(..., past_key_values=cache)     # or model(input_ids, past_key_values=cache, use_cache=True)

One block table int32 [B, n_pages] and one seq_lens / pos vector int32 [B] live on the device and serve ALL layers; each layer owns a
K pool and a V pool of n_pages pages, sized from its first update (ranks differ per layer in a compressed model, so pitches do too).
A host free list hands a sequence a page when it crosses a page boundary -- the host knows the length, because Transformers advances
all sequences of a batch together -- and the first layer's update of a step writes the new table entries, pos and seq_lens; every
layer then appends its K and V rows with ONE ops.kv8_paged_append launch (csrc/kv8_paged.hip).  update() returns two PagedFp8Rows.
The forwards of patchers/compressed_attention.py recognise them: a call the two decode switches would send to attn_decode_kv8 runs
ops.attn_decode_paged8 (csrc/attn_decode_paged8.hip) straight from the pools, every other cached call the fused kernels serve (a
chunked prefill, a later prompt, a wide verification step, masked or not) runs ops.attn_fwd_paged8 (csrc/attn_fwd_paged8.hip)
straight from the pools as well, and a prefill into an empty cache attends over the fresh k / v.  Only a call that takes HF's
attention interface gathers the rows with ops.kv8_paged_dequant.  step() is update() with the rotary stage of q and k in front, all in
one launch (ops.rope_kv8_paged_step, csrc/rope_kv8_step.hip); the forward calls it instead of update() under MODEGPT_FUSED_KV_STEP=1.

Engine-only, like kv8_cache.py.  An exhausted pool raises; reset() returns every page; beam search (reorder_cache) is refused."""
from __future__ import annotations

import torch
from transformers.cache_utils import Cache, CacheLayerMixin

from .. import ops


class PagedFp8Rows:
    """The first S rows of every sequence in one pool of a layer: pool = (data uint8 [n_pages, n_kv, page, pitch], scale float32
    [n_pages, n_kv, page]) behind the cache's block_table and seq_lens, r elements a row; `fresh` is the bf16 / f16 tensor whose rows
    the last update appended.  It answers what the attention forward asks of a key / value tensor before it picks a kernel."""
    is_kv8 = True
    is_paged = True
    requires_grad = False

    def __init__(self, pool, block_table, seq_lens, S, r, fresh, dtype=None):
        # fresh is None for the K rows of a fused step (PagedFp8KVLayer.step) that wrote no bf16 k: then `dtype` is the layer's
        self.pool, self.block_table, self.seq_lens, self.S, self.r, self.fresh = pool, block_table, seq_lens, S, r, fresh
        self.dtype, self.device = (dtype, pool[0].device) if fresh is None else (fresh.dtype, fresh.device)
        self.shape = torch.Size((block_table.shape[0], pool[0].shape[1], S, r))

    def stride(self, dim=None):
        st = (self.shape[1] * self.S * self.r, self.S * self.r, self.r, 1)     # of the gathered tensor
        return st if dim is None else st[dim]

    def dequant(self) -> torch.Tensor:
        return ops.kv8_paged_dequant(self.pool, self.block_table, self.S, self.r, self.dtype)


class PagedFp8KVLayer(CacheLayerMixin):
    is_sliding = False

    def __init__(self, owner: "PagedFp8KVCache"):
        super().__init__()
        self.owner = owner
        self.length = 0

    def lazy_initialization(self, key_states: torch.Tensor, value_states: torch.Tensor) -> None:
        if not key_states.is_cuda or key_states.dtype not in (torch.bfloat16, torch.float16):
            raise ValueError(f"PagedFp8KVCache holds bf16 / f16 states of a GPU model, got {key_states.dtype} on {key_states.device}")
        self.dtype, self.device = key_states.dtype, key_states.device
        self.batch, self.n_kv = key_states.shape[0], key_states.shape[1]
        self.r_qk, self.r_vo = key_states.shape[-1], value_states.shape[-1]
        n_pages, page = self.owner.n_pages, self.owner.page
        self.keys, self.values = (
            (torch.empty(n_pages, self.n_kv, page, ops.kv8_pitch(r), dtype=torch.uint8, device=self.device),
             torch.empty(n_pages, self.n_kv, page, dtype=torch.float32, device=self.device)) for r in (self.r_qk, self.r_vo))
        self.is_initialized = True

    def update(self, key_states: torch.Tensor, value_states: torch.Tensor, *args, **kwargs):
        if not self.is_initialized:
            self.lazy_initialization(key_states, value_states)
        if (tuple(key_states.shape[:2]) != (self.batch, self.n_kv) or key_states.shape[-1] != self.r_qk
                or value_states.shape[-1] != self.r_vo or key_states.shape[2] != value_states.shape[2]):
            raise ValueError(f"PagedFp8KVCache layer of [{self.batch}, {self.n_kv}, *, {self.r_qk} / {self.r_vo}] was given k "
                             f"{tuple(key_states.shape)}, v {tuple(value_states.shape)}")
        T = key_states.shape[2]
        table, seq_lens, pos = self.owner.advance(self.batch, self.length, T, self.device)
        ops.kv8_paged_append(key_states, value_states, self.keys, self.values, table, pos)
        self.length += T
        return (PagedFp8Rows(self.keys, table, seq_lens, self.length, self.r_qk, key_states),
                PagedFp8Rows(self.values, table, seq_lens, self.length, self.r_vo, value_states))

    def step(self, q, k, v, cos, sin, mask, n_heads, head_dim, q_norm_weight=None, k_norm_weight=None, eps=1e-6):
        """update() with the rotary stage in front, in one launch (ops.rope_kv8_paged_step): q [B, T, n_heads*r_qk] and
        k [B, T, n_kv*r_qk] as the projections wrote them, v [B, n_kv, T, r_vo] (a view).  Returns (q_rot [B, n_heads, T, r_qk], k_rows,
        v_rows); the rotated k exists as a tensor (k_rows.fresh) only when the layer was empty, where the forward attends over it."""
        B, T, n_kv = v.shape[0], v.shape[2], v.shape[1]
        if k.dim() != 3 or k.shape[-1] % n_kv:
            raise ValueError(f"PagedFp8KVCache.step: k {tuple(k.shape)} is not [B, T, {n_kv} * r_qk]")
        if not self.is_initialized:
            self.lazy_initialization(k.view(B, T, n_kv, -1).transpose(1, 2), v)
        if (B, n_kv) != (self.batch, self.n_kv) or k.shape[-1] != n_kv * self.r_qk or v.shape[-1] != self.r_vo or k.shape[1] != T:
            raise ValueError(f"PagedFp8KVCache layer of [{self.batch}, {self.n_kv}, *, {self.r_qk} / {self.r_vo}] was given k "
                             f"{tuple(k.shape)}, v {tuple(v.shape)}")
        table, seq_lens, pos = self.owner.advance(self.batch, self.length, T, self.device)
        q_rot, fresh = ops.rope_kv8_paged_step(q, k, v, cos, sin, mask, n_heads, n_kv, head_dim, self.keys, self.values, table, pos,
                                               q_norm_weight=q_norm_weight, k_norm_weight=k_norm_weight, eps=eps,
                                               k_out=True if self.length == 0 else None)
        self.length += T
        return (q_rot, PagedFp8Rows(self.keys, table, seq_lens, self.length, self.r_qk, fresh, self.dtype),
                PagedFp8Rows(self.values, table, seq_lens, self.length, self.r_vo, v))

    def get_seq_length(self) -> int:
        return self.length

    def get_mask_sizes(self, query_length: int) -> tuple[int, int]:
        return self.length + query_length, 0

    def get_max_length(self) -> int:
        return -1

    def reset(self) -> None:
        self.length = 0          # the pools stay: the pages go back to the cache's free list (PagedFp8KVCache.reset)

    def reorder_cache(self, beam_idx) -> None:
        raise NotImplementedError("PagedFp8KVCache does not reorder its rows: beam search is out of scope (use a DynamicCache)")


class PagedFp8KVCache(Cache):
    """One PagedFp8KVLayer per model layer, created on first use, behind one block table.  n_pages pages of `page` tokens (a positive
    multiple of 64) are shared by the sequences of the batch; each layer's two pools hold n_pages pages of its own widths."""

    def __init__(self, n_pages: int, page: int = 64):
        if n_pages < 1 or page < 64 or page % 64:
            raise ValueError(f"PagedFp8KVCache(n_pages={n_pages}, page={page}): at least one page, page a positive multiple of 64")
        super().__init__(layer_class_to_replicate=lambda: PagedFp8KVLayer(self))
        self.n_pages, self.page = int(n_pages), int(page)
        self.length = 0                                   # tokens every sequence holds: what the table, pos and seq_lens describe
        self.free = list(range(self.n_pages - 1, -1, -1))  # the host free list (pages are popped from its end: 0, 1, 2, ...)
        self.owned = None                                 # per sequence, the pages it was handed, in order
        self.block_table = self.seq_lens = self.pos = None

    def step(self, layer_idx: int, *args, **kwargs):
        """PagedFp8KVLayer.step of layer `layer_idx` (created on first use, as update does): the fused rotary + append."""
        while len(self.layers) <= layer_idx:
            self.layers.append(self.layer_class_to_replicate())
        return self.layers[layer_idx].step(*args, **kwargs)

    @property
    def pages_in_use(self) -> int:
        return self.n_pages - len(self.free)

    def advance(self, batch: int, start: int, T: int, device):
        """Called by every layer's update with the length it holds: the first layer of a step (start == self.length) extends the
        table by the pages the T new tokens need and sets pos = start, seq_lens = start + T on the device; the other layers of the
        step find it done.  Returns (block_table, seq_lens, pos)."""
        if self.block_table is None:
            self.owned = [[] for _ in range(batch)]
            self.block_table = torch.zeros(batch, self.n_pages, dtype=torch.int32, device=device)
            self.seq_lens = torch.zeros(batch, dtype=torch.int32, device=device)
            self.pos = torch.zeros(batch, dtype=torch.int32, device=device)
        if batch != len(self.owned) or device != self.block_table.device:
            raise ValueError(f"PagedFp8KVCache of {len(self.owned)} sequences on {self.block_table.device} was given {batch} on {device}")
        if start == self.length and T > 0:
            have, need = len(self.owned[0]), -(-(start + T) // self.page)
            if (need - have) * batch > len(self.free):
                raise RuntimeError(f"PagedFp8KVCache(n_pages={self.n_pages}, page={self.page}) is exhausted: {batch} sequences of "
                                   f"{start + T} tokens need {need * batch} pages")
            if need > have:
                new = [[self.free.pop() for _ in range(need - have)] for _ in range(batch)]
                for mine, got in zip(self.owned, new):
                    mine.extend(got)
                self.block_table[:, have:need] = torch.tensor(new, dtype=torch.int32).to(device)
            self.pos.fill_(start)
            self.seq_lens.fill_(start + T)
            self.length = start + T
        elif start + T != self.length:
            raise RuntimeError(f"PagedFp8KVCache: a layer holding {start} tokens was given {T} while the cache holds {self.length} "
                               f"(the layers of a model advance together)")
        return self.block_table, self.seq_lens, self.pos

    def reset(self) -> None:
        for layer in self.layers:
            layer.reset()
        self.length = 0
        self.free = list(range(self.n_pages - 1, -1, -1))
        if self.owned is not None:
            self.owned = [[] for _ in self.owned]
            self.seq_lens.zero_()
            self.pos.zero_()
