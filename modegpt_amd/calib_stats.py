"""The optional calibration statistics, one record each: what calibration collects beside the four reference statistics when a
switch asks for it.  Everything that allocates, normalises, hands to the hooks, saves, loads or validates them reads this table
(calibration.SigmaBuffers and collected, calib_cache, the adapters' register_hooks, compress_qk), so a new statistic is one row
here, its launch in a hook and its consumer.  Host only: no torch, no library."""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

from .reports import _switch

QK_ROPE_ARCHS = ("llama", "qwen2")      # rotary models whose compressed attention keeps the dropped-column identity


class Stat(NamedTuple):
    name: str
    switch: str                             # the environment switch that collects, saves and demands it
    members: Tuple[Tuple[str, str], ...]    # (file kind, shape): "n_inner" / "d_model" -- a vector of that width; "q" / "k" -- like that statistic
    layout: str                             # on disk: "vector" (entry with sum_bits) or "full" (entry with trace_bits, through the staging buffers)
    sums_attr: str                          # the adapter attribute the hooks accumulate into during the sweep
    stats_attr: str                         # the adapter attribute the compressors read afterwards
    noun: str                               # what the adapter carries, as the refusals say it
    mirror: bool = False                    # finalised by ops.cov_finalize (mirror + normaliser), not by mul_
    token_power: int = 1                    # the normaliser is 1 / (n_texts * TOKENS_PER_TEXT_NORMALISER ** token_power)
    archs: Optional[Tuple[str, ...]] = None     # collected on these architectures only (None: on every one)
    needs: Optional[str] = None             # the statistic that must be collected beside it
    entry: Optional[str] = None             # the entry point whose head_dim <= 128 limit applies
    adjective: str = ""                     # "the <adjective> statistic" of the collection rule's messages
    elsewhere: str = ""                     # what the log says on an architecture without rotary embedding

    @property
    def kinds(self) -> Tuple[str, ...]:
        return tuple(kind for kind, _ in self.members)

    def enabled(self) -> bool:
        """The switch as it stands when asked (not frozen at import)."""
        return _switch(self.switch)


def _sequence_stat(name: str, switch: str, adjective: str, entry: str, token_power: int) -> Stat:
    """A [n_heads, hd, hd] pair (centred, raw) accumulated from the post-RoPE rows, one call per layer and batch."""
    return Stat(name, switch, ((name, "q"), (name + "_raw", "q")), "full", name + "_sums", name + "_stats", adjective + " statistic",
                token_power=token_power, archs=QK_ROPE_ARCHS, needs="qk_rope", entry=entry, adjective=adjective,
                elsewhere=f"has no rotary embedding and separate q / k hooks; the {adjective} statistic is not collected for it")


STATS = (
    Stat("mlp_mean", "MODEGPT_MLP_INTERCEPT", (("mlp_mean", "n_inner"),), "vector", "mlp_sums", "mlp_means", "activation means"),
    Stat("x_mean", "MODEGPT_VO_INTERCEPT", (("x_mean", "d_model"),), "vector", "x_sums", "x_means", "input means"),
    Stat("qk_rope", "MODEGPT_QK_ROPE", (("q_rope", "q"), ("k_rope", "k")), "full", "qk_rope_sums", "qk_rope_stats", "post-RoPE statistics",
         mirror=True, archs=QK_ROPE_ARCHS, adjective="post-RoPE",
         elsewhere="has no rotary embedding, the pre-RoPE statistic is already the exact one; nothing more is collected"),
    _sequence_stat("qk_pair", "MODEGPT_QK_SEQ", "within-sequence", "mdg_qk_pair_accum", token_power=2),
    _sequence_stat("qk_causal", "MODEGPT_QK_CAUSAL", "causal", "mdg_qk_causal_accum", token_power=1),
)
BY_NAME = {stat.name: stat for stat in STATS}
KIND_STAT = {kind: stat for stat in STATS for kind in stat.kinds}       # file kind -> its record, in table order
KIND_SHAPE = {kind: shape for stat in STATS for kind, shape in stat.members}


def layer_value(holder, name: str, layer: int, attr: str = "stats_attr"):
    """The value of statistic `name` for `layer` as `holder` carries it -- under the record's stats_attr, or its sums_attr during the
    sweep: the layer's tensor for a one-member statistic, the tuple of its members' otherwise.  None if the attribute is absent or
    None, if the layer's entry is None, or if the statistic it needs is None."""
    stat = BY_NAME[name]
    if stat.needs is not None and layer_value(holder, stat.needs, layer, attr) is None:
        return None
    value = getattr(holder, getattr(stat, attr), None)
    if value is None:
        return None
    if len(stat.members) == 1:
        return value[layer]
    entry = tuple(member[layer] for member in value)
    return None if any(t is None for t in entry) else entry
