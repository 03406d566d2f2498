"""Modeling file copied next to a compressed Qwen2 / Qwen2.5 checkpoint; config.auto_map names
`Qwen2Rebuild.Qwen2ForCausalLM`.  Same construction as DenseQwenRebuild.py: stock HF classes, projections resized to the
config's per-layer ranks, rotary masks from config.mask_path.  Qwen2 has no q_norm / k_norm; it has biases on q_proj,
k_proj and v_proj, which the compressors always carry for this family (the entries at the kept q/k columns, and
P_g b_v for the truncated v_proj), so config.projection_biases names all three and the resized modules keep them (the
reference has no Qwen2 patcher)."""
from transformers.models.qwen2.modeling_qwen2 import Qwen2ForCausalLM as _StockQwen2ForCausalLM

from .compressed_attention import shrink_to_config_ranks   # travels with the checkpoint (save_compressed_model copies both files)


class Qwen2ForCausalLM(_StockQwen2ForCausalLM):
    def __init__(self, config):
        super().__init__(config)
        shrink_to_config_ranks(self, "qwen2")
