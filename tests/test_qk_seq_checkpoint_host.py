"""CPU: a checkpoint whose rotary masks are what MODEGPT_QK_SEQ_SELECT=1 writes -- per kv head the lowest-frequency pair dropped,
where the post-RoPE rule keeps it first -- round-trips through the modeling file shipped with it: strict load, the live model's
logits bit for bit, in a process that cannot import the engine.  Beside a checkpoint with the other rule's masks nothing but the
mask (and the rows it gathered) differs: the same files, the same config keys, the same state-dict keys and shapes.  A mask is a mask."""
import json
import os
import subprocess
import sys

import pytest
import torch


def _model(scratch):
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    cfg = transformers.LlamaConfig(hidden_size=64, intermediate_size=160, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                   head_dim=16, vocab_size=97, max_position_embeddings=32)
    src = os.path.join(str(scratch), "source")
    transformers.LlamaForCausalLM(cfg).to(torch.bfloat16).save_pretrained(src)
    return transformers.AutoModelForCausalLM.from_pretrained(src, dtype=torch.bfloat16).eval()


def _compressed(scratch, rule):
    """A live compressed model without a GPU: the q / k rows the masks select (bit copies, as compress_qk gathers them), rank 8 of 16.
    rule "rope": unit 7, the lowest-frequency pair, first; rule "seq": unit 7 dropped."""
    from modegpt_amd.adapters.model_adapter import ModelAdapter
    from modegpt_amd.patchers import install_compressed_attention
    ad = ModelAdapter.from_model(_model(scratch), None)
    n_h, n_kv, hd, d = ad.n_heads, ad.n_kv_heads, ad.head_dim, ad.d_model
    g, ns = n_h // n_kv, hd // 2
    units = {"rope": [[7, 2, 5, 0], [7, 1, 3, 6]], "seq": [[2, 5, 0, 4], [1, 3, 6, 0]]}[rule]
    masks = []
    for i in range(ad.n_layers):
        idx = torch.tensor(units, dtype=torch.int64)
        mask = torch.cat((idx, idx + ns), dim=1)                             # [n_kv, rank]: compress_qk's layout
        c = ad.get_qk_components(i)
        q_rows = torch.cat([mask[h // g] + h * hd for h in range(n_h)])
        k_rows = torch.cat([mask[v] + v * hd for v in range(n_kv)])

        def lin(w):
            m = torch.nn.Linear(w.shape[1], w.shape[0], bias=False, dtype=torch.bfloat16)
            m.weight.data.copy_(w)
            return m
        ad.replace_attn_layers(i, lin(c.query_proj.weight.detach()[q_rows]), lin(c.key_proj.weight.detach()[k_rows]), None, None)
        masks.append(mask)
    install_compressed_attention(ad, masks)
    return ad, masks


def test_a_within_sequence_mask_round_trips_and_only_the_mask_differs(tmp_path):
    from modegpt_amd.model_utils import save_compressed_model
    ids = torch.randint(0, 97, (2, 12), generator=torch.Generator().manual_seed(5))
    saved = {}
    for rule in ("rope", "seq"):
        scratch = tmp_path / rule
        scratch.mkdir()
        ad, masks = _compressed(scratch, rule)
        ad.model.config._attn_implementation = "eager"
        with torch.no_grad():
            want = ad.model(ids).logits.float()
        out = str(scratch / "model")
        ad.patch_config()
        save_compressed_model(ad, rotary_masks=masks, save_dir=out, source_model_name="none")
        saved[rule] = (out, want, masks, {k: tuple(v.shape) for k, v in ad.model.state_dict().items()})
    out, want, masks, shapes = saved["seq"]
    cfg = json.load(open(os.path.join(out, "config.json")))
    assert cfg["auto_map"]["AutoModelForCausalLM"] == "LlamaRebuild.LlamaForCausalLM"
    torch.save({"ids": ids}, str(tmp_path / "live.pt"))
    script = f'''
import importlib.util, torch, transformers
assert importlib.util.find_spec("modegpt_amd") is None, "the engine must NOT be importable here"
m, info = transformers.AutoModelForCausalLM.from_pretrained({out!r}, trust_remote_code=True, dtype=torch.bfloat16, output_loading_info=True)
m = m.eval()
assert type(m).__module__.endswith("LlamaRebuild"), type(m).__module__
bad = {{k: sorted(v) for k, v in info.items() if k in ("missing_keys", "unexpected_keys", "mismatched_keys") and len(v)}}
assert not bad, bad
m.config._attn_implementation = "eager"
with torch.no_grad():
    logits = m(torch.load({str(tmp_path / "live.pt")!r})["ids"]).logits.float()
torch.save(logits, {str(tmp_path / "logits.pt")!r})
'''
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    env["HF_MODULES_CACHE"] = str(tmp_path / "hf_modules")
    p = subprocess.run([sys.executable, "-c", script], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    got = torch.load(str(tmp_path / "logits.pt"))
    assert torch.equal(got, want), float((got - want).abs().max())
    # beside the other rule's checkpoint: the same files, config keys and tensor shapes; the masks differ, and so do the logits
    other, other_want, other_masks, other_shapes = saved["rope"]
    assert sorted(os.listdir(out)) == sorted(os.listdir(other))
    other_cfg = json.load(open(os.path.join(other, "config.json")))
    assert sorted(cfg) == sorted(other_cfg)
    assert {k: v for k, v in cfg.items() if k != "mask_path"} == {k: v for k, v in other_cfg.items() if k != "mask_path"}
    assert shapes == other_shapes
    stored = torch.load(os.path.join(out, "rotary_masks.pt"))
    assert all(torch.equal(a, b) for a, b in zip(stored, masks)) and not any(torch.equal(a, b) for a, b in zip(masks, other_masks))
    assert all(7 not in m[:, :4].tolist()[v] for m in stored for v in range(2)) and all(int(m[v][0]) == 7 for m in other_masks for v in range(2))
    assert not torch.equal(want, other_want)
