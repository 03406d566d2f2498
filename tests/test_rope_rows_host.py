"""CPU: the model of mdg_rope_rows is the library's rotary expression; the entry point checks its arguments without a device."""
import numpy as np
import pytest
import torch

from modegpt_amd import _lib
from tests import rope_rows_ref as R


@pytest.mark.parametrize("hd", R.HEAD_DIMS)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_model_is_the_librarys_expression_bit_for_bit(dt, hd):
    """tests/rope_rows_ref.rope_rows against transformers' apply_rotary_pos_emb ([B, heads, T, hd] layout, cos / sin unsqueezed over
    the heads) on every case of the GPU test: element-wise ops, so the layout cannot change a bit."""
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb
    for c in R.all_cases(dt, hd):
        B, T = c.dims
        q = c.x.reshape(B, T, c.n_heads, hd).transpose(1, 2)
        cos, sin = (t.expand(B, T, hd) for t in (c.cos, c.sin))
        lib_q, lib_k = apply_rotary_pos_emb(q, q[:, :1], cos, sin)
        assert R.same_bits(lib_q.transpose(1, 2).reshape(B, T, -1), c.want), (dt, hd, c.n_heads, c.dims)
        assert R.same_bits(lib_k, lib_q[:, :1])
        assert not bool(torch.isnan(c.want).any())


def test_signs_of_zeros_are_part_of_the_model():
    """An all-zero row gives (+0) + (-0 * sin) ...: the model keeps whatever torch gives, and same_bits sees a flipped sign."""
    c = R.make_case("f16", 16, 3, 2, 70, "shared")
    flipped = c.want.clone()
    zero = (flipped == 0).nonzero()[0]
    flipped[tuple(zero)] = -flipped[tuple(zero)]
    assert R.same_bits(c.want, c.want.clone()) and not R.same_bits(flipped, c.want)


def test_bad_arguments_return_a_status_and_a_message_without_a_device():
    lib = _lib.load()
    X, O, Cs, Sn = 0x10000, 0x90000, 0x20000, 0x30000          # never dereferenced: every call below is refused before any device work

    def call(x=X, dtype=_lib.MDG_BF16, ld_x=64, B=2, T=5, n_heads=4, hd=16, cos=Cs, sin=Sn, cs=0, out=O, ld_out=64):
        return lib.mdg_rope_rows(x, dtype, ld_x, B, T, n_heads, hd, cos, sin, cs, out, ld_out, None)

    bad = [(dict(x=None), "null"), (dict(out=None), "null"), (dict(cos=None), "null"), (dict(sin=None), "null"),
           (dict(dtype=_lib.MDG_F64), "dtype"), (dict(dtype=99), "dtype"),
           (dict(hd=15, ld_x=60, ld_out=60), "even"), (dict(hd=0), "even"), (dict(hd=258, ld_x=2000, ld_out=2000), "256"),
           (dict(ld_x=63), "ld_x"), (dict(ld_out=63), "ld_out"), (dict(n_heads=0), "n_heads"), (dict(B=-1), "negative"),
           (dict(cs=79), "stride"),
           (dict(out=X), "overlap"), (dict(out=X + 2 * 64 * 3), "overlap"), (dict(x=O + 2), "overlap"),
           (dict(out=X + 2 * 16, ld_x=128, ld_out=128), "overlap")]          # interleaved column slices of one buffer: refused too
    for kw, word in bad:
        assert call(**kw) == _lib.MDG_ERR_BAD_ARG, kw
        assert word in lib.mdg_last_error().decode(), (kw, lib.mdg_last_error())
        with pytest.raises(RuntimeError):
            _lib.check(call(**kw), "mdg_rope_rows")
    # an empty call is not an error and launches nothing, whatever the pointers
    assert call(B=0, x=None, out=None) == _lib.MDG_OK and call(T=0, cos=None) == _lib.MDG_OK


def test_ops_rope_rows_refuses_cpu_tensors():
    from modegpt_amd import ops
    c = R.make_case("bf16", 16, 3, 1, 5, "shared")
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.rope_rows(c.x, c.cos, c.sin, c.n_heads, c.hd)


def test_switches_are_read_at_call_time(monkeypatch):
    from modegpt_amd import ops, reports
    for fn, name in ((reports.qk_rope_enabled, "MODEGPT_QK_ROPE"), (reports.qk_rope_select_enabled, "MODEGPT_QK_ROPE_SELECT")):
        monkeypatch.delenv(name, raising=False)
        assert fn() is False and getattr(ops, fn.__name__) is fn
        monkeypatch.setenv(name, "1")
        assert fn() is True
        monkeypatch.setenv(name, "0")
        assert fn() is False


def test_cache_entries_of_the_rope_statistics_are_validated_like_q_and_k(tmp_path):
    from modegpt_amd import calib_cache as CC
    arch = {"n_inner": 8, "d_model": 8, "head_dim": 4, "n_heads": 2, "n_kv_heads": 1}
    rng = np.random.default_rng(0)
    vals = rng.standard_normal(2 * 4 * 4)
    entry = CC.write_data_file(str(tmp_path), 3, "q_rope", vals, 4, 2)
    assert entry["file"] == "layer_3_q_rope.f64" and entry["layout"] == "full" and entry["bytes"] == 8 * 32
    assert sorted(entry) == sorted(CC.write_data_file(str(tmp_path), 3, "q", vals, 4, 2))          # the sidecar fields of q / k
    assert CC.validate_extra_entry({"files": {"q_rope": entry}}, arch, 3, "q_rope") == entry
    out = np.empty(32)
    CC.read_data_file(str(tmp_path), 3, "q_rope", entry, out)
    assert np.array_equal(out.view(np.int64), vals.view(np.int64))
    with pytest.raises(ValueError, match=r"layer 3.*q_rope"):
        CC.validate_extra_entry({"files": {}}, arch, 3, "q_rope")
    with pytest.raises(ValueError, match=r"layer 3.*k_rope\.batch"):
        CC.validate_extra_entry({"files": {"k_rope": entry}}, arch, 3, "k_rope")
