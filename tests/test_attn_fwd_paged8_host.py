"""CPU: mdg_attn_fwd_paged8 checks its arguments without a device, with a message before any device work -- what mdg_attn_fwd_kv8
refuses and the paged entries' own; causal with few keys is NOT refused (decided per sequence on the device); an empty call returns
MDG_OK whatever the pointers."""
import pytest

from modegpt_amd import _lib
from tests.test_attn_fwd_host import O, Q, refused
from tests.test_kv8_host import KD, KS, M, VD, VS
from tests.test_kv8_paged_host import LEN, PAGE, PAGES, TAB

NAME = "mdg_attn_fwd_paged8"
SM = 0x680000                                                             # a summary; never dereferenced
NEED = 4                                                                  # mdg_attn_mask_summary_bytes(2, 1, 5, 70): 2 x 1 x 1 x 2 tiles
PITCHES = ": pitches (%d, %d) must be multiples of 16 and >= mdg_kv8_pitch of r_qk=%d, r_vo=%d"
ALIGNED = ": data must be 16-byte and scales 4-byte aligned"
TABLE4 = ": block_table and seq_lens must be 4-byte aligned"


def call(q=Q, kd=KD, ks=KS, vd=VD, vs=VS, dtype=_lib.MDG_BF16, B=2, T=5, max_S=70, n_heads=4, n_kv=2, r_qk=6, r_vo=3, n_pages=6, page=64,
         kp=16, vp=16, table=TAB, table_len=3, lens=LEN, scale=0.5, causal=1, out=O, ld_out=12, mask=None, Hm=1, mbs=350, mhs=0, mqs=70,
         summary=SM, summary_bytes=NEED):
    return _lib.load().mdg_attn_fwd_paged8(q, kd, ks, vd, vs, dtype, B, T, max_S, n_heads, n_kv, r_qk, r_vo, n_pages, page, kp, vp, table,
                                           table_len, lens, scale, causal, out, ld_out, None, mask, Hm, mbs, mhs, mqs, summary, summary_bytes)


BAD = [  # what mdg_attn_fwd_kv8 refuses, in its words
    (dict(dtype=_lib.MDG_F32), ": dtype 2 (bf16 or f16; fp32 inputs are out of scope)"), (dict(max_S=-1), ": negative extent"),
    (dict(T=-1), ": negative extent"), (dict(n_kv=3), ": n_heads=4 is not a positive multiple of n_kv=3"),
    (dict(r_qk=7), ": r_qk=7 must be even, >= 2 and <= 256"), (dict(r_qk=258, kp=272), ": r_qk=258 must be even, >= 2 and <= 256"),
    (dict(r_vo=257, vp=272), ": r_vo=257 must be in 1..256"),
    (dict(kp=8), PITCHES % (8, 16, 6, 3)), (dict(vp=24), PITCHES % (16, 24, 6, 3)), (dict(r_qk=18), PITCHES % (16, 16, 18, 3)),
    (dict(r_vo=17), PITCHES % (16, 16, 6, 17)),
    (dict(ld_out=11), ": ld_out=11 < n_heads*r_vo=12"), (dict(scale=0.0), ": scale 0 must be finite and positive"),
    (dict(scale=float("nan")), ": scale nan must be finite and positive"), (dict(B=2 ** 60), ": B*T overflows"),
    (dict(q=None), ": null pointer"), (dict(out=None), ": null pointer"), (dict(kd=None), ": null pointer"), (dict(ks=None), ": null pointer"),
    (dict(vd=None), ": null pointer"), (dict(vs=None), ": null pointer"),
    (dict(kd=KD + 4), ALIGNED), (dict(vd=VD + 8), ALIGNED), (dict(ks=KS + 1), ALIGNED), (dict(vs=VS + 2), ALIGNED),
    (dict(q=O + 2), ": out overlaps q"), (dict(kd=O - 16), ": out overlaps k data"), (dict(ks=O + 236), ": out overlaps k scale"),
    (dict(vd=O + 16), ": out overlaps v data"), (dict(vs=O + 4), ": out overlaps v scale"),
    # the mask and its summary over max_S keys
    (dict(mask=M, Hm=2), ": mask heads Hm=2 must be 1 or n_heads=4"), (dict(mask=M, mqs=-70), ": negative mask stride (350, 0, -70)"),
    (dict(mask=M, summary=None), ": null summary"),
    (dict(mask=M, summary_bytes=NEED - 1), ": summary of %d bytes is short of mdg_attn_mask_summary_bytes = %d" % (NEED - 1, NEED)),
    (dict(mask=M, summary=O + 238), ": out overlaps summary"), (dict(mask=O + 1), ": out overlaps mask"),
    (dict(mask=M, summary=M + 699), ": summary overlaps mask"), (dict(mask=M, summary=Q), ": summary overlaps q"),
    (dict(mask=M, summary=KD + 6 * 2 * 64 * 16 - 2), ": summary overlaps k data"), (dict(mask=M, summary=KS), ": summary overlaps k scale"),
    (dict(mask=M, summary=VD + 100), ": summary overlaps v data"), (dict(mask=M, summary=VS + 190), ": summary overlaps v scale"),
    (dict(mask=M, summary=TAB + 20), ": summary overlaps block_table"), (dict(mask=M, summary=LEN + 4), ": summary overlaps seq_lens"),
    # the pages' own
    (dict(page=0), PAGE % 0), (dict(page=100), PAGE % 100), (dict(page=-64), PAGE % -64), (dict(n_pages=-1), PAGES),
    (dict(table_len=-1), PAGES), (dict(table_len=2 ** 60), ": table_len*page overflows"),
    (dict(max_S=193), ": max_S=193 keys exceed table_len*page=192"),
    (dict(n_pages=2 ** 31 - 1, page=2 ** 30, table_len=1), ": n_pages*n_kv*page*pitch overflows"),
    (dict(table_len=2 ** 40, B=2 ** 22, T=1), ": B*table_len overflows"),
    (dict(table=None), ": null pointer"), (dict(lens=None), ": null pointer"), (dict(table=TAB + 2), TABLE4), (dict(lens=LEN + 3), TABLE4),
    (dict(table=O + 8), ": out overlaps block_table"), (dict(lens=O + 236), ": out overlaps seq_lens")]


@pytest.mark.parametrize("kw,text", BAD, ids=lambda x: ",".join(x) if isinstance(x, dict) else None)
def test_fwd_paged8_refuses_a_bad_argument_without_a_device(kw, text):
    refused(_lib.load(), call, [(kw, NAME + text)], NAME)


@pytest.mark.parametrize("kw", [dict(B=0), dict(T=0)], ids=lambda kw: ",".join(kw))
def test_an_empty_call_returns_ok_whatever_the_pointers(kw):
    assert _lib.load().mdg_attn_mask_summary_bytes(2, 1, 5, 70) == NEED
    assert call(q=None, kd=None, ks=None, vd=None, vs=None, table=None, lens=None, out=None, summary=None, **kw) == _lib.MDG_OK


def test_causal_with_fewer_keys_than_queries_is_left_to_the_device():
    """max_S < T passes every check: the refusal that follows is the next one in order (a null q), not mdg_attn_fwd_kv8's causal one."""
    refused(_lib.load(), call, [(dict(max_S=3, q=None), NAME + ": null pointer")], NAME)
