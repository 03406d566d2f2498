"""CPU: the paged fp8 KV cache entries (mdg_kv8_paged_append, mdg_kv8_paged_dequant, mdg_attn_decode_paged8) check their arguments
without a device, with a message before any device work; an empty call returns MDG_OK whatever the pointers."""
from modegpt_amd import _lib
from tests.test_attn_decode_host import NEED, W
from tests.test_attn_fwd_host import O, Q, refused
from tests.test_kv8_host import KD, KS, M, VD, VS

KSRC, VSRC, TAB, LEN = 0x100000, 0x180000, 0x700000, 0x780000       # never dereferenced; TAB: the table, LEN: seq_lens or pos
PAGE = ": page=%d must be a positive multiple of 64"
PAGES = ": negative n_pages or table_len"


def test_append_refuses_bad_arguments_without_a_device():
    lib, name = _lib.load(), "mdg_kv8_paged_append"

    def call(ksrc=KSRC, vsrc=VSRC, dtype=_lib.MDG_BF16, B=2, n_kv=2, T=5, r_k=90, r_v=77, ks_=(900, 450, 90), vs_=(770, 385, 77), kd=KD,
             ks=KS, vd=VD, vs=VS, n_pages=6, page=64, kp=96, vp=80, table=TAB, table_len=3, pos=LEN):
        return lib.mdg_kv8_paged_append(ksrc, vsrc, dtype, B, n_kv, T, r_k, r_v, *ks_, *vs_, kd, ks, vd, vs, n_pages, page, kp, vp, table,
                                        table_len, pos, None)

    pitch = ": pitch=%d must be a multiple of 16 and >= mdg_kv8_pitch(%d) = %d"
    bad = [(dict(dtype=_lib.MDG_F32), ": dtype 2 (bf16 or f16)"), (dict(B=-1), ": negative extent"), (dict(T=-1), ": negative extent"),
           (dict(r_k=0), ": r_k=0 must be in 1..256"), (dict(r_v=257, vp=272), ": r_v=257 must be in 1..256"),
           (dict(kp=80), pitch % (80, 90, 96)), (dict(vp=88), pitch % (88, 77, 80)),
           (dict(page=0), PAGE % 0), (dict(page=96), PAGE % 96), (dict(page=-64), PAGE % -64),
           (dict(n_pages=-1), PAGES), (dict(table_len=-1), PAGES), (dict(table_len=2 ** 60), ": table_len*page overflows"),
           (dict(n_pages=2 ** 31 - 1, page=2 ** 30), ": n_pages*n_kv*page*pitch overflows"),
           (dict(ksrc=None), ": null pointer"), (dict(vsrc=None), ": null pointer"), (dict(table=None), ": null pointer"),
           (dict(pos=None), ": null pointer"), (dict(kd=None), ": null pointer"), (dict(vs=None), ": null pointer"),
           (dict(table=TAB + 2), ": block_table and pos must be 4-byte aligned"), (dict(pos=LEN + 1), ": block_table and pos must be 4-byte aligned"),
           (dict(kd=KD + 8), ": data must be 16-byte and scales 4-byte aligned"), (dict(vs=VS + 2), ": data must be 16-byte and scales 4-byte aligned"),
           (dict(ksrc=KD + 100), ": k data overlaps k src"), (dict(vsrc=VS + 8), ": v scale overlaps v src"),
           (dict(table=KS + 4), ": k scale overlaps block_table"), (dict(pos=VD + 64), ": v data overlaps pos"),
           (dict(ks=KD + 64), ": k data overlaps k scale"), (dict(vd=KD + 6 * 2 * 64 * 96 - 16), ": k data overlaps v data")]
    refused(lib, call, [(kw, name + text) for kw, text in bad], name)
    for kw in (dict(B=0), dict(n_kv=0), dict(T=0)):
        assert call(ksrc=None, vsrc=None, kd=None, ks=None, vd=None, vs=None, table=None, pos=None, **kw) == _lib.MDG_OK, kw


def test_dequant_refuses_bad_arguments_without_a_device():
    lib, name = _lib.load(), "mdg_kv8_paged_dequant"

    def call(data=KD, scale=KS, dtype=_lib.MDG_BF16, B=2, n_kv=2, S=70, r=77, n_pages=6, page=64, pitch=80, table=TAB, table_len=3, out=O):
        return lib.mdg_kv8_paged_dequant(data, scale, dtype, B, n_kv, S, r, n_pages, page, pitch, table, table_len, out, None)

    bad = [(dict(dtype=_lib.MDG_F64), ": dtype 3 (bf16 or f16)"), (dict(S=-1), ": negative extent"), (dict(r=0), ": r=0 must be in 1..256"),
           (dict(pitch=64), ": pitch=64 must be a multiple of 16 and >= mdg_kv8_pitch(77) = 80"), (dict(page=32), PAGE % 32),
           (dict(n_pages=-1), PAGES), (dict(S=193), ": S=193 rows exceed table_len*page=192"),
           (dict(n_pages=0), ": S=70 rows of a pool without pages"), (dict(data=None), ": null pointer"), (dict(table=None), ": null pointer"),
           (dict(out=None), ": null pointer"), (dict(scale=KS + 2), ": data must be 16-byte and scale 4-byte aligned"),
           (dict(table=TAB + 1), ": block_table must be 4-byte aligned"),
           (dict(out=KD + 6 * 2 * 64 * 80 - 2), ": data overlaps out"), (dict(out=KS - 2), ": scale overlaps out"),
           (dict(out=TAB + 20), ": block_table overlaps out")]
    refused(lib, call, [(kw, name + text) for kw, text in bad], name)
    for kw in (dict(B=0), dict(n_kv=0), dict(S=0)):
        assert call(data=None, scale=None, table=None, out=None, **kw) == _lib.MDG_OK, kw


def test_decode_refuses_bad_arguments_without_a_device():
    lib, name = _lib.load(), "mdg_attn_decode_paged8"

    def call(q=Q, kd=KD, ks=KS, vd=VD, vs=VS, dtype=_lib.MDG_BF16, B=2, T=5, max_S=70, n_heads=4, n_kv=2, r_qk=6, r_vo=3, n_pages=6, page=64,
             kp=16, vp=16, table=TAB, table_len=3, lens=LEN, scale=0.5, causal=1, splits=3, ws=W, ws_bytes=NEED, out=O, ld_out=12, mask=None,
             Hm=1, mbs=350, mhs=0, mqs=70):
        return lib.mdg_attn_decode_paged8(q, kd, ks, vd, vs, dtype, B, T, max_S, n_heads, n_kv, r_qk, r_vo, n_pages, page, kp, vp, table,
                                          table_len, lens, scale, causal, splits, ws, ws_bytes, out, ld_out, None, mask, Hm, mbs, mhs, mqs)

    pitches = ": pitches (%d, %d) must be multiples of 16 and >= mdg_kv8_pitch of r_qk=%d, r_vo=%d"
    aligned = ": data must be 16-byte and scales 4-byte aligned"
    bad = [  # what mdg_attn_decode_kv8 refuses, in its words
           (dict(dtype=_lib.MDG_F32), ": dtype 2 (bf16 or f16; fp32 inputs are out of scope)"), (dict(max_S=-1), ": negative extent"),
           (dict(n_kv=3), ": n_heads=4 is not a positive multiple of n_kv=3"), (dict(r_qk=7), ": r_qk=7 must be even, >= 2 and <= 256"),
           (dict(r_vo=257, vp=272), ": r_vo=257 must be in 1..256"),
           (dict(T=17), ": T=17 queries x group of 2 heads exceed the tile of 32 columns"),
           (dict(splits=0), ": splits=0 must be in 1..256"), (dict(splits=257), ": splits=257 must be in 1..256"),
           (dict(kp=8), pitches % (8, 16, 6, 3)), (dict(vp=24), pitches % (16, 24, 6, 3)), (dict(r_qk=18), pitches % (16, 16, 18, 3)),
           (dict(ld_out=11), ": ld_out=11 < n_heads*r_vo=12"), (dict(scale=0.0), ": scale 0 must be finite and positive"),
           (dict(B=2 ** 60), ": B*T overflows"), (dict(q=None), ": null pointer"), (dict(out=None), ": null pointer"),
           (dict(kd=None), ": null pointer"), (dict(vs=None), ": null pointer"), (dict(kd=KD + 4), aligned), (dict(vs=VS + 2), aligned),
           (dict(ws=None), ": null workspace"),
           (dict(ws_bytes=NEED - 1), ": workspace of %d bytes is short of mdg_attn_decode_ws_bytes = %d" % (NEED - 1, NEED)),
           (dict(ws=W + 8), ": workspace must be 16-byte aligned"), (dict(out=W + 64), ": workspace overlaps out"),
           (dict(q=O + 2), ": out overlaps q"), (dict(kd=O - 16), ": out overlaps k data"), (dict(ks=W + 16), ": workspace overlaps k scale"),
           (dict(vd=W + NEED - 16), ": workspace overlaps v data"), (dict(vs=O + 4), ": out overlaps v scale"),
           (dict(mask=M, Hm=2), ": mask heads Hm=2 must be 1 or n_heads=4"), (dict(mask=M, mqs=-70), ": negative mask stride (350, 0, -70)"),
           (dict(mask=O + 1), ": out overlaps mask"), (dict(mask=W + 100), ": workspace overlaps mask"),
           # the pages' own
           (dict(page=0), PAGE % 0), (dict(page=100), PAGE % 100), (dict(n_pages=-1), PAGES), (dict(table_len=-1), PAGES),
           (dict(table_len=2 ** 60), ": table_len*page overflows"), (dict(max_S=193), ": max_S=193 keys exceed table_len*page=192"),
           (dict(n_pages=2 ** 31 - 1, page=2 ** 30, table_len=1), ": n_pages*n_kv*page*pitch overflows"),
           (dict(table=None), ": null pointer"), (dict(lens=None), ": null pointer"),
           (dict(table=TAB + 2), ": block_table and seq_lens must be 4-byte aligned"),
           (dict(lens=LEN + 3), ": block_table and seq_lens must be 4-byte aligned"),
           (dict(table=O + 8), ": out overlaps block_table"), (dict(lens=W + 32), ": workspace overlaps seq_lens")]
    refused(lib, call, [(kw, name + text) for kw, text in bad], name)
    for kw in (dict(B=0), dict(T=0)):
        assert call(q=None, kd=None, ks=None, vd=None, vs=None, table=None, lens=None, ws=None, ws_bytes=0, out=None, **kw) == _lib.MDG_OK, kw
