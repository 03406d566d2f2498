"""CPU: the fp8 KV cache entries (mdg_kv8_pitch, mdg_kv8_append, mdg_kv8_dequant, mdg_attn_decode_kv8) check their arguments without a
device, with a message before any device work; an empty call returns MDG_OK whatever the pointers."""
from modegpt_amd import _lib
from tests.test_attn_decode_host import NEED, W
from tests.test_attn_fwd_host import O, Q, refused

SRC, KD, KS, VD, VS, M = 0x100000, 0x200000, 0x280000, 0x300000, 0x380000, 0x600000      # never dereferenced


def test_pitch_is_the_width_rounded_up_to_16():
    f = _lib.load().mdg_kv8_pitch
    assert [f(r) for r in (1, 2, 15, 16, 17, 77, 90, 128, 255, 256)] == [16, 16, 16, 16, 32, 80, 96, 128, 256, 256]
    assert f(0) == 0 and f(-3) == 0


def test_append_and_dequant_refuse_bad_arguments_without_a_device():
    lib = _lib.load()

    def append(src=SRC, dtype=_lib.MDG_BF16, B=2, n_kv=2, T=5, r=77, sbs=2 * 5 * 77, shs=5 * 77, sts=77, data=KD, scale=KS, cap=32,
               pitch=80, pos=3):
        return lib.mdg_kv8_append(src, dtype, B, n_kv, T, r, sbs, shs, sts, data, scale, cap, pitch, pos, None)

    def dequant(data=KD, scale=KS, dtype=_lib.MDG_BF16, B=2, n_kv=2, S=9, r=77, cap=32, pitch=80, out=O):
        return lib.mdg_kv8_dequant(data, scale, dtype, B, n_kv, S, r, cap, pitch, out, None)

    pitch = ": pitch=%d must be a multiple of 16 and >= mdg_kv8_pitch(77) = 80"
    for name, call, own in (
            ("mdg_kv8_append", append,
             [(dict(T=-1), ": negative extent"), (dict(pos=28), ": pos=28 + T=5 rows exceed cap=32"), (dict(pos=-1), ": pos=-1 + T=5 rows exceed cap=32"),
              (dict(T=33, pos=0), ": pos=0 + T=33 rows exceed cap=32"), (dict(src=None), ": null pointer"),
              (dict(src=KD + 100), ": data overlaps src"), (dict(src=KS + 8), ": scale overlaps src"), (dict(scale=KD + 64), ": data overlaps scale")]),
            ("mdg_kv8_dequant", dequant,
             [(dict(S=-1), ": negative extent"), (dict(S=33), ": S=33 rows exceed cap=32"), (dict(out=None), ": null pointer"),
              (dict(out=KD + 2 * 2 * 32 * 80 - 2), ": data overlaps out"), (dict(out=KS - 2), ": scale overlaps out")])):
        shared = [(dict(dtype=_lib.MDG_F32), ": dtype 2 (bf16 or f16)"), (dict(B=-1), ": negative extent"), (dict(n_kv=-2), ": negative extent"),
                  (dict(cap=-1), ": negative extent"), (dict(r=0), ": r=0 must be in 1..256"), (dict(r=257, pitch=272), ": r=257 must be in 1..256"),
                  (dict(pitch=64), pitch % 64), (dict(pitch=88), pitch % 88), (dict(data=None), ": null pointer"), (dict(scale=None), ": null pointer"),
                  (dict(data=KD + 8), ": data must be 16-byte and scale 4-byte aligned"), (dict(scale=KS + 2), ": data must be 16-byte and scale 4-byte aligned")]
        refused(lib, call, [(kw, name + text) for kw, text in shared + own], name)
        for kw in (dict(B=0), dict(n_kv=0), dict(T=0, pos=32) if call is append else dict(S=0)):      # empty: nothing is launched
            assert call(**{**dict(data=None, scale=None), **kw}) == _lib.MDG_OK, (name, kw)


def test_decode_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    name = "mdg_attn_decode_kv8"

    def call(q=Q, kd=KD, ks=KS, vd=VD, vs=VS, dtype=_lib.MDG_BF16, B=2, T=5, S=9, n_heads=4, n_kv=2, r_qk=6, r_vo=3, cap=12, kp=16, vp=16,
             scale=0.5, causal=1, splits=3, ws=W, ws_bytes=NEED, out=O, ld_out=12, mask=None, Hm=1, mbs=45, mhs=0, mqs=9):
        return lib.mdg_attn_decode_kv8(q, kd, ks, vd, vs, dtype, B, T, S, n_heads, n_kv, r_qk, r_vo, cap, kp, vp, scale, causal, splits, ws,
                                       ws_bytes, out, ld_out, None, mask, Hm, mbs, mhs, mqs)

    pitches = ": pitches (%d, %d) must be multiples of 16 and >= mdg_kv8_pitch of r_qk=%d, r_vo=%d"
    aligned = ": data must be 16-byte and scales 4-byte aligned"
    bad = [  # what mdg_attn_decode refuses, in its words
           (dict(dtype=_lib.MDG_F32), ": dtype 2 (bf16 or f16; fp32 inputs are out of scope)"), (dict(S=-1), ": negative extent"),
           (dict(n_kv=3), ": n_heads=4 is not a positive multiple of n_kv=3"), (dict(r_qk=7), ": r_qk=7 must be even, >= 2 and <= 256"),
           (dict(r_vo=257, vp=272), ": r_vo=257 must be in 1..256"),
           (dict(T=17, S=20, cap=20), ": T=17 queries x group of 2 heads exceed the tile of 32 columns"),
           (dict(splits=0), ": splits=0 must be in 1..256"), (dict(splits=257), ": splits=257 must be in 1..256"),
           (dict(S=3), ": causal with S=3 < T=5 keys"), (dict(ld_out=11), ": ld_out=11 < n_heads*r_vo=12"),
           (dict(scale=0.0), ": scale 0 must be finite and positive"), (dict(q=None), ": null pointer"), (dict(ws=None), ": null workspace"),
           (dict(ws_bytes=NEED - 1), ": workspace of %d bytes is short of mdg_attn_decode_ws_bytes = %d" % (NEED - 1, NEED)),
           (dict(ws=W + 8), ": workspace must be 16-byte aligned"), (dict(out=W + 64), ": workspace overlaps out"),
           (dict(q=O + 2), ": out overlaps q"), (dict(q=W + NEED - 2), ": workspace overlaps q"),
           # the cache's own
           (dict(S=13), ": S=13 keys exceed cap=12"), (dict(cap=-1), ": S=9 keys exceed cap=-1"),
           (dict(kp=8), pitches % (8, 16, 6, 3)), (dict(vp=24), pitches % (16, 24, 6, 3)), (dict(r_qk=18), pitches % (16, 16, 18, 3)),
           (dict(r_vo=17), pitches % (16, 16, 6, 17)),
           (dict(kd=None), ": null pointer"), (dict(ks=None), ": null pointer"), (dict(vd=None), ": null pointer"), (dict(vs=None), ": null pointer"),
           (dict(kd=KD + 4), aligned), (dict(vd=VD + 8), aligned), (dict(ks=KS + 1), aligned), (dict(vs=VS + 2), aligned),
           (dict(kd=O - 16), ": out overlaps k data"), (dict(ks=W + 16), ": workspace overlaps k scale"),
           (dict(vd=W + NEED - 16), ": workspace overlaps v data"), (dict(vs=O + 4), ": out overlaps v scale"),
           # the mask: mdg_attn_decode_masked's checks
           (dict(mask=M, Hm=2), ": mask heads Hm=2 must be 1 or n_heads=4"), (dict(mask=M, mqs=-9), ": negative mask stride (45, 0, -9)"),
           (dict(mask=O + 1), ": out overlaps mask"), (dict(mask=W + 100), ": workspace overlaps mask")]
    refused(lib, call, [(kw, name + text) for kw, text in bad], name)
    for kw in (dict(B=0), dict(T=0)):
        assert call(q=None, kd=None, ks=None, vd=None, vs=None, ws=None, ws_bytes=0, out=None, **kw) == _lib.MDG_OK, kw
