"""CPU: mdg_attn_fwd_kv8 checks its arguments without a device, with a message before any device work; an empty call returns MDG_OK
whatever the pointers."""
from modegpt_amd import _lib
from tests.test_attn_fwd_host import O, Q, refused
from tests.test_kv8_host import KD, KS, M, VD, VS

SM = 0x700000                                                                                     # a summary; never dereferenced


def test_fwd_kv8_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    name = "mdg_attn_fwd_kv8"
    need = lib.mdg_attn_mask_summary_bytes(2, 1, 5, 9)

    def call(q=Q, kd=KD, ks=KS, vd=VD, vs=VS, dtype=_lib.MDG_BF16, B=2, T=5, S=9, n_heads=4, n_kv=2, r_qk=6, r_vo=3, cap=12, kp=16, vp=16,
             scale=0.5, causal=1, out=O, ld_out=12, mask=None, Hm=1, mbs=45, mhs=0, mqs=9, summary=SM, summary_bytes=need):
        return lib.mdg_attn_fwd_kv8(q, kd, ks, vd, vs, dtype, B, T, S, n_heads, n_kv, r_qk, r_vo, cap, kp, vp, scale, causal, out, ld_out,
                                    None, mask, Hm, mbs, mhs, mqs, summary, summary_bytes)

    pitches = ": pitches (%d, %d) must be multiples of 16 and >= mdg_kv8_pitch of r_qk=%d, r_vo=%d"
    aligned = ": data must be 16-byte and scales 4-byte aligned"
    bad = [  # what mdg_attn_fwd refuses, in its words
           (dict(dtype=_lib.MDG_F32), ": dtype 2 (bf16 or f16; fp32 inputs are out of scope)"), (dict(S=-1), ": negative extent"),
           (dict(n_kv=3), ": n_heads=4 is not a positive multiple of n_kv=3"), (dict(r_qk=7), ": r_qk=7 must be even, >= 2 and <= 256"),
           (dict(r_vo=257, vp=272), ": r_vo=257 must be in 1..256"), (dict(S=3), ": causal with S=3 < T=5 keys"),
           (dict(ld_out=11), ": ld_out=11 < n_heads*r_vo=12"), (dict(scale=0.0), ": scale 0 must be finite and positive"),
           (dict(B=2 ** 60), ": B*T overflows"), (dict(q=None), ": null pointer"), (dict(out=None), ": null pointer"),
           (dict(q=O + 2), ": out overlaps q"),
           # the cache's own, as mdg_attn_decode_kv8 refuses them
           (dict(S=13), ": S=13 keys exceed cap=12"), (dict(cap=-1), ": S=9 keys exceed cap=-1"),
           (dict(kp=8), pitches % (8, 16, 6, 3)), (dict(vp=24), pitches % (16, 24, 6, 3)), (dict(r_qk=18), pitches % (16, 16, 18, 3)),
           (dict(r_vo=17), pitches % (16, 16, 6, 17)),
           (dict(kd=None), ": null pointer"), (dict(ks=None), ": null pointer"), (dict(vd=None), ": null pointer"), (dict(vs=None), ": null pointer"),
           (dict(kd=KD + 4), aligned), (dict(vd=VD + 8), aligned), (dict(ks=KS + 1), aligned), (dict(vs=VS + 2), aligned),
           (dict(kd=O - 16), ": out overlaps k data"), (dict(ks=O + 236), ": out overlaps k scale"),
           (dict(vd=O + 16), ": out overlaps v data"), (dict(vs=O + 4), ": out overlaps v scale"),
           # the mask and its summary: mdg_attn_fwd_masked's checks, and the planes against the summary
           (dict(mask=M, Hm=2), ": mask heads Hm=2 must be 1 or n_heads=4"), (dict(mask=M, mqs=-9), ": negative mask stride (45, 0, -9)"),
           (dict(mask=M, summary=None), ": null summary"),
           (dict(mask=M, summary_bytes=need - 1), ": summary of %d bytes is short of mdg_attn_mask_summary_bytes = %d" % (need - 1, need)),
           (dict(mask=M, summary=O + 238), ": out overlaps summary"), (dict(mask=O + 1), ": out overlaps mask"),
           (dict(mask=M, summary=M + 89), ": summary overlaps mask"), (dict(mask=M, summary=Q), ": summary overlaps q"),
           (dict(mask=M, summary=KD + 766), ": summary overlaps k data"), (dict(mask=M, summary=KS), ": summary overlaps k scale"),
           (dict(mask=M, summary=VD + 100), ": summary overlaps v data"), (dict(mask=M, summary=VS + 190), ": summary overlaps v scale")]
    refused(lib, call, [(kw, name + text) for kw, text in bad], name)
    for kw in (dict(B=0), dict(T=0)):
        assert call(q=None, kd=None, ks=None, vd=None, vs=None, out=None, summary=None, **kw) == _lib.MDG_OK, kw
